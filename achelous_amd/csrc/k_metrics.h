// k_metrics.h — the per-batch half of the reference's per-epoch evaluation, without a host read:
//   confusion  utils_seg/utils_metrics.py:31-33 `fast_hist` (and utils_seg_pc/utils_metrics.py `mean_iou`'s counts) with the arg-max over the classes fused in:
//              hist[n * label + pred] += 1 into a device-resident uint64 [n, n] that the kernel adds to and never clears.  A pixel counts only if 0 <= label < n.
//   match      utils/utils_map.py:462-498 in its parallel form, one workgroup per image: for every detection the best same-class ground-truth box of its image
//              (float64 IoU with the +1 pixel convention, first box reaching the maximum wins) and, for up to 10 IoU thresholds at once, tp / fp / ignored.
// Everything here is integer arithmetic or an ordering decision: integer adds do not depend on their order, so the histogram is bit-identical from run to run
// and independent of the grid; the IoU is float64 in the reference's order of operations with contraction off.
// Arg-max: the LOWEST class index among equal values wins (numpy / torch.argmax).  NaN logits: unspecified (a NaN never compares greater, so it is never chosen
// unless it is class 0's value; torch would choose it).  A class-map value >= n is dropped, like a label outside 0..n-1.
#pragma once
#include "ach_platform.h"
#include "k_train2.h"

namespace ach {

constexpr int CONF_MAXN = 16;        // classes: n * n <= 256 bins, one uint32 copy per wave in LDS
constexpr int CONF_BLOCKS = 1024;    // grid-stride above this many workgroups
enum ConfPred : int { CONF_F32 = 0, CONF_BF16 = 1, CONF_F16 = 2, CONF_MAP_U8 = 3 };

struct ConfusionParams {
    const void* pred; int layout;            // logits [B, n, HW] (layout 0) or [B, HW, n] (layout 1), or a uint8 class map [B, HW]
    const void* lab; int lab_kind;           // [B, HW]; 0 int64, 1 int32, 2 uint8 (the encoding of ach_train_seg_loss)
    int B, n; long HW;
    unsigned long long* hist;                // [n, n], row = label, column = prediction
};

struct conf_u8 {};                           // tag: the prediction is a ready class map

// V consecutive labels at element offset i (16-byte loads for the 4- and 8-byte kinds when V > 1; i is then a multiple of V and the base 16-byte aligned)
template <int V> __device__ __forceinline__ void conf_labels(const ConfusionParams& p, long i, long long (&L)[V]) {
    if constexpr (V == 1) {
        if (p.lab_kind == 0) L[0] = static_cast<const long long*>(p.lab)[i];
        else if (p.lab_kind == 1) L[0] = static_cast<const int*>(p.lab)[i];
        else L[0] = static_cast<const unsigned char*>(p.lab)[i];
    } else if (p.lab_kind == 0) {
        const uint4* q = reinterpret_cast<const uint4*>(static_cast<const long long*>(p.lab) + i);
        ACH_UNROLL
        for (int k = 0; k < V / 2; ++k) {
            const uint4 t = q[k];
            L[2 * k] = (long long)((unsigned long long)(t.y) << 32 | t.x);
            L[2 * k + 1] = (long long)((unsigned long long)(t.w) << 32 | t.z);
        }
    } else if (p.lab_kind == 1) {
        const uint4* q = reinterpret_cast<const uint4*>(static_cast<const int*>(p.lab) + i);
        ACH_UNROLL
        for (int k = 0; k < V / 4; ++k) {
            const uint4 t = q[k];
            L[4 * k] = int(t.x); L[4 * k + 1] = int(t.y); L[4 * k + 2] = int(t.z); L[4 * k + 3] = int(t.w);
        }
    } else {
        const unsigned* q = reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(p.lab) + i);
        ACH_UNROLL
        for (int k = 0; k < V / 4; ++k) {
            const unsigned t = q[k];
            L[4 * k] = t & 0xffu; L[4 * k + 1] = (t >> 8) & 0xffu; L[4 * k + 2] = (t >> 16) & 0xffu; L[4 * k + 3] = t >> 24;
        }
    }
}

// V consecutive logits of one class
template <class T, int V> __device__ __forceinline__ void conf_vals(const T* q, float (&o)[V]) {
    if constexpr (V == 1) o[0] = Store<T>::ld(q);
    else if constexpr (V == 4) Store<T>::ld4(q, o);
    else Store<T>::ld8(q, o);
}

// the predicted class of V consecutive pixels of image b starting at pixel q (layout 1: V == 1, the classes of a point are consecutive)
template <class T, int V> __device__ __forceinline__ void conf_pred(const ConfusionParams& p, long b, long q, int (&arg)[V]) {
    if constexpr (std::is_same<T, conf_u8>::value) {
        const unsigned char* m = static_cast<const unsigned char*>(p.pred) + b * p.HW + q;
        if constexpr (V == 1) arg[0] = m[0];
        else {
            const unsigned* w = reinterpret_cast<const unsigned*>(m);
            ACH_UNROLL
            for (int k = 0; k < V / 4; ++k) {
                const unsigned t = w[k];
                arg[4 * k] = t & 0xffu; arg[4 * k + 1] = (t >> 8) & 0xffu; arg[4 * k + 2] = (t >> 16) & 0xffu; arg[4 * k + 3] = t >> 24;
            }
        }
    } else {
        const T* x = static_cast<const T*>(p.pred);
        float best[V], cur[V];
        if (p.layout == 0) {
            const T* xb = x + b * p.n * p.HW + q;
            conf_vals<T, V>(xb, best);
            ACH_UNROLL
            for (int v = 0; v < V; ++v) arg[v] = 0;
            for (int c = 1; c < p.n; ++c) {
                conf_vals<T, V>(xb + long(c) * p.HW, cur);
                ACH_UNROLL
                for (int v = 0; v < V; ++v) if (cur[v] > best[v]) { best[v] = cur[v]; arg[v] = c; }        // strict: the lowest index keeps a tie
            }
        } else {
            const T* xb = x + (b * p.HW + q) * p.n;
            best[0] = Store<T>::ld(xb); arg[0] = 0;
            for (int c = 1; c < p.n; ++c) {
                const float t = Store<T>::ld(xb + c);
                if (t > best[0]) { best[0] = t; arg[0] = c; }
            }
        }
    }
}

// Every lane of a workgroup runs the same number of iterations (the wave-level combine below is a collective).  The realistic label map is the worst one for
// LDS atomics — nearly every pixel is water, all 64 lanes add to one bin — so a wave whose lanes all hit the same bin adds 64 once from lane 0.
template <class T, int V>
static __global__ __launch_bounds__(256) void confusion_kernel(const ConfusionParams p) {
    __shared__ unsigned s_bins[4][CONF_MAXN * CONF_MAXN];
    const int n = p.n, nn = n * n, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 4 * CONF_MAXN * CONF_MAXN; i += 256) (&s_bins[0][0])[i] = 0u;
    __syncthreads();
    const long per = p.HW / V, items = long(p.B) * per, stride = long(gridDim.x) * 256;
    const long iters = (items + stride - 1) / stride;
    for (long k = 0; k < iters; ++k) {
        const long it = k * stride + long(blockIdx.x) * 256 + threadIdx.x;
        int bin[V];
        ACH_UNROLL
        for (int v = 0; v < V; ++v) bin[v] = -1;
        if (it < items) {
            const long b = tdiv(it, per), q = (it - b * per) * V;
            long long L[V];
            int arg[V];
            conf_labels<V>(p, b * p.HW + q, L);
            conf_pred<T, V>(p, b, q, arg);
            ACH_UNROLL
            for (int v = 0; v < V; ++v) if (L[v] >= 0 && L[v] < n && arg[v] < n) bin[v] = int(L[v]) * n + arg[v];
        }
        ACH_UNROLL
        for (int v = 0; v < V; ++v) {
            const int first = wave_lane_i32(bin[v], 0);
            if (wave_ballot64(bin[v] == first) == ~0ull) { if (lane == 0 && first >= 0) atomicAdd(&s_bins[wave][first], 64u); }
            else if (bin[v] >= 0) atomicAdd(&s_bins[wave][bin[v]], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nn; i += 256) {
        const unsigned long long t = (unsigned long long)(s_bins[0][i]) + s_bins[1][i] + s_bins[2][i] + s_bins[3][i];
        if (t) atomicAdd(p.hist + i, t);
    }
}

template <class T> static void confusion_launch(const ConfusionParams& p, bool vec, int nblk, hipStream_t s) {
    constexpr int V = (std::is_same<T, float>::value) ? 4 : 8;
    if (vec) ACH_LAUNCH((confusion_kernel<T, V>), dim3(unsigned(nblk)), dim3(256), s, p);
    else ACH_LAUNCH((confusion_kernel<T, 1>), dim3(unsigned(nblk)), dim3(256), s, p);
}
constexpr int conf_vec(int pred_kind) { return pred_kind == CONF_F32 ? 4 : 8; }

// ------------------------------------------------------------------------------------------ detection matching
constexpr int MATCH_MAXD = 1024;     // detections per image held in LDS
constexpr int MATCH_MAXG = 128;      // ground-truth boxes per image
constexpr int MATCH_MAXT = 10;       // IoU thresholds per launch
enum MatchFlag : int { MATCH_EMPTY = 0, MATCH_TP = 1, MATCH_FP = 2, MATCH_IGNORED = 3 };

struct MatchParams {
    const float* rows; const int* counts;            // [B, D, 7], [B]
    int yx_order, truncate;                          // columns (y1, x1, y2, x2, ...) instead of (x1, y1, x2, y2, ...); int() of the four coordinates
    const float* gt; const unsigned char* difficult; const int* gt_counts;      // [B, G, 5] (x1, y1, x2, y2, class), [B, G] or null, [B]
    int B, D, G, C, T;
    double thr[MATCH_MAXT];
    unsigned char* flags; int* match; double* iou; float* score;                // [T, B, D], [B, D], [B, D], [B, D]
    unsigned long long* gt_per_class;                // [C], added to
};

static __global__ __launch_bounds__(256) void match_kernel(const MatchParams p) {
    __shared__ double s_g[MATCH_MAXG][4];
    __shared__ int s_gc[MATCH_MAXG];
    __shared__ unsigned char s_gd[MATCH_MAXG];
    __shared__ double s_ov[MATCH_MAXD];
    __shared__ float s_sc[MATCH_MAXD];
    __shared__ int s_m[MATCH_MAXD];
    const int b = blockIdx.x, tid = threadIdx.x;
    int nd = p.counts[b], ng = p.gt_counts[b];
    nd = nd < 0 ? 0 : (nd > p.D ? p.D : nd);
    ng = ng < 0 ? 0 : (ng > p.G ? p.G : ng);
    for (int g = tid; g < ng; g += 256) {
        const float* q = p.gt + (long(b) * p.G + g) * 5;
        s_g[g][0] = double(q[0]); s_g[g][1] = double(q[1]); s_g[g][2] = double(q[2]); s_g[g][3] = double(q[3]);
        const int c = int(q[4]);
        const unsigned char d = p.difficult ? p.difficult[long(b) * p.G + g] : (unsigned char)0;
        s_gc[g] = c; s_gd[g] = d;
        if (!d && c >= 0 && c < p.C) atomicAdd(p.gt_per_class + c, 1ull);                 // utils_map.py:364-368
    }
    __syncthreads();
    for (int i = tid; i < p.D; i += 256) {
        const long o = long(b) * p.D + i;
        if (i >= nd) { p.match[o] = -1; p.iou[o] = -1.0; p.score[o] = 0.0f; continue; }
        const float* r = p.rows + o * 7;
        double bb[4];
        if (p.yx_order) { bb[0] = double(r[1]); bb[1] = double(r[0]); bb[2] = double(r[3]); bb[3] = double(r[2]); }
        else { bb[0] = double(r[0]); bb[1] = double(r[1]); bb[2] = double(r[2]); bb[3] = double(r[3]); }
        if (p.truncate) { bb[0] = trunc(bb[0]); bb[1] = trunc(bb[1]); bb[2] = trunc(bb[2]); bb[3] = trunc(bb[3]); }      // utils/callbacks.py:216-217
        const float sc = r[4] * r[5];
        const int cls = int(r[6]);
        double ovmax = -1.0;
        int m = -1;
        {
#if !defined(ACH_HOSTEMU)
#pragma clang fp contract(off)
#endif
            for (int g = 0; g < ng; ++g) {
                if (s_gc[g] != cls) continue;
                const double g0 = s_g[g][0], g1 = s_g[g][1], g2 = s_g[g][2], g3 = s_g[g][3];
                const double iw = fmin(bb[2], g2) - fmax(bb[0], g0) + 1.0, ih = fmin(bb[3], g3) - fmax(bb[1], g1) + 1.0;
                if (iw > 0.0 && ih > 0.0) {
                    const double inter = iw * ih;
                    const double ua = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (g2 - g0 + 1.0) * (g3 - g1 + 1.0) - inter;
                    const double ov = inter / ua;
                    if (ov > ovmax) { ovmax = ov; m = g; }
                }
            }
        }
        s_ov[i] = ovmax; s_sc[i] = sc; s_m[i] = m;
        p.match[o] = m; p.iou[o] = ovmax; p.score[o] = sc;
    }
    __syncthreads();
    for (int i = tid; i < p.D; i += 256) {
        const long o = long(b) * p.D + i;
        if (i >= nd) {
            for (int t = 0; t < p.T; ++t) p.flags[(long(t) * p.B + b) * p.D + i] = MATCH_EMPTY;
            continue;
        }
        const int m = s_m[i];
        const float sc = s_sc[i];
        const double ov = s_ov[i];
        // the largest overlap an EARLIER-ranked detection (score descending, then slot ascending) has with the same box: that one took the box at
        // every threshold it reaches (utils_map.py:485-487 `used`)
        double prev = -1.0;
        if (m >= 0) {
            for (int k = 0; k < nd; ++k) {
                if (s_m[k] != m) continue;
                const float sk = s_sc[k];
                if ((sk > sc || (sk == sc && k < i)) && s_ov[k] > prev) prev = s_ov[k];
            }
        }
        const bool diff = m >= 0 && s_gd[m] != 0;
        for (int t = 0; t < p.T; ++t) {
            const double thr = p.thr[t];
            int f;
            if (!(ov >= thr)) f = MATCH_FP;
            else if (diff) f = MATCH_IGNORED;
            else f = prev >= thr ? MATCH_FP : MATCH_TP;
            p.flags[(long(t) * p.B + b) * p.D + i] = (unsigned char)f;
        }
    }
}

}  // namespace ach
