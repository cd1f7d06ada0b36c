// k_heatmap.h — the reference's heat-map mode (achelous.detect_heatmap, achelous.py:451-555) for a whole ragged batch in THREE launches whatever the batch, from the
// detection maps a forward leaves on the device: per cell max_c sigmoid(cls) * sigmoid(obj), every level stretched to the frame's own size with cv2's INTER_LINEAR,
// truncated to uint8, the maximum over the levels (the mask), and the mask drawn over the frame through a colour map normalised to the mask's own range.
//
//   (a) heat_scores_kernel   det3 / det4 / det5 [B, 5 + num_det, R/s, R/s] (fp32, bf16 or fp16; s = 8, 16, 32) -> scores float32 [B, A], level-major,
//                            A = (R/8)^2 + (R/16)^2 + (R/32)^2.  sigma(x) = 1 / (1 + exp(-x)) in float32; sigma is monotone, so the class maximum is taken on the
//                            logits and ONE exp serves the classes.  A cell with a NaN logit scores 0 (our rule: numpy's cast of NaN to uint8 is undefined).  Channel
//                            planes are read coalesced across cells.  The launch also zeroes the per-frame statistics of (b): no memset.
//   (b) heat_mask_kernel     mask uint8 [H, W] per frame in a packed arena (frame starts and pitches multiples of 16; a thread owns 4 neighbouring pixels and stores
//                            one dword; pixels past W in that dword are zero): m = max_l uint8(trunc(resize_l(y, x) * 255.0f)).  A workgroup stages the frame's three
//                            score maps in LDS (A <= 4096 floats, 16 KB) and owns a HEAT_TW x HEAT_TH tile.  resize_l is INTER_LINEAR on the level's map: coordinate
//                            float((double(d) + 0.5) * sc + off - 0.5), floor, the two clamps with weight 0 (to the level's WHOLE extent), horizontal blend then
//                            vertical blend in float32 — the UNCONTRACTED sequence on the device as under the emulation (`#pragma clang fp contract(off)`; unlike
//                            k_serve.h this kernel has no contracted legacy kernel to mirror).  Per axis sc = double(nw) / (double(W) * double(s)), off = double(x0) /
//                            double(s), (y0, x0, nh, nw) the window of the R x R network input the frame covers.  With (0, 0, R, R) that is bit for bit the
//                            reference, which stretches the whole map over the frame.  Per-frame statistics int32 [B][2] = (max m, max 255 - m): wave64 reduction,
//                            one atomicMax per workgroup and word; lo = 255 - stats[1], hi = stats[0].
//   (c) heat_colour_kernel   each workgroup builds the frame's 256-entry RGB table in LDS: table[m] = cmap[idx(m)], idx(m) = min(int(((double)m - lo) / (hi - lo) *
//                            256.0), 255), 0 when hi == lo (matplotlib's Normalize(lo, hi) and Colormap.__call__(bytes=True) on 256 entries); then
//                            out = blend(base, table[m], alpha), blend(a, b, t) = (uint8)(a + t * (b - a)) in float32, not contracted (PIL's Image.blend, serve_mix).
//                            `base` is any packed HWC arena (any pitch >= 3 W), `out` an arena with 16-byte aligned frame starts and pitches — or the base itself.
//
//   frame table int64 [B][16]: 0 byte offset of the frame in the base arena, 1 H, 2 W, 3 base pitch, 4 y0, 5 x0, 6 nh, 7 nw, 8 byte offset of the mask in its arena,
//                9 mask pitch, 10 byte offset of the coloured frame in the out arena, 11 its pitch, 12-15 unused.
// The C entry (api_frames.cpp ach_heatmap_frames, declared in include/achelous_heatmap.h) checks every extent, pitch, alignment and window on the host before the first launch: the kernels trust the table.
#pragma once
#include "ach_platform.h"
#include "k_serve.h"       // ServeAxis, serve_mix

namespace ach {

constexpr int HEAT_TABLE_COLS = 16;
constexpr int HEAT_TW = 128, HEAT_TH = 64;    // a workgroup's tile: 32 threads x 4 pixels wide, 8 passes of 8 rows
constexpr int HEAT_MAX_CELLS = 4096;          // a frame's three score maps in LDS (R <= 416: 3549)

__host__ __device__ __forceinline__ int heat_cells(int R) { return (R / 8) * (R / 8) + (R / 16) * (R / 16) + (R / 32) * (R / 32); }

// one axis of INTER_LINEAR with the window's offset, every operation rounded on its own
__host__ __device__ __forceinline__ ServeAxis heat_axis(int d, double sc, double off, int n) {
#pragma clang fp contract(off)
    const double t = (double(d) + 0.5) * sc;
    const double u = t + off;
    float f = float(u - 0.5);
    int i = int(floorf(f));
    f -= float(i);
    if (i < 0) { i = 0; f = 0.f; }
    if (i >= n - 1) { i = n - 1; f = 0.f; }
    ServeAxis a;
    a.i0 = i; a.i1 = i + 1 < n ? i + 1 : i; a.f = f;
    return a;
}
__host__ __device__ __forceinline__ float heat_blend(float p, float q, float w0, float w1) {      // p * w0 + q * w1, two rounded products and an add
#pragma clang fp contract(off)
    const float x = p * w0, y = q * w1;
    return x + y;
}

struct HeatScoreParams {
    const void* det[3];
    float* scores; int* stats;
    int R, num_det, A;
};

template <class T>
static __global__ __launch_bounds__(256) void heat_scores_kernel(const HeatScoreParams p) {
#pragma clang fp contract(off)
    const long b = blockIdx.y;
    const int a = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (blockIdx.x == 0 && threadIdx.x < 2) p.stats[2 * b + threadIdx.x] = 0;
    if (a >= p.A) return;
    const int n0 = (p.R / 8) * (p.R / 8), n1 = (p.R / 16) * (p.R / 16), n2 = (p.R / 32) * (p.R / 32);
    const int level = a < n0 ? 0 : a < n0 + n1 ? 1 : 2;
    const int cell = level == 0 ? a : level == 1 ? a - n0 : a - n0 - n1;
    const long n = level == 0 ? n0 : level == 1 ? n1 : n2;
    const T* x = static_cast<const T*>(p.det[level]) + b * (5 + p.num_det) * n + cell;
    const float obj = Store<T>::ld(x + 4 * n);
    bool bad = obj != obj;
    float best = Store<T>::ld(x + 5 * n);
    bad = bad || best != best;
    for (int c = 1; c < p.num_det; ++c) {
        const float v = Store<T>::ld(x + (5 + c) * n);
        bad = bad || v != v;
        best = v > best ? v : best;
    }
    const float sc = 1.0f / (1.0f + expf(-best)), so = 1.0f / (1.0f + expf(-obj));
    p.scores[b * p.A + a] = bad ? 0.f : sc * so;
}

struct HeatParams {
    const float* scores; int* stats;
    const uint8_t* base; const long long* table; const uint8_t* cmap;
    uint8_t* mask; uint8_t* out;
    int R, A;
    float alpha;
};

static __global__ __launch_bounds__(256) void heat_mask_kernel(const HeatParams p) {
#pragma clang fp contract(off)
    __shared__ float sc[HEAT_MAX_CELLS];
    __shared__ int red[8];
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const long long* f = p.table + b * HEAT_TABLE_COLS;
    const int H = int(f[1]), W = int(f[2]), y0 = int(f[4]), x0 = int(f[5]), nh = int(f[6]), nw = int(f[7]);
    const int ntx = (W + HEAT_TW - 1) / HEAT_TW, nty = (H + HEAT_TH - 1) / HEAT_TH;
    if (long(blockIdx.x) >= long(ntx) * nty) return;                     // (the whole workgroup: the grid is sized for the batch's largest frame)
    const int ty = int(blockIdx.x) / ntx, oy0 = ty * HEAT_TH, ox0 = (int(blockIdx.x) - ty * ntx) * HEAT_TW;
    for (int i = tid; i < p.A; i += 256) sc[i] = p.scores[b * p.A + i];
    __syncthreads();
    const int x4 = ox0 + 4 * (tid & 31);
    const int npx = x4 >= W ? 0 : W - x4 < 4 ? W - x4 : 4;
    // the thread's four columns on the three levels: computed once, kept for every row
    ServeAxis ax[3][4];
    int base_l[3], n_l[3];
    double sy[3], oy[3];
    {
        int at = 0;
        ACH_UNROLL
        for (int l = 0; l < 3; ++l) {
            const int s = 8 << l, n = p.R / s;
            const double sx = double(nw) / (double(W) * double(s)), ox = double(x0) / double(s);
            sy[l] = double(nh) / (double(H) * double(s));
            oy[l] = double(y0) / double(s);
            base_l[l] = at; n_l[l] = n;
            at += n * n;
            ACH_UNROLL
            for (int i = 0; i < 4; ++i) ax[l][i] = heat_axis(x4 + i < W ? x4 + i : W - 1, sx, ox, n);
        }
    }
    int hi = 0, nlo = 0;                                                 // max m, max 255 - m over this thread's pixels
    const int y_end = oy0 + HEAT_TH < H ? oy0 + HEAT_TH : H;
    if (npx > 0)
        for (int dy = oy0 + (tid >> 5); dy < y_end; dy += 8) {
            int m[4] = {0, 0, 0, 0};
            ACH_UNROLL
            for (int l = 0; l < 3; ++l) {
                const ServeAxis ay = heat_axis(dy, sy[l], oy[l], n_l[l]);
                const float ay0 = 1.f - ay.f;
                const float* top = sc + base_l[l] + ay.i0 * n_l[l];
                const float* bot = sc + base_l[l] + ay.i1 * n_l[l];
                ACH_UNROLL
                for (int i = 0; i < 4; ++i) {
                    const ServeAxis& a = ax[l][i];
                    const float a0 = 1.f - a.f;
                    const float t = heat_blend(top[a.i0], top[a.i1], a0, a.f), u = heat_blend(bot[a.i0], bot[a.i1], a0, a.f);
                    const float v = heat_blend(t, u, ay0, ay.f) * 255.0f;
                    int q = int(v);                                      // truncation; the scores lie in [0, 1], the clamp is for safety only
                    q = q < 0 ? 0 : q > 255 ? 255 : q;
                    m[i] = q > m[i] ? q : m[i];
                }
            }
            ACH_UNROLL
            for (int i = 0; i < 4; ++i) {
                if (i >= npx) { m[i] = 0; continue; }                    // past the row's end: the padding gets zeros
                hi = m[i] > hi ? m[i] : hi;
                nlo = 255 - m[i] > nlo ? 255 - m[i] : nlo;
            }
            *reinterpret_cast<uint32_t*>(p.mask + f[8] + long(dy) * f[9] + x4) = uint32_t(m[0]) | uint32_t(m[1]) << 8 | uint32_t(m[2]) << 16 | uint32_t(m[3]) << 24;
        }
    // the tile's two maxima: wave64 reduction, then one atomicMax per workgroup and word
    ACH_UNROLL
    for (int d = 32; d >= 1; d >>= 1) {
        const int h2 = __shfl_xor(hi, d), n2 = __shfl_xor(nlo, d);
        hi = h2 > hi ? h2 : hi;
        nlo = n2 > nlo ? n2 : nlo;
    }
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = hi; red[2 * (tid >> 6) + 1] = nlo; }
    __syncthreads();
    if (tid < 2) {
        int v = red[tid];
        for (int w = 1; w < 4; ++w) v = red[2 * w + tid] > v ? red[2 * w + tid] : v;
        atomicMax(p.stats + 2 * b + tid, v);
    }
}

static __global__ __launch_bounds__(256) void heat_colour_kernel(const HeatParams p) {
#pragma clang fp contract(off)
    __shared__ uint32_t lut[256];                                        // r | g << 8 | b << 16 per mask value
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const long long* f = p.table + b * HEAT_TABLE_COLS;
    const int H = int(f[1]), W = int(f[2]);
    const int ntx = (W + HEAT_TW - 1) / HEAT_TW, nty = (H + HEAT_TH - 1) / HEAT_TH;
    if (long(blockIdx.x) >= long(ntx) * nty) return;
    const int ty = int(blockIdx.x) / ntx, oy0 = ty * HEAT_TH, ox0 = (int(blockIdx.x) - ty * ntx) * HEAT_TW;
    {
        const int hi = p.stats[2 * b], lo = 255 - p.stats[2 * b + 1];
        int idx = 0;
        if (hi > lo) {
            const double r = (double(tid) - double(lo)) / double(hi - lo);
            const double x = r * 256.0;
            idx = x <= 0.0 ? 0 : x >= 255.0 ? 255 : int(x);
        }
        lut[tid] = uint32_t(p.cmap[3 * idx]) | uint32_t(p.cmap[3 * idx + 1]) << 8 | uint32_t(p.cmap[3 * idx + 2]) << 16;
    }
    __syncthreads();
    const int x4 = ox0 + 4 * (tid & 31);
    if (x4 >= W) return;
    const int npx = W - x4 < 4 ? W - x4 : 4;
    const int y_end = oy0 + HEAT_TH < H ? oy0 + HEAT_TH : H;
    for (int dy = oy0 + (tid >> 5); dy < y_end; dy += 8) {
        const uint32_t m4 = *reinterpret_cast<const uint32_t*>(p.mask + f[8] + long(dy) * f[9] + x4);
        // the 3 * npx base bytes start at any byte: aligned dwords (the arena is 4-byte aligned and padded, a dword that holds a needed byte is inside it)
        const long a = f[0] + long(dy) * f[3] + 3L * x4, A = a & ~3L;
        const int nbytes = 3 * npx, sh = int(a & 3) * 8;
        uint32_t w[4], in[3], out[3] = {0u, 0u, 0u};
        ACH_UNROLL
        for (int k = 0; k < 4; ++k) w[k] = A + 4 * k < a + nbytes ? *reinterpret_cast<const uint32_t*>(p.base + A + 4 * k) : 0u;
        ACH_UNROLL
        for (int k = 0; k < 3; ++k) in[k] = sh ? (w[k] >> sh) | (w[k + 1] << (32 - sh)) : w[k];
        ACH_UNROLL
        for (int i = 0; i < 4; ++i) {
            if (i >= npx) break;
            const uint32_t rgb = lut[(m4 >> (8 * i)) & 0xffu];
            ACH_UNROLL
            for (int ch = 0; ch < 3; ++ch) {
                const int j = 3 * i + ch;
                const int v = int((in[j >> 2] >> (8 * (j & 3))) & 0xffu);
                const int o = int(serve_mix(float(v), p.alpha, float(int((rgb >> (8 * ch)) & 0xffu) - v)));
                out[j >> 2] |= uint32_t(o) << (8 * (j & 3));
            }
        }
        uint32_t* o = reinterpret_cast<uint32_t*>(p.out + f[10] + long(dy) * f[11] + 3L * x4);
        ACH_UNROLL
        for (int k = 0; k < 3; ++k)
            if (4 * k < nbytes) o[k] = out[k];
    }
}

}  // namespace ach
