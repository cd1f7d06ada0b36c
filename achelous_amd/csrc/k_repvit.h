// k_repvit.h — the RepViT backbone (backbone/vision/repvit_modules/repvit.py, repvit_m1 / m2 / m3), every BatchNorm folded on the host (Engine::repvit):
//
//     stem          : conv3x3 s2 p1 (3 -> C0/2) + b, GELU                                   rv_stem_kernel (from the caller's NCHW image)
//                     conv3x3 s2 p1 (C0/2 -> C0) + b                                        the implicit GEMM (k_gemm.h)
//     stride-1 block: d = dw3x3(x) + b          (RepVGGDW: 3x3 + 1x1 + identity in ONE kernel)  rv_dw3_kernel<T, 1, SE>
//                     g = sigmoid(fc2(relu(fc1(mean_hw(d)))))      only in SE blocks          rv_gate_kernel
//                     y = g.d + W2 GELU(W1 (g.d) + b1) + b2         hidden 2C                  rv_mlp_kernel
//     stride-2 block: t = dw3x3 s2 (x) + b ; t = W t + b (inp -> oup) ; y = t + MLP(t)        rv_dw3_kernel<T, 2, false>, GEMM, rv_mlp_kernel
//
// SqueezeExcite needs a per-sample, per-channel mean over the whole map between two launches.  Scheme (no atomics, deterministic, batch-invariant; the one
// k_poolformer.h uses for GroupNorm(1)): every workgroup of the depthwise kernel owns a band of rows of ONE sample and writes one fp32 sum per channel of the
// values it stored — taken from the values AS STORED in T — into a table [sample][band][C]; the gate kernel adds a sample's bands in band order.  The
// band height depends on the map alone and grids are (bands or tiles, sample), so a frame's result is bit-identical whatever batch it sits in.
#pragma once
#include "ach_platform.h"
#include "k_gemm.h"
#include "k_mlp.h"

namespace ach {

// ------------------------------------------------------------------------------------------ stem, first conv
// conv 3x3 / stride 2 / pad 1, 3 -> 16 channels + bias + GELU, gathered from the NCHW image, NHWC out (16 channels per pixel).  27 x 16 multiply-adds per
// pixel: a thread owns a pixel, weights [27][16] + bias [16] in LDS (read at wave-uniform addresses).  grid (cdiv(Ho * Wo, 256), B)
constexpr int RV_STEM_C = 16;
struct RvStemParams { const void* X; void* Y; const float* w; int H, W, Ho, Wo; };        // w: [27][16] (k = (c * 3 + dy) * 3 + dx), then bias [16]
template <class T, class IO>
__global__ __launch_bounds__(256) void rv_stem_kernel(const RvStemParams p) { f16_sat_mode<T>();
    __shared__ float wl[28 * RV_STEM_C];
    for (int i = threadIdx.x; i < 28 * RV_STEM_C; i += 256) wl[i] = p.w[i];
    __syncthreads();
    const int b = blockIdx.y, px = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (px >= p.Ho * p.Wo) return;
    const int oy = px / p.Wo, ox = px - oy * p.Wo;
    const IO* X = static_cast<const IO*>(p.X) + long(b) * 3 * p.H * p.W;
    float acc[RV_STEM_C];
    ACH_UNROLL
    for (int n = 0; n < RV_STEM_C; ++n) acc[n] = wl[27 * RV_STEM_C + n];
    ACH_NO_UNROLL                           // (fully unrolled, the compiler hoists all 432 weight reads: 256 registers)
    for (int c = 0; c < 3; ++c) {
        ACH_NO_UNROLL
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = 2 * oy - 1 + dy;
            ACH_UNROLL
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = 2 * ox - 1 + dx;
                const bool in = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                const float v = in ? Store<IO>::ld(X + (long(c) * p.H + iy) * p.W + ix) : 0.f;
                const float* wr = wl + ((c * 3 + dy) * 3 + dx) * RV_STEM_C;
                ACH_UNROLL
                for (int n = 0; n < RV_STEM_C; ++n) acc[n] += v * wr[n];
            }
        }
    }
    apply_act_n<T, RV_STEM_C, ACT_GELU>(acc, ACT_GELU);
    T* y = static_cast<T*>(p.Y) + (long(b) * p.Ho * p.Wo + px) * RV_STEM_C;
    float o[8];
    ACH_UNROLL
    for (int h = 0; h < 2; ++h) {
        ACH_UNROLL
        for (int i = 0; i < 8; ++i) o[i] = acc[h * 8 + i];
        Store<T>::st8(y + h * 8, o);
    }
}

// ------------------------------------------------------------------------------------------ depthwise 3x3 (+ SE partial sums)
// y = dw3x3(x) + bias, stride 1 or 2, pad 1; weights [9][C] fp32 with every BatchNorm (and, stride 1, the 1x1 branch and the identity) folded in.
// A workgroup owns a band of RB OUTPUT rows of one sample; a thread owns one (output column, 16-byte channel piece) — its channel piece is fixed, so its nine
// weight vectors stay in registers — and walks down the band.  Stride 1: every input row is fetched once per band (its own column and the two beside it, which
// the neighbouring threads fetch too: L1) and added into the three output rows it belongs to, which are kept as running sums; the two halo rows of a band
// are the only re-reads.  An output row's sum is always taken in the order (row above, own row, row below), whatever the band: bit-identical for any band height.
// SE: the workgroup's per-channel sum of the values as stored goes to psum[(sample * bands + band) * C + c].        grid (cdiv(Ho, RB), B)
struct RvDwParams { const void* X; long ldx; void* Y; long ldy; const float* w; const float* bias; float* psum; int H, W, Ho, Wo, C, RB; };
template <class T, int STRIDE, bool SE>
__global__ __launch_bounds__(256) void rv_dw3_kernel(const RvDwParams p) { f16_sat_mode<T>();
    constexpr int VEC = Store<T>::VEC;
    __shared__ float sh[SE ? 256 * VEC : 1];
    const int b = blockIdx.y, band = blockIdx.x;
    const int CG = p.C / VEC, NX = 256 / CG;                 // columns walked at a time; threads beyond NX * CG idle
    const int cg = int(threadIdx.x) % CG, xs = int(threadIdx.x) / CG, c0 = cg * VEC;
    const bool live = xs < NX;
    const int y0 = band * p.RB, y1 = y0 + p.RB < p.Ho ? y0 + p.RB : p.Ho;
    const T* X = static_cast<const T*>(p.X) + long(b) * p.H * p.W * p.ldx;
    T* Y = static_cast<T*>(p.Y) + long(b) * p.Ho * p.Wo * p.ldy;
    float w[9][VEC], bias[VEC], csum[VEC];
    ACH_UNROLL
    for (int i = 0; i < VEC; ++i) { bias[i] = 0.f; csum[i] = 0.f; }
    if (live) {
        ACH_UNROLL
        for (int t = 0; t < 9; ++t)
            ACH_UNROLL
            for (int i = 0; i < VEC; ++i) w[t][i] = p.w[t * p.C + c0 + i];
        ACH_UNROLL
        for (int i = 0; i < VEC; ++i) bias[i] = p.bias[c0 + i];
    }
    // the three weighted column taps of input row r at input column ix (centre), into acc: acc += sum_kx w[ky][kx] * x[r][ix + kx - 1]
    auto row_taps = [&](int r, int ix, int ky, float* acc) {
        const T* xr = X + (long(r) * p.W + ix) * p.ldx + c0;
        const bool hl = ix > 0, hr = ix + 1 < p.W;
        const uint4 fc = *reinterpret_cast<const uint4*>(xr);
        uint4 fl = make_uint4(0u, 0u, 0u, 0u), fr = make_uint4(0u, 0u, 0u, 0u);
        if (hl) fl = *reinterpret_cast<const uint4*>(xr - p.ldx);
        if (hr) fr = *reinterpret_cast<const uint4*>(xr + p.ldx);
        float l[8], c[8], rr[8];
        frag_unpack<T>(fl, l); frag_unpack<T>(fc, c); frag_unpack<T>(fr, rr);
        ACH_UNROLL
        for (int i = 0; i < VEC; ++i) acc[i] += (w[ky * 3][i] * l[i] + w[ky * 3 + 1][i] * c[i]) + w[ky * 3 + 2][i] * rr[i];
    };
    auto emit = [&](int oy, int ox, const float* acc) {
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        ACH_UNROLL
        for (int i = 0; i < VEC; ++i) o[i] = acc[i] + bias[i];
        const uint4 f = frag_pack<T>(o);
        *reinterpret_cast<uint4*>(Y + (long(oy) * p.Wo + ox) * p.ldy + c0) = f;
        if (SE) {
            frag_unpack<T>(f, o);
            ACH_UNROLL
            for (int i = 0; i < VEC; ++i) csum[i] += o[i];
        }
    };
    if (live)
    for (int ox = xs; ox < p.Wo; ox += NX) {
        if (STRIDE == 1) {
            float up[VEC], cur[VEC], dn[VEC];                // running sums of output rows r - 1, r, r + 1 while input row r is added
            ACH_UNROLL
            for (int i = 0; i < VEC; ++i) { up[i] = 0.f; cur[i] = 0.f; dn[i] = 0.f; }
            for (int r = y0 - 1; r <= y1; ++r) {
                if (r >= 0 && r < p.H) {
                    if (r - 1 >= y0) row_taps(r, ox, 2, up);
                    if (r >= y0 && r < y1) row_taps(r, ox, 1, cur);
                    if (r + 1 < y1) row_taps(r, ox, 0, dn);
                }
                if (r - 1 >= y0) emit(r - 1, ox, up);
                ACH_UNROLL
                for (int i = 0; i < VEC; ++i) { up[i] = cur[i]; cur[i] = dn[i]; dn[i] = 0.f; }
            }
        } else {
            for (int oy = y0; oy < y1; ++oy) {
                float acc[VEC];
                ACH_UNROLL
                for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
                ACH_UNROLL
                for (int ky = 0; ky < 3; ++ky) {
                    const int r = 2 * oy - 1 + ky;
                    if (r >= 0 && r < p.H) row_taps(r, 2 * ox, ky, acc);
                }
                emit(oy, ox, acc);
            }
        }
    }
    if (SE) {
        // threads t = x * CG + cg hold the sums of channel piece cg: thread c adds the NX of its piece in thread order
        ACH_UNROLL
        for (int i = 0; i < VEC; ++i) sh[int(threadIdx.x) * VEC + i] = csum[i];
        __syncthreads();
        for (int c = threadIdx.x; c < p.C; c += 256) {
            float s = 0.f;
            for (int k = 0; k < NX; ++k) s += sh[(k * CG + c / VEC) * VEC + c % VEC];
            p.psum[(long(b) * gridDim.x + band) * p.C + c] = s;
        }
    }
}
template <class T>
inline void launch_rv_dw3(const RvDwParams& p, int stride, bool se, int B, hipStream_t s) {
    const dim3 grid(unsigned((p.Ho + p.RB - 1) / p.RB), unsigned(B)), block(256);
    if (stride == 2) ACH_LAUNCH((rv_dw3_kernel<T, 2, false>), grid, block, s, p);
    else if (se) ACH_LAUNCH((rv_dw3_kernel<T, 1, true>), grid, block, s, p);
    else ACH_LAUNCH((rv_dw3_kernel<T, 1, false>), grid, block, s, p);
}

// ------------------------------------------------------------------------------------------ SE gate
// gate[b][c] = sigmoid(fc2(relu(fc1(mean_b)))) in fp32.  One workgroup per sample; everything is summed in a fixed order that depends on (P, C, RD) alone:
//   mean : a thread per channel adds the sample's P band sums in band order (neighbouring threads read neighbouring addresses);
//   fc1  : RD outputs x S slices of the C inputs (S = 8 / 4 / 2 for RD <= 32 / 64 / 96: all 256 threads busy, C / S terms each), slice sums added in slice order;
//   fc2  : a thread per channel over the RD hidden units.
// Weights transposed on the host (w1t [C][RD], w2t [RD][C]) so that neighbouring threads read neighbouring addresses.  grid (B)
// (First form: a wave per channel with a 64-lane butterfly over the partials, one thread per fc1 output — a chain of dependent steps, 18 us per launch on the
//  20 x 20 maps where this form takes 12)
constexpr int RV_SE_CMAX = 288, RV_SE_RMAX = 96;
struct RvGateParams { const float* psum; int P; float inv_hw; const float* w1t; const float* b1; const float* w2t; const float* b2; float* gate; int C, RD; };
template <class T>      // (T only names the engine: one symbol per code object)
__global__ __launch_bounds__(256) void rv_gate_kernel(const RvGateParams p) {
    __shared__ float mean[RV_SE_CMAX], hid[RV_SE_RMAX], ps[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* part = p.psum + long(b) * p.P * p.C;
    for (int c = tid; c < p.C; c += 256) {
        float v = 0.f;
        for (int i = 0; i < p.P; ++i) v += part[long(i) * p.C + c];
        mean[c] = v * p.inv_hw;
    }
    __syncthreads();
    const int S = p.RD <= 32 ? 8 : (p.RD <= 64 ? 4 : 2);
    if (tid < p.RD * S) {
        const int r = tid % p.RD, sl = tid / p.RD;
        float a = 0.f;
        for (int k = sl; k < p.C; k += S) a += p.w1t[k * p.RD + r] * mean[k];
        ps[sl * p.RD + r] = a;
    }
    __syncthreads();
    if (tid < p.RD) {
        float a = p.b1[tid];
        for (int sl = 0; sl < S; ++sl) a += ps[sl * p.RD + tid];
        hid[tid] = a > 0.f ? a : 0.f;
    }
    __syncthreads();
    for (int c = tid; c < p.C; c += 256) {
        float a = p.b2[c];
        for (int r = 0; r < p.RD; ++r) a += p.w2t[r * p.C + c] * hid[r];
        p.gate[long(b) * p.C + c] = apply_act(a, ACT_SIGMOID);
    }
}

// ------------------------------------------------------------------------------------------ MLP
// y = g.d + W2' GELU( W1' (g.d) + b1' ) + b2': mlp_kernel's fragment chain (k_mlp.h: the lane's accumulators of a pair of hidden tiles ARE the B fragment of the
// second GEMM), same packed weights (Engine::chain_weights), hidden 2C, no norm prologue.  The per-sample, per-channel gate is applied as the row is loaded
// (gate = null: g = 1) and the residual is the GATED row.  Tiles are cut per SAMPLE — grid (.., B), row = tile * 16 + px inside the sample — so a tile has one
// gate vector.  SPLIT = false: four tiles per workgroup, one per wave (grid.x = cdiv(tiles, 4)).  SPLIT = true (small maps): the four waves share one tile,
// each takes every fourth hidden chunk, partial outputs summed through LDS in wave order (grid.x = tiles).  16-bit k-chunks are two 16x16x16 instructions
// (mfma16_pair).
// The chunk loop and the SPLIT reduction below are the same text as pf_mlp_kernel's (k_poolformer.h) and, for the reduction, mlp_kernel's: a fix to one belongs in
// all three.  Stated once as force-inlined helpers they compiled to other register allocations in this kernel, so each kernel keeps its own; the
// width dispatch (mlp_for_dt) and the weight packing are shared.
struct RvMlpParams { MlpParams m; const float* gate; int HW; };
template <class T, int DT, bool SPLIT>
__global__ __launch_bounds__(256, (MlpOcc<DT, SPLIT, Store<T>::VEC>::blocks)) void rv_mlp_kernel(const RvMlpParams q) { f16_sat_mode<T>();
    constexpr int VEC = Store<T>::VEC;
    constexpr int KC = 4 * VEC;
    constexpr int K1MAX = (16 * DT + KC - 1) / KC;
    constexpr int HSTEP = 8 / VEC;
    constexpr int RT = DT < MLP_RED_TILES ? DT : MLP_RED_TILES;
    __shared__ float red[SPLIT ? 4 * RT * 4 * 64 : 1];
    const MlpParams& p = q.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const T* X = static_cast<const T*>(p.X);
    const float* gate = q.gate ? q.gate + long(b) * p.C : nullptr;
    const uint4* W1f = static_cast<const uint4*>(p.W1) + lane;
    const uint4* W2f = static_cast<const uint4*>(p.W2) + lane;
    const int tile = SPLIT ? int(blockIdx.x) : int(blockIdx.x) * 4 + wave;
    const int rraw = tile * 16 + px;
    const bool valid = rraw < q.HW;
    const long m = long(b) * q.HW + (valid ? rraw : 0);
    // ---- 1. input fragments, gated
    uint4 xf[K1MAX];
    ACH_UNROLL
    for (int s = 0; s < K1MAX; ++s) {
        xf[s] = make_uint4(0u, 0u, 0u, 0u);
        const int k0 = s * KC + g * VEC;
        if (s < p.k1 && valid && k0 < p.C) {
            xf[s] = *reinterpret_cast<const uint4*>(X + m * p.ldx + k0);
            if (gate) {
                float v[8];
                frag_unpack<T>(xf[s], v);
                ACH_UNROLL
                for (int i = 0; i < VEC; ++i) v[i] *= gate[k0 + i];
                xf[s] = frag_pack<T>(v);
            }
        }
    }
    // ---- 2. hidden chunks of 32 channels: GEMM1 (2 tiles) -> bias, GELU -> GEMM2 accumulation
    f32x4 acc2[DT];
    ACH_UNROLL
    for (int t = 0; t < DT; ++t) { acc2[t][0] = 0.f; acc2[t][1] = 0.f; acc2[t][2] = 0.f; acc2[t][3] = 0.f; }
    constexpr int JS = SPLIT ? 4 : 1;
    for (int j = SPLIT ? wave : 0; j < p.J; j += JS) {
        f32x4 a0, a1;
        a0[0] = a0[1] = a0[2] = a0[3] = 0.f;
        a1[0] = a1[1] = a1[2] = a1[3] = 0.f;
        const f32x4 bA = *reinterpret_cast<const f32x4*>(p.b1 + j * 32 + g * 8), bB = *reinterpret_cast<const f32x4*>(p.b1 + j * 32 + g * 8 + 4);
        const uint4* w1 = W1f + long(j) * p.k1 * 2 * 64;
        // (k-steps beyond k1 re-read the last fragment against a zero input: branch-free, all of the chunk's loads can be in flight at once)
        uint4 wa[K1MAX], wb[K1MAX];
        ACH_UNROLL
        for (int s = 0; s < K1MAX; ++s) { const int sc = s < p.k1 ? s : p.k1 - 1; wa[s] = w1[(sc * 2) * 64]; wb[s] = w1[(sc * 2 + 1) * 64]; }
        ACH_UNROLL
        for (int s = 0; s < K1MAX; ++s) { mfma16_pair<T>(wa[s], xf[s], a0); mfma16_pair<T>(wb[s], xf[s], a1); }
        float h[8];
        ACH_UNROLL
        for (int r = 0; r < 4; ++r) { h[r] = a0[r] + bA[r]; h[4 + r] = a1[r] + bB[r]; }
        apply_act_n<T, 8, ACT_GELU>(h, ACT_GELU);
        ACH_UNROLL
        for (int hh = 0; hh < HSTEP; ++hh) {
            const uint4 hf = frag_pack<T>(h + hh * VEC);
            const uint4* w2 = W2f + long(j * HSTEP + hh) * DT * 64;
            ACH_UNROLL
            for (int t = 0; t < DT; ++t) mfma16_pair<T>(w2[t * 64], hf, acc2[t]);
        }
    }
    // ---- 3. + bias + residual (the gated input row), 8 consecutive channels per lane per tile pair
    auto finish = [&](int pair, const float* v8) {
        const int nb = pair * 32 + g * 8;
        if (!valid || nb >= p.Cout) return;
        float o[8], r8[8];
        Store<T>::ld8(X + m * p.ldx + nb, r8);
        if (gate) {
            ACH_UNROLL
            for (int i = 0; i < 8; ++i) r8[i] *= gate[nb + i];
        }
        ACH_UNROLL
        for (int i = 0; i < 8; ++i) o[i] = v8[i] + p.b2[nb + i] + r8[i];
        Store<T>::st8(static_cast<T*>(p.Y) + m * p.ldy + nb, o);
    };
    if (!SPLIT) {
        ACH_UNROLL
        for (int pair = 0; pair < DT / 2; ++pair) {
            float v8[8];
            ACH_UNROLL
            for (int r = 0; r < 4; ++r) { v8[r] = acc2[2 * pair][r]; v8[4 + r] = acc2[2 * pair + 1][r]; }
            finish(pair, v8);
        }
    } else {
        ACH_UNROLL
        for (int t0 = 0; t0 < DT; t0 += RT) {
            if (t0 > 0) __syncthreads();
            ACH_UNROLL
            for (int t = 0; t < RT; ++t) {
                if (t0 + t >= DT) continue;
                ACH_UNROLL
                for (int r = 0; r < 4; ++r) red[((wave * RT + t) * 4 + r) * 64 + lane] = acc2[t0 + t][r];
            }
            __syncthreads();
            ACH_UNROLL
            for (int qd = 0; qd < RT / 2; ++qd) {                     // pair qd of this round belongs to wave qd % 4
                if ((qd & 3) != wave || t0 + 2 * qd >= DT) continue;
                float v8[8];
                ACH_UNROLL
                for (int i = 0; i < 8; ++i) {
                    const int t = 2 * qd + (i >> 2), r = i & 3;
                    float a = 0.f;
                    ACH_UNROLL
                    for (int w = 0; w < 4; ++w) a += red[((w * RT + t) * 4 + r) * 64 + lane];
                    v8[i] = a;
                }
                finish((t0 >> 1) + qd, v8);
            }
        }
    }
}
inline int rv_mlp_blocks(int HW, bool split) { const int tiles = (HW + 15) / 16; return split ? tiles : (tiles + 3) / 4; }
template <class T>
inline bool launch_rv_mlp(const RvMlpParams& q, int DT, bool split, int B, hipStream_t stream) {
    const dim3 grid(unsigned(rv_mlp_blocks(q.HW, split)), unsigned(B)), block(256);
    return mlp_for_dt<2, 4, 6, 8, 10, 12, 18>(DT, [&](auto dt) {
        constexpr int D = decltype(dt)::value;
        if (split) ACH_LAUNCH((rv_mlp_kernel<T, D, true>), grid, block, stream, q); else ACH_LAUNCH((rv_mlp_kernel<T, D, false>), grid, block, stream, q);
    });
}

}  // namespace ach
