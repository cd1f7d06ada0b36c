// k_poolformer.h — the PoolFormer backbone (backbone/vision/poolformer_modules/poolformer.py, poolformer_S0/S1/S2):
//
//     x0 = conv7x7 s4 p2 (3 -> C0, bias)
//     block:  y = x + ls1 * ( avgpool3x3(GN1(x)) - GN1(x) )          (stride 1, pad 1, count_include_pad = False)
//             z = y + ls2 * fc2( GELU( fc1( GN2(y) ) ) )              (1x1 convs, hidden 4C)
//     out_i = GN_fork_i(stage output);  between stages conv3x3 s2 p1 on the un-normalised stage output
//
// GN = GroupNorm(1, C): mean / biased variance per SAMPLE over the whole C x H x W map — the one normalisation of this library whose
// statistics cross workgroups.  Scheme (no atomics, deterministic, batch-invariant):
//   * every kernel that writes a tensor a GroupNorm will read also writes, per workgroup, the (count, mean, M2) triple of the values it
//     stored — taken from the values AS STORED in T — into a small fp32 table [sample][partial][4];
//   * every consumer merges the partials of its sample in a fixed order (lane-strided, then a butterfly in which the lower lane is
//     always the left operand), in fp32.  The decomposition into partials depends on (H, W, C) only and grids are (partials, sample),
//     so a frame's statistics — and its result — are bit-identical whatever batch it sits in, and no 16-pixel MFMA tile holds pixels
//     of two samples.
// Two folds make the block two launches:
//   * the pool averages over valid cells only, so a per-channel constant passes through it: pool(GN1 x) - GN1 x = g1_c rstd_b (pool x - x);
//     mean and beta cancel, and a_c = ls1_c g1_c is folded on the host: y = x + a_c rstd_b (pool(x) - x)        (pf_mixer_kernel)
//   * the MLP is mlp_kernel's register chain (k_mlp.h) with (mu, rstd) per sample instead of per pixel; g2 -> W1, W1 b2 -> b1,
//     ls2 -> W2 / b2 on the host                                                                                   (pf_mlp_kernel)
#pragma once
#include "ach_platform.h"
#include "k_gemm.h"
#include "k_mlp.h"

namespace ach {

// ------------------------------------------------------------------------------------------ moments
struct PfMom { float n, mean, m2; };
// Chan's merge; `a` is the left operand (the order is part of the result).  An empty side (n = 0, mean = 0, m2 = 0) leaves the other unchanged.
__device__ __forceinline__ PfMom pf_merge(const PfMom& a, const PfMom& b) {
    PfMom r;
    r.n = a.n + b.n;
    const float f = r.n > 0.f ? b.n / r.n : 0.f, d = b.mean - a.mean;
    r.mean = a.mean + d * f;
    r.m2 = a.m2 + b.m2 + d * d * a.n * f;
    return r;
}
// all 64 lanes receive the merge of the wave's triples in lane order
__device__ __forceinline__ PfMom pf_wave_merge(PfMom v, int lane) {
    ACH_UNROLL
    for (int k = 1; k < 64; k <<= 1) {
        PfMom o;
        o.n = __shfl_xor(v.n, k); o.mean = __shfl_xor(v.mean, k); o.m2 = __shfl_xor(v.m2, k);
        v = (lane & k) ? pf_merge(o, v) : pf_merge(v, o);
    }
    return v;
}
// N values (two passes over registers) merged into a lane's running triple
template <int N> __device__ __forceinline__ void pf_mom_add(PfMom& acc, const float* v) {
    float s = 0.f;
    ACH_UNROLL
    for (int i = 0; i < N; ++i) s += v[i];
    PfMom g;
    g.n = float(N); g.mean = s * (1.0f / float(N)); g.m2 = 0.f;
    ACH_UNROLL
    for (int i = 0; i < N; ++i) { const float d = v[i] - g.mean; g.m2 += d * d; }
    acc = pf_merge(acc, g);
}
// store 8 consecutive elements and replace `o` by the values as stored (the clamping Store<T> path: fp16 saturation is counted on them)
template <class T> __device__ __forceinline__ void pf_store8(T* dst, float (&o)[8]) {
    Store<T>::st8(dst, o);
    if constexpr (sizeof(T) == 2) {
        const uint4 f = frag_pack<T>(o);
        frag_unpack<T>(f, o);
    }
}
// the workgroup's triple -> dst[0..3]; `sh` holds 3 floats per wave.  Every thread of the workgroup calls this.
__device__ __forceinline__ void pf_block_moments(PfMom v, float* dst, float* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = int(blockDim.x) >> 6;
    v = pf_wave_merge(v, lane);
    if (lane == 0) { sh[wave * 3] = v.n; sh[wave * 3 + 1] = v.mean; sh[wave * 3 + 2] = v.m2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        PfMom t{sh[0], sh[1], sh[2]};
        for (int w = 1; w < nw; ++w) t = pf_merge(t, PfMom{sh[w * 3], sh[w * 3 + 1], sh[w * 3 + 2]});
        *reinterpret_cast<float4*>(dst) = make_float4(t.n, t.mean, t.m2, 0.f);
    }
}
// a sample's (mu, rstd) from its P partials; every lane of the wave calls this and receives the same pair
__device__ __forceinline__ void pf_sample_stats(const float* part, int P, float eps, float& mu, float& rstd) {
    const int lane = threadIdx.x & 63;
    PfMom v{0.f, 0.f, 0.f};
    for (int i = lane; i < P; i += 64) {
        const float4 q = *reinterpret_cast<const float4*>(part + long(i) * 4);
        v = pf_merge(v, PfMom{q.x, q.y, q.z});
    }
    v = pf_wave_merge(v, lane);
    mu = v.mean;
    rstd = ln_rstd(v.m2 / v.n + eps);
}

// ------------------------------------------------------------------------------------------ moments of an existing tensor
// (behind the implicit-GEMM down-sampling convs, whose epilogue stays as it is)  grid (cdiv(HW, 256), B)
struct PfMomParams { const void* X; long ldx; float* mout; int HW, C; };
constexpr int PF_MOM_PIX = 256;
template <class T>
__global__ __launch_bounds__(256) void pf_moments_kernel(const PfMomParams p) { f16_sat_mode<T>();
    constexpr int VEC = Store<T>::VEC;
    __shared__ float sh[12];
    const int b = blockIdx.y, CG = p.C / VEC;
    const int px0 = int(blockIdx.x) * PF_MOM_PIX, npx = p.HW - px0 < PF_MOM_PIX ? p.HW - px0 : PF_MOM_PIX;
    const T* X = static_cast<const T*>(p.X) + (long(b) * p.HW + px0) * p.ldx;
    PfMom acc{0.f, 0.f, 0.f};
    for (int it = threadIdx.x; it < npx * CG; it += 256) {
        const int px = it / CG, c0 = (it - px * CG) * VEC;
        float v[8];
        frag_unpack<T>(*reinterpret_cast<const uint4*>(X + long(px) * p.ldx + c0), v);
        pf_mom_add<VEC>(acc, v);
    }
    pf_block_moments(acc, p.mout + (long(b) * gridDim.x + blockIdx.x) * 4, sh);
}

// ------------------------------------------------------------------------------------------ fork norms
// Y = (X - mu_b) rstd_b g_c + beta_c, into the neck's concat-buffer slice or a map of its own.  grid (cdiv(HW * C / VEC, 256), B)
struct PfNormParams { const void* X; long ldx; void* Y; long ldy; const float* g; const float* beta; const float* min; int Pin, HW, C; float eps; };
template <class T>
__global__ __launch_bounds__(256) void pf_norm_apply_kernel(const PfNormParams p) { f16_sat_mode<T>();
    constexpr int VEC = Store<T>::VEC;
    const int b = blockIdx.y, CG = p.C / VEC;
    float mu, rstd;
    pf_sample_stats(p.min + long(b) * p.Pin * 4, p.Pin, p.eps, mu, rstd);
    const int it = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (it >= p.HW * CG) return;
    const int px = it / CG, c0 = (it - px * CG) * VEC;
    const long row = long(b) * p.HW + px;
    float v[8], o[8];
    frag_unpack<T>(*reinterpret_cast<const uint4*>(static_cast<const T*>(p.X) + row * p.ldx + c0), v);
    ACH_UNROLL
    for (int i = 0; i < VEC; ++i) o[i] = (v[i] - mu) * rstd * p.g[c0 + i] + p.beta[c0 + i];
    *reinterpret_cast<uint4*>(static_cast<T*>(p.Y) + row * p.ldy + c0) = frag_pack<T>(o);
}

// ------------------------------------------------------------------------------------------ token mixer
// y = x + a_c rstd_b (pool3x3(x) - x).  A workgroup owns a band of RB rows of one sample; a thread owns one (column, 16-byte channel piece)
// and walks down the band with the three-column sums of the previous / current / next row in registers: per output it fetches one row of
// three neighbours (its own column and the two beside it, which the threads next to it fetch too: those come from L1), so a row of the
// band is read from memory once; the two halo rows of a band are the only re-reads.  grid (cdiv(H, RB), B)
struct PfMixParams { const void* X; long ldx; void* Y; long ldy; const float* a; const float* min; int Pin; float* mout; int H, W, C, RB; float eps; };
template <class T>
__global__ __launch_bounds__(256) void pf_mixer_kernel(const PfMixParams p) { f16_sat_mode<T>();
    constexpr int VEC = Store<T>::VEC;
    __shared__ float sh[12];
    const int b = blockIdx.y, band = blockIdx.x;
    float mu, rstd;
    pf_sample_stats(p.min + long(b) * p.Pin * 4, p.Pin, p.eps, mu, rstd);
    const int CG = p.C / VEC, items = p.W * CG;
    const int y0 = band * p.RB, y1 = y0 + p.RB < p.H ? y0 + p.RB : p.H;
    const T* X = static_cast<const T*>(p.X) + long(b) * p.H * p.W * p.ldx;
    T* Y = static_cast<T*>(p.Y) + long(b) * p.H * p.W * p.ldy;
    PfMom acc{0.f, 0.f, 0.f};
    for (int it = threadIdx.x; it < items; it += 256) {
        const int x = it / CG, c0 = (it - x * CG) * VEC;
        const bool hl = x > 0, hr = x + 1 < p.W;
        const int nx = 1 + (hl ? 1 : 0) + (hr ? 1 : 0);
        float av[VEC];
        ACH_UNROLL
        for (int i = 0; i < VEC; ++i) av[i] = p.a[c0 + i] * rstd;
        // three-column sum of row r (cs) and its centre value (ct)
        auto row3 = [&](int r, float* cs, float* ct) {
            const T* xr = X + (long(r) * p.W + x) * p.ldx + c0;
            const uint4 fc = *reinterpret_cast<const uint4*>(xr);
            uint4 fl = make_uint4(0u, 0u, 0u, 0u), fr = make_uint4(0u, 0u, 0u, 0u);
            if (hl) fl = *reinterpret_cast<const uint4*>(xr - p.ldx);
            if (hr) fr = *reinterpret_cast<const uint4*>(xr + p.ldx);
            float l[8], rr[8];
            frag_unpack<T>(fc, ct); frag_unpack<T>(fl, l); frag_unpack<T>(fr, rr);
            ACH_UNROLL
            for (int i = 0; i < VEC; ++i) cs[i] = (l[i] + ct[i]) + rr[i];
        };
        float prev[8], cur[8], nxt[8], ctc[8], ctn[8];
        ACH_UNROLL
        for (int i = 0; i < 8; ++i) { prev[i] = 0.f; nxt[i] = 0.f; ctn[i] = 0.f; }
        if (y0 > 0) { float dump[8]; row3(y0 - 1, prev, dump); }
        row3(y0, cur, ctc);
        for (int r = y0; r < y1; ++r) {
            const bool hd = r + 1 < p.H;
            if (hd) row3(r + 1, nxt, ctn);
            const int ny = 1 + (r > 0 ? 1 : 0) + (hd ? 1 : 0);
            const float inv = 1.0f / float(nx * ny);
            float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            ACH_UNROLL
            for (int i = 0; i < VEC; ++i) {
                const float sum = (prev[i] + cur[i]) + (hd ? nxt[i] : 0.f);
                o[i] = ctc[i] + av[i] * (sum * inv - ctc[i]);
            }
            const uint4 f = frag_pack<T>(o);
            *reinterpret_cast<uint4*>(Y + (long(r) * p.W + x) * p.ldy + c0) = f;
            frag_unpack<T>(f, o);
            pf_mom_add<VEC>(acc, o);
            ACH_UNROLL
            for (int i = 0; i < VEC; ++i) { prev[i] = cur[i]; cur[i] = nxt[i]; ctc[i] = ctn[i]; }
        }
    }
    pf_block_moments(acc, p.mout + (long(b) * gridDim.x + band) * 4, sh);
}

// ------------------------------------------------------------------------------------------ MLP
// z = y + W2' GELU( W1' ((y - mu_b) rstd_b) + b1' ) + b2': mlp_kernel's fragment chain (k_mlp.h: the lane's accumulators of a pair of hidden tiles ARE the
// B fragment of the second GEMM), same packed weights (Engine::chain_weights).  Tiles are cut per SAMPLE — grid (.., B), row = tile * 16 + px inside the
// sample — so a tile's (mu, rstd) is one pair.  SPLIT = false: four tiles per workgroup, one per wave (grid.x = cdiv(tiles, 4)).  SPLIT = true (small
// maps): the four waves share one tile, each takes every fourth hidden chunk, partial outputs summed through LDS in wave order (grid.x = tiles).
// 16-bit k-chunks are two 16x16x16 instructions (mfma16_pair).
// The chunk loop and the SPLIT reduction below are the same text as rv_mlp_kernel's (k_repvit.h) and, for the reduction, mlp_kernel's: a fix to one belongs in all
// three.  Stated once as force-inlined helpers they compiled to other register allocations and more scratch in this kernel, so each kernel keeps its
// own; the width dispatch (mlp_for_dt) and the weight packing are shared.
struct PfMlpParams { MlpParams m; const float* min; int Pin; float* mout; int HW; float eps; int tpw; };
// mlp_kernel's register budgets, except that the one-tile-per-wave kernels stop at five workgroups per CU: with the running moments next to the accumulators the
// narrow widths spilled 12 / 20 bytes at six
template <int DT, bool SPLIT, int VEC> struct PfMlpOcc {
    static constexpr int base = MlpOcc<DT, SPLIT, VEC>::blocks;
    static constexpr int blocks = (!SPLIT && base > 5) ? 5 : base;
};
template <class T, int DT, bool SPLIT>
__global__ __launch_bounds__(256, (PfMlpOcc<DT, SPLIT, Store<T>::VEC>::blocks)) void pf_mlp_kernel(const PfMlpParams q) { f16_sat_mode<T>();
    constexpr int VEC = Store<T>::VEC;
    constexpr int KC = 4 * VEC;
    constexpr int K1MAX = (16 * DT + KC - 1) / KC;
    constexpr int HSTEP = 8 / VEC;
    constexpr int RT = DT < MLP_RED_TILES ? DT : MLP_RED_TILES;
    __shared__ float red[SPLIT ? 4 * RT * 4 * 64 : 1];
    __shared__ float sh[12];
    const MlpParams& p = q.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    float mu, rstd;
    pf_sample_stats(q.min + long(b) * q.Pin * 4, q.Pin, q.eps, mu, rstd);
    PfMom acc{0.f, 0.f, 0.f};
    const T* X = static_cast<const T*>(p.X);
    const uint4* W1f = static_cast<const uint4*>(p.W1) + lane;
    const uint4* W2f = static_cast<const uint4*>(p.W2) + lane;
    // one-tile-per-wave form on the large maps: a wave walks q.tpw consecutive tiles, so the statistics merge in front and the moments reduction behind are paid once
    ACH_NO_UNROLL
    for (int tt = 0; tt < (SPLIT ? 1 : q.tpw); ++tt) {
    const int tile = SPLIT ? int(blockIdx.x) : (int(blockIdx.x) * 4 + wave) * q.tpw + tt;
    const int rraw = tile * 16 + px;
    const bool valid = rraw < q.HW;
    const long m = long(b) * q.HW + (valid ? rraw : 0);
    // ---- 1. input fragments, normalised with the sample's statistics (affine folded into W1 / b1)
    uint4 xf[K1MAX];
    ACH_UNROLL
    for (int s = 0; s < K1MAX; ++s) {
        xf[s] = make_uint4(0u, 0u, 0u, 0u);
        const int k0 = s * KC + g * VEC;
        if (s < p.k1 && valid && k0 < p.C) {
            float v[8];
            frag_unpack<T>(*reinterpret_cast<const uint4*>(X + m * p.ldx + k0), v);
            ACH_UNROLL
            for (int i = 0; i < VEC; ++i) v[i] = (v[i] - mu) * rstd;
            xf[s] = frag_pack<T>(v);
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
    // ---- 3. + bias + residual (the un-normalised input row), 8 consecutive channels per lane per tile pair; moments of what is stored
    auto finish = [&](int pair, const float* v8) {
        const int nb = pair * 32 + g * 8;
        if (!valid || nb >= p.Cout) return;
        float o[8], r8[8];
        Store<T>::ld8(X + m * p.ldx + nb, r8);
        ACH_UNROLL
        for (int i = 0; i < 8; ++i) o[i] = v8[i] + p.b2[nb + i] + r8[i];
        pf_store8<T>(static_cast<T*>(p.Y) + m * p.ldy + nb, o);
        pf_mom_add<8>(acc, o);
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
    pf_block_moments(acc, q.mout + (long(b) * gridDim.x + blockIdx.x) * 4, sh);
}
// workgroups per sample = partials per sample of the output
inline int pf_mlp_tpw(int HW, bool split) { return (!split && HW >= 4096) ? 4 : 1; }           // tiles per wave: by the map alone (the partials must not depend on the batch)
inline int pf_mlp_blocks(int HW, bool split) { const int tiles = (HW + 15) / 16; return split ? tiles : (tiles + 4 * pf_mlp_tpw(HW, split) - 1) / (4 * pf_mlp_tpw(HW, split)); }
template <class T>
inline bool launch_pf_mlp(const PfMlpParams& q, int DT, bool split, int B, hipStream_t stream) {
    const dim3 grid(unsigned(pf_mlp_blocks(q.HW, split)), unsigned(B)), block(256);
    return mlp_for_dt<2, 4, 6, 8, 10, 12, 18>(DT, [&](auto dt) {
        constexpr int D = decltype(dt)::value;
        if (split) ACH_LAUNCH((pf_mlp_kernel<T, D, true>), grid, block, stream, q); else ACH_LAUNCH((pf_mlp_kernel<T, D, false>), grid, block, stream, q);
    });
}

// ------------------------------------------------------------------------------------------ stem
// conv 7x7 / stride 4 / pad 2, 3 -> 32 channels + bias, gathered from the caller's NCHW image, NHWC out, as an MFMA GEMM with K = (dy, c, dx) and dx
// padded from 7 to 8: a lane's 16-byte B fragment is then 8 (fp32: 4) CONSECUTIVE input pixels of one row of one channel.  Windows overlap (7 wide,
// stride 4), so a workgroup — one output row, PF_STEM_SEG output pixels, a 16-pixel tile per wave — stages its 3 x 7 input rows in LDS as fp32, with the
// zero padding written in, and the fragments are aligned 16-byte LDS reads.  K = 7 * 3 * 8 = 168, zero-padded to the k-step (192 / 176).
// grid (Ho * cdiv(Wo, PF_STEM_SEG), B)
constexpr int PF_STEM_SEG = 64, PF_STEM_PITCH = 4 * PF_STEM_SEG + 4, PF_STEM_K = 168;
struct PfStemParams { const void* X; void* Y; long ldy; const void* Wp; const float* bias; float* mout; int H, W, Ho, Wo, segs; };
__host__ __device__ __forceinline__ int pf_stem_k(int c, int dy, int dx) { return (dy * 3 + c) * 8 + dx; }
template <class T, class IO>
__global__ __launch_bounds__(256) void pf_stem_kernel(const PfStemParams p) { f16_sat_mode<T>();
    constexpr int VEC = Store<T>::VEC;
    constexpr int KS = (PF_STEM_K + 4 * VEC - 1) / (4 * VEC);
    __shared__ __attribute__((aligned(16))) float bandl[21 * PF_STEM_PITCH];
    __shared__ float sh[12];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, seg = int(blockIdx.x) % p.segs, oy = int(blockIdx.x) / p.segs;
    const int ox0 = seg * PF_STEM_SEG, ix0 = 4 * ox0 - 2, iy0 = 4 * oy - 2;
    const IO* X = static_cast<const IO*>(p.X) + long(b) * 3 * p.H * p.W;
    // the band, in aligned pieces of 8 input pixels (W is a multiple of 8: a piece is inside the row or outside it), only as wide as this segment's tiles:
    // LDS column j is input column ix0 + j; ix0 is even, so an even pair of a piece lands on an 8-byte LDS address or outside the band
    const int tiles = (p.Wo - ox0 + 15) / 16 < PF_STEM_SEG / 16 ? (p.Wo - ox0 + 15) / 16 : PF_STEM_SEG / 16;
    const int q0 = (ix0 - 6) / 8, nq = (64 * tiles + 4 + 6 + 7) / 8;                 // ix0 - 6 = 4 ox0 - 8: a multiple of 8
    for (int it = threadIdx.x; it < 21 * nq; it += 256) {
        const int row = it / nq, q = q0 + (it - row * nq);
        const int c = row / 7, dy = row - c * 7, iy = iy0 + dy;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (iy >= 0 && iy < p.H && q >= 0 && 8 * q + 7 < p.W) {
            const IO* src = X + (long(c) * p.H + iy) * p.W + 8 * q;
            if constexpr (sizeof(IO) == 2) frag_unpack<IO>(*reinterpret_cast<const uint4*>(src), v);
            else Store<IO>::ld8(src, v);
        }
        ACH_UNROLL
        for (int e = 0; e < 8; e += 2) {
            const int j = 8 * q + e - ix0;
            if (j >= 0 && j + 1 < PF_STEM_PITCH) *reinterpret_cast<float2*>(bandl + row * PF_STEM_PITCH + j) = make_float2(v[e], v[e + 1]);
        }
    }
    __syncthreads();
    const int ox = ox0 + wave * 16 + px;
    const bool valid = ox < p.Wo;
    const int jb = valid ? (wave * 16 + px) * 4 : 0;
    const uint4* Wf = static_cast<const uint4*>(p.Wp) + lane;
    f32x4 a0, a1;
    a0[0] = a0[1] = a0[2] = a0[3] = 0.f;
    a1[0] = a1[1] = a1[2] = a1[3] = 0.f;
    ACH_UNROLL
    for (int s = 0; s < KS; ++s) {
        const int piece = s * 4 + g;                                  // 16-byte piece of K
        const int u = VEC == 8 ? piece : piece >> 1, half = VEC == 8 ? 0 : (piece & 1);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (u < 21) {
            const int dy = u / 3, c = u - dy * 3;
            const float* src = bandl + (c * 7 + dy) * PF_STEM_PITCH + jb + half * 4;
            ACH_UNROLL
            for (int qv = 0; qv < VEC / 4; ++qv) {
                const f32x4 t4 = *reinterpret_cast<const f32x4*>(src + 4 * qv);
                v[4 * qv] = t4[0]; v[4 * qv + 1] = t4[1]; v[4 * qv + 2] = t4[2]; v[4 * qv + 3] = t4[3];
            }
        }
        const uint4 xfrag = frag_pack<T>(v);
        mfma16_pair<T>(Wf[(s * 2) * 64], xfrag, a0);
        mfma16_pair<T>(Wf[(s * 2 + 1) * 64], xfrag, a1);
    }
    PfMom acc{0.f, 0.f, 0.f};
    if (valid) {
        float o[8];
        ACH_UNROLL
        for (int r = 0; r < 4; ++r) { o[r] = a0[r] + p.bias[g * 8 + r]; o[4 + r] = a1[r] + p.bias[g * 8 + 4 + r]; }
        pf_store8<T>(static_cast<T*>(p.Y) + ((long(b) * p.Ho + oy) * p.Wo + ox) * p.ldy + g * 8, o);
        pf_mom_add<8>(acc, o);
    }
    pf_block_moments(acc, p.mout + (long(b) * gridDim.x + blockIdx.x) * 4, sh);
}

}  // namespace ach
