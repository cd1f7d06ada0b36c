// k_lngemm.h — the LayerNorm-prologue GEMMs of the 16-bit engines with every row tile read and normalised ONCE: EdgeNeXt's three 2x2 / stride-2 patchify convs with the
// per-tap LayerNorm of their input pixels (k_gemm.h LNTAP) and the LayerNorm + qkv projections in front of the cross-covariance attention.
//
// gemm_body (k_gemm.h) walks the k-steps of a tile twice per N-chunk — once for the statistics, a load and its use per trip of a loop whose trip count it learns at run
// time, and again inside the chunk's k-loop, where it normalises and rounds every fragment anew — and the engine deals the N-chunks of a tile to DIFFERENT workgroups when
// the rows alone do not fill the chip (zsplit, engine_impl.h gemm()): each of them fetches the same rows and repeats the statistics.  On the 20 x 20 and 10 x 10 maps these
// launches are a chain of a dozen L2 round trips per wave in front of the first matrix instruction.  Here K is a template parameter:
//   phase A  all of a tile's activation fragments are requested together (the loop unrolls: every load is in flight before the first use), the statistics come from those
//            registers — the lane's VEC elements in order, k-steps in order, then the butterflies over lanes 16 and 32: gemm_body's summation order exactly — and every
//            fragment is normalised and rounded to the storage type once;
//   phase B  per N-chunk the mfma16 sequence over k, bias, activation, residual and stores of gemm_body (ln_gemm_store_tile).  The weight fragments stream through a ring of
//            LNG_DEPTH k-steps that runs on across the wave's chunks, so the next chunk's first fragments are in flight during the epilogue.
// SHARE = false: a wave owns a 16-row tile and walks the chunk range of its blockIdx.z with the normalised fragments in registers — no LDS, no barrier (the launches whose
//                rows alone fill the chip; with one chunk this is the whole kernel).
// SHARE = true:  a WORKGROUP owns a 16-row tile.  Wave 0 runs phase A and writes the normalised B fragments to LDS in lane order (16 bytes per lane and k-step: at most
//                12 KB at K = 384); behind one barrier wave w takes the chunks w, w + NW, ... and reads its fragments back from its own lane's slots.  NW = the number of
//                blockIdx.z slices gemm() would have dealt the chunks to, so a launch has the wave count it had — the parallelism the split was made for — and a tile's rows
//                are fetched and normalised once instead of once per slice.  The other waves request their first weight fragments before they wait at the barrier.
// Same products, same sums in the same order as gemm_body: bit-identical outputs.
#pragma once
#include "k_gemm.h"

namespace ach {

// gemm_body's epilogue for one 16-row tile of one chunk (NT = 4; a copy, so that gemm_body compiles to what it was): the lane holds, for its pixel (row m), the channels
// chunk_channel(NT, t, g, r) of the chunk at cbase — bias, activation, residual, then 16-byte stores (or the NCHW scatter of a network output).
template <class T, int NT>
__device__ __forceinline__ void ln_gemm_store_tile(const GemmParams& p, const f32x4 (&acc)[NT], const float (&bv)[4 * NT], long m, int cbase, int g) {
    float o[4 * NT];
    ACH_UNROLL
    for (int t = 0; t < NT; ++t)
        ACH_UNROLL
        for (int r = 0; r < 4; ++r) o[t * 4 + r] = acc[t][r] + bv[t * 4 + r];
    apply_act_n<T, 4 * NT>(o, p.act);
    if (p.out_nchw) {
        T* Y = static_cast<T*>(p.Y);
        const long b = m / p.HW, pix = m - b * p.HW;
        ACH_UNROLL
        for (int t = 0; t < NT; ++t)
            ACH_UNROLL
            for (int r = 0; r < 4; ++r) {
                const int n = cbase + chunk_channel(NT, t, g, r);
                if (n < p.N) st_user<T>(Y, (b * p.Ctot + p.coff + n) * p.HW + pix, o[t * 4 + r], p.out_nchw == 2);
            }
        return;
    }
    T* yrow = static_cast<T*>(p.Y) + m * p.ldy;
    const T* rrow = p.R ? static_cast<const T*>(p.R) + m * p.ldr : nullptr;
    static_assert(NT >= 2, "pairs of 16-channel tiles");
    ACH_UNROLL
    for (int j = 0; j < NT / 2; ++j) {
        const int nb = cbase + j * 32 + g * 8;                  // 8 consecutive channels nb .. nb+7
        if (nb >= p.N) continue;
        float v8[8];
        ACH_UNROLL
        for (int i = 0; i < 8; ++i) v8[i] = o[j * 8 + i];       // tiles 2j (first 4) and 2j+1 (last 4)
        if (p.vec_store && nb + 8 <= p.N) {
            if (rrow) { float r8[8]; Store<T>::ld8(rrow + nb, r8); ACH_UNROLL for (int i = 0; i < 8; ++i) v8[i] += r8[i]; }
            Store<T>::st8(yrow + nb, v8);
        } else {
            for (int i = 0; i < 8; ++i)
                if (nb + i < p.N) {
                    float v = v8[i];
                    if (rrow) v += Store<T>::ld(rrow + nb + i);
                    Store<T>::st(yrow + nb + i, v);
                }
        }
    }
}

constexpr int LNG_DEPTH = 3;                    // k-steps of weight fragments in flight per wave
constexpr int LNG_MAX_WAVES = 10;               // waves of a SHARE workgroup (its launch bound)

// activation fragments of k-steps 0 .. KS-1 of this lane's row -> normalised, rounded to T, in place
template <class T, int K, bool LNTAP>
__device__ __forceinline__ void ln_rows_phase_a(const GemmParams& p, bool valid, long m, int g, uint4 (&xr)[(K + 4 * Store<T>::VEC - 1) / (4 * Store<T>::VEC)]) {
    constexpr int VEC = Store<T>::VEC, KC = 4 * VEC, KS = (K + KC - 1) / KC, CIN = K / 4;
    static_assert(!LNTAP || (K % KC == 0 && CIN % VEC == 0), "per-tap LayerNorm: whole k-steps, a lane's channels inside one tap");
    const T* X = static_cast<const T*>(p.X);
    long xbase = m * p.ldx;
    int iy0 = 0, ix0 = 0;
    if constexpr (LNTAP) {
        const long b = m / (long(p.Ho) * p.Wo);
        const int rem = int(m - b * long(p.Ho) * p.Wo);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        iy0 = oy * p.conv_s - p.conv_p;
        ix0 = ox * p.conv_s - p.conv_p;
        xbase = b * p.Hin * long(p.Win);            // pixel index of the sample's first input pixel
    }
    ACH_UNROLL
    for (int s = 0; s < KS; ++s) {
        const int k0 = s * KC + g * VEC;
        xr[s] = make_uint4(0u, 0u, 0u, 0u);
        if (!valid || k0 >= K) continue;
        if constexpr (LNTAP) {
            const int tap = k0 / CIN, c = k0 - tap * CIN;
            const int iy = iy0 + (tap >> 1), ix = ix0 + (tap & 1);
            if (iy < 0 || iy >= p.Hin || ix < 0 || ix >= p.Win) continue;
            xr[s] = *reinterpret_cast<const uint4*>(X + (xbase + long(iy) * p.Win + ix) * p.ldx + c);
        } else {
            xr[s] = *reinterpret_cast<const uint4*>(X + xbase + k0);
        }
    }
    if constexpr (LNTAP) {
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        ACH_UNROLL
        for (int s = 0; s < KS; ++s) {
            float v[8];
            frag_unpack<T>(xr[s], v);
            float a1 = 0.f, a2 = 0.f;
            ACH_UNROLL
            for (int j = 0; j < VEC; ++j) { a1 += v[j]; a2 += v[j] * v[j]; }
            const int tp = (s * KC + g * VEC) / CIN;
            ACH_UNROLL
            for (int t = 0; t < 4; ++t) { s1[t] += tp == t ? a1 : 0.f; s2[t] += tp == t ? a2 : 0.f; }
        }
        float tmean[4], trstd[4];
        ACH_UNROLL
        for (int t = 0; t < 4; ++t) {
            s1[t] += __shfl_xor(s1[t], 16); s2[t] += __shfl_xor(s2[t], 16);
            s1[t] += __shfl_xor(s1[t], 32); s2[t] += __shfl_xor(s2[t], 32);
            const float mu = s1[t] / float(CIN);
            float var = s2[t] / float(CIN) - mu * mu;
            var = var > 0.f ? var : 0.f;
            tmean[t] = mu;
            trstd[t] = ln_rstd(var + p.ln_eps);
        }
        ACH_UNROLL
        for (int s = 0; s < KS; ++s) {
            const int tp = (s * KC + g * VEC) / CIN;
            const float mu = tp == 0 ? tmean[0] : (tp == 1 ? tmean[1] : (tp == 2 ? tmean[2] : tmean[3]));
            const float rs = tp == 0 ? trstd[0] : (tp == 1 ? trstd[1] : (tp == 2 ? trstd[2] : trstd[3]));
            float v[8];
            frag_unpack<T>(xr[s], v);
            ACH_UNROLL
            for (int j = 0; j < VEC; ++j) v[j] = (v[j] - mu) * rs;
            xr[s] = frag_pack<T>(v);
        }
    } else {
        float s1 = 0.f, s2 = 0.f;
        ACH_UNROLL
        for (int s = 0; s < KS; ++s) {
            float v[8];
            frag_unpack<T>(xr[s], v);                              // channels >= K loaded as 0
            ACH_UNROLL
            for (int j = 0; j < VEC; ++j) { s1 += v[j]; s2 += v[j] * v[j]; }
        }
        s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
        const float mean = s1 / float(K);
        float var = s2 / float(K) - mean * mean;
        var = var > 0.f ? var : 0.f;
        const float rstd = ln_rstd(var + p.ln_eps);
        ACH_UNROLL
        for (int s = 0; s < KS; ++s) {
            float v[8];
            frag_unpack<T>(xr[s], v);
            ACH_UNROLL
            for (int j = 0; j < VEC; ++j) v[j] = (v[j] - mean) * rstd;
            xr[s] = frag_pack<T>(v);
        }
    }
}

template <class T, int K, bool LNTAP, bool SHARE>
__global__ __launch_bounds__(SHARE ? 64 * LNG_MAX_WAVES : 256) void ln_gemm_rows_kernel(const GemmParams p) { f16_sat_mode<T>();
    constexpr int NT = 4, VEC = Store<T>::VEC, KC = 4 * VEC, KS = (K + KC - 1) / KC;
    constexpr int DEPTH = KS < LNG_DEPTH ? KS : LNG_DEPTH;
    __shared__ __attribute__((aligned(16))) uint4 xs[SHARE ? KS * 64 : 1];
    const int lane = threadIdx.x & 63, wave = wave_uniform(int(threadIdx.x >> 6));
    const int px = lane & 15, g = lane >> 4;
    const int grp = blockIdx.y;
    // SHARE: blockIdx.x = the 16-row tile; otherwise four tiles per workgroup in gemm_body's order (the patchify convs: XCD-aware, as there)
    const long row0 = SHARE ? long(blockIdx.x) * 16 : long(LNTAP ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x) * 64 + wave * 16;
    const long mloc = row0 + px;
    const bool valid = mloc < p.M_per_group;
    const long m = long(grp) * p.M_per_group + (valid ? mloc : 0);
    const uint4* Wf = reinterpret_cast<const uint4*>(static_cast<const T*>(p.W) + long(grp) * p.w_group_stride) + lane;
    const float* bias = p.bias + long(grp) * p.bias_group_stride;

    // this wave's chunks: c0, c0 + cstep, ... < c_end
    int c0, cstep, c_end;
    if constexpr (SHARE) { c0 = wave; cstep = int(blockDim.x >> 6); c_end = p.nchunks; }
    else { c0 = int(blockIdx.z) * p.chunks_per_block; cstep = 1; c_end = (c0 + p.chunks_per_block < p.nchunks) ? c0 + p.chunks_per_block : p.nchunks; }

    uint4 wb[DEPTH][NT];
    auto fill = [&](int d, int c, int s) {
        ACH_UNROLL
        for (int t = 0; t < NT; ++t) wb[d][t] = Wf[((long(c) * KS + s) * NT + t) * 64];
    };
    uint4 xr[KS];
    if constexpr (SHARE) {
        if (wave == 0) {
            ln_rows_phase_a<T, K, LNTAP>(p, valid, m, g, xr);
            ACH_UNROLL
            for (int s = 0; s < KS; ++s) xs[s * 64 + lane] = xr[s];
        }
        ACH_UNROLL
        for (int d = 0; d < DEPTH; ++d) fill(d, c0, d);               // (every wave has a chunk: NW <= nchunks) in flight while the wave waits at the barrier
        __syncthreads();
    } else {
        ln_rows_phase_a<T, K, LNTAP>(p, valid, m, g, xr);
        if (c0 < c_end) {
            ACH_UNROLL
            for (int d = 0; d < DEPTH; ++d) fill(d, c0, d);
        }
    }

    for (int c = c0; c < c_end; c += cstep) {
        const int cbase = c * (16 * NT);
        float bv[4 * NT];
        ACH_UNROLL
        for (int t = 0; t < NT; ++t) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + cbase + chunk_channel(NT, t, g, 0));
            bv[t * 4] = b4[0]; bv[t * 4 + 1] = b4[1]; bv[t * 4 + 2] = b4[2]; bv[t * 4 + 3] = b4[3];
        }
        f32x4 acc[NT];
        ACH_UNROLL
        for (int t = 0; t < NT; ++t) { acc[t][0] = 0.f; acc[t][1] = 0.f; acc[t][2] = 0.f; acc[t][3] = 0.f; }
        const int cn = c + cstep;
        ACH_UNROLL
        for (int s = 0; s < KS; ++s) {
            const int d = s % DEPTH;
            uint4 xf;
            if constexpr (SHARE) xf = xs[s * 64 + lane]; else xf = xr[s];
            ACH_UNROLL
            for (int t = 0; t < NT; ++t) mfma16<T>(wb[d][t], xf, acc[t]);
            if (s + DEPTH < KS) fill(d, c, s + DEPTH);
            else if (cn < c_end) fill(d, cn, s + DEPTH - KS);            // the ring runs on into the wave's next chunk
        }
        if (valid) ln_gemm_store_tile<T, NT>(p, acc, bv, m, cbase, g);
    }
}

// the instantiated (K, form) pairs: EdgeNeXt-S0's patchify convs (K = 4 Cin) and its LayerNorm + qkv widths
template <class T> inline bool ln_gemm_rows_has(int K, bool tap) {
    if constexpr (!is_h16<T>::value) return false;
    return tap ? (K == 128 || K == 192 || K == 384) : (K == 48 || K == 96 || K == 176);
}
// p as launch_gemm takes it (NT = 4, one 16-row sub-tile per wave): the chunk slices of blockIdx.z become the waves of a tile's workgroup
template <class T>
inline void launch_ln_gemm_rows(const GemmParams& p, hipStream_t stream) {
    if constexpr (is_h16<T>::value) {
        const int nw = cdiv(p.nchunks, p.chunks_per_block) < LNG_MAX_WAVES ? cdiv(p.nchunks, p.chunks_per_block) : LNG_MAX_WAVES;
        const bool share = nw > 1;
        const dim3 grid(unsigned(cdivl(p.M_per_group, share ? 16L : 64L)), unsigned(p.groups), 1u), block(share ? 64u * unsigned(nw) : 256u);
#define ACH_LNG_CASE(k, tap) if (p.K == k && (p.ln == 2) == tap) { \
            if (share) ACH_LAUNCH((ln_gemm_rows_kernel<T, k, tap, true>), grid, block, stream, p); \
            else ACH_LAUNCH((ln_gemm_rows_kernel<T, k, tap, false>), grid, block, stream, p); \
            return; }
        ACH_LNG_CASE(128, true) ACH_LNG_CASE(192, true) ACH_LNG_CASE(384, true)
        ACH_LNG_CASE(48, false) ACH_LNG_CASE(96, false) ACH_LNG_CASE(176, false)
#undef ACH_LNG_CASE
    }
}

}  // namespace ach
