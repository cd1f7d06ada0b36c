// api_train.cpp — the stateless entries of the training-mode kernels (k_train.h, k_train2.h, k_train3.h), the training losses (k_loss.h) and the validation
// metrics (k_metrics.h): argument checks and launch policy.  fp32, no handle; errors through ach_last_error(NULL).  See api.cpp / api_util.h.
// Also the optimizer step and weight EMA over the flat training-state arena (k_optim.h; declared in include/achelous_optim.h).
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>

#include "api_util.h"
#include "k_train.h"
#include "k_train2.h"
#include "k_train3.h"
#include "k_loss.h"
#include "k_metrics.h"
#include "k_optim.h"
#include "../../include/achelous_optim.h"

// in an entry: `st` is its stream.  One thread per element of `total`, or `nblocks` workgroups, of 256 threads
#define ACH_TRAIN_1D(kern, p, total) ACH_LAUNCH(kern, dim3(unsigned(ach::cdivl((total), 256))), dim3(256), st, p)
#define ACH_TRAIN_ROWS(kern, p, nblocks) ACH_LAUNCH(kern, dim3(unsigned(nblocks)), dim3(256), st, p)

static_assert(int(ach::CONF_F32) == KIND_F32 && int(ach::CONF_BF16) == KIND_BF16 && int(ach::CONF_F16) == KIND_F16 && int(ach::CONF_MAP_U8) == KIND_U8, "ach_eval_confusion's kinds are ElemKind");

extern "C" {

// ---- training-mode kernels (k_train.h): stateless, fp32, no handle
// scratch for split reductions: one buffer per DEVICE, grown on demand.  Its users are ordered on the caller's stream; training runs on one.
static float* train_workspace(size_t bytes) {
    static std::mutex mu;
    static std::map<int, std::pair<float*, size_t>> pool;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    auto& ent = pool[dev];
    if (bytes > ent.second) {
        if (ent.first) { (void)hipDeviceSynchronize(); (void)hipFree(ent.first); ent.first = nullptr; ent.second = 0; }
        const size_t want = std::max(bytes, size_t(8) << 20);
        if (hipMalloc(reinterpret_cast<void**>(&ent.first), want) != hipSuccess) { ent.first = nullptr; throw ach::AchError{ACH_ERR_NOMEM, "training workspace"}; }
        ent.second = want;
    }
    return ent.first;
}
// slices of a per-channel reduction over `total` values: ~16 K values per workgroup, at most ~2048 workgroups in all
static int train_slices(long total, int C) {
    const long want = (total + 16383) / 16384, cap = std::max<long>(1, 2048 / std::max(C, 1));
    return int(std::max<long>(1, std::min<long>(std::min<long>(want, cap), 64)));
}
// the slices of such a reduction and, above one slice, its workspace: `per_slice` floats for every slice
static int train_sliced(long total, int C, size_t per_slice, float*& ws) {
    const int S = train_slices(total, C);
    if (S > 1) ws = train_workspace(per_slice * S * sizeof(float));
    return S;
}
// element type of the training GEMMs' matrix-instruction operands, process-wide: 0 = fp32 (default), 1 = bf16 operands with fp32 accumulation (k_train.h)
static std::atomic<int> g_train_gemm_precision{0};
int ach_train_set_gemm_precision(int32_t precision) {
    if (precision != 0 && precision != 1) return ACH_ERR_INVALID;
    g_train_gemm_precision.store(precision, std::memory_order_relaxed);
    return ACH_OK;
}
int ach_train_get_gemm_precision(void) { return g_train_gemm_precision.load(std::memory_order_relaxed); }
int ach_train_gemm(const float* A, const float* B, float* C, const float* bias, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                   int64_t stride_a, int64_t stride_b, int64_t stride_c, int32_t trans_a, int32_t trans_b, int32_t batch, int32_t reduce_batch,
                   int32_t accumulate, void* stream) {
    return ach_train_gemm_p(A, B, C, bias, M, N, K, lda, ldb, ldc, stride_a, stride_b, stride_c, trans_a, trans_b, batch, reduce_batch, accumulate, -1, stream);
}
int ach_train_gemm_p(const float* A, const float* B, float* C, const float* bias, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                     int64_t stride_a, int64_t stride_b, int64_t stride_c, int32_t trans_a, int32_t trans_b, int32_t batch, int32_t reduce_batch,
                     int32_t accumulate, int32_t precision, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        if (precision < -1 || precision > 1) throw ach::AchError{ACH_ERR_INVALID, "train_gemm precision must be -1 (the process-wide setting), 0 (fp32) or 1 (bf16 operands)"};
        if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || batch <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_gemm arguments"};
        ach::TrainGemmParams p{A, B, C, bias, M, N, K, long(lda), long(ldb), long(ldc), long(stride_a), long(stride_b), long(stride_c), trans_a, trans_b, batch, reduce_batch, accumulate, 1, nullptr};
        // block tile: 32 rows / columns where the output has no more (k_train.h: the streaming shapes)
        const int tm = M <= 32 ? 32 : 64, tn = N <= 32 ? 32 : 64;
        dim3 grid(unsigned((N + tn - 1) / tn), unsigned((M + tm - 1) / tm), unsigned(reduce_batch ? 1 : batch));
        if (reduce_batch) {           // few output tiles, long reduction (weight gradients): split it over ~1024 workgroups, partial sums in a workspace
            const long T = long(batch) * ((K + ach::TRAIN_GEMM_TK - 1) / ach::TRAIN_GEMM_TK), tiles = long(grid.x) * grid.y;
            long split = std::min<long>(std::min<long>(2048 / tiles, T / 4), 2048);
            if (split > 1) {
                p.ksplit = int(split);
                p.ws = train_workspace(size_t(split) * M * N * sizeof(float));
                grid.z = unsigned(split);
            }
        }
        const bool h16 = (precision >= 0 ? precision : g_train_gemm_precision.load(std::memory_order_relaxed)) == 1;
#define ACH_TG_LAUNCH(TM, TN) { if (h16) ACH_LAUNCH((ach::train_gemm_kernel<ach::bf16_t, TM, TN>), grid, dim3(256), st, p); else ACH_LAUNCH((ach::train_gemm_kernel<float, TM, TN>), grid, dim3(256), st, p); }
        if (tm == 32 && tn == 32) ACH_TG_LAUNCH(32, 32)
        else if (tm == 32) ACH_TG_LAUNCH(32, 64)
        else if (tn == 32) ACH_TG_LAUNCH(64, 32)
        else ACH_TG_LAUNCH(64, 64)
#undef ACH_TG_LAUNCH
        if (p.ksplit > 1) ACH_TRAIN_ROWS(ach::train_gemm_reduce_kernel, p, ach::cdivl(long(M) * N, 16));
    });
}
int ach_train_bn_stats(const float* z, float* mean, float* var, int32_t B, int32_t C, int32_t N, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        if (!z || !mean || !var || B <= 0 || C <= 0 || N <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_stats arguments"};
        float* ws = nullptr;
        const int S = train_sliced(long(B) * N, C, size_t(2) * C, ws);
        if (S > 1) {
            ach::BnSliceParams q{z, ws, mean, var, B, C, N, S};
            ACH_LAUNCH(ach::train_bn_slice2_kernel, dim3(unsigned(C), unsigned(S)), dim3(256), st, q);          // both passes of a slice, the second out of the L2
            ACH_TRAIN_1D(ach::train_bn_slice2_finalize_kernel, q, C);
            return;
        }
        ach::BnStatsParams p{z, mean, var, B, C, N};
        ACH_TRAIN_ROWS(ach::train_bn_stats_kernel, p, C);
    });
}
int ach_train_bn_running(const float* mean, const float* var, float* running_mean, float* running_var, int32_t C, float momentum, float unbias, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        if (!mean || !var || !running_mean || !running_var || C <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_running arguments"};
        ach::BnRunningParams p{mean, var, running_mean, running_var, C, momentum, unbias};
        ACH_TRAIN_1D(ach::train_bn_running_kernel, p, C);
    });
}
int ach_train_bn_relu_fwd(const float* z, const float* mean, const float* var, const float* gamma, const float* beta, float* y, int32_t B, int32_t C,
                          int32_t N, float eps, int32_t relu, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        if (!z || !mean || !var || !gamma || !beta || !y || B <= 0 || C <= 0 || N <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_relu_fwd arguments"};
        ach::BnReluFwdParams p{z, mean, var, gamma, beta, y, B, C, N, eps, relu};
        const bool quad = quad_ok(N, z, y) && long(B) * C <= 65535;      // a plane per blockIdx.y, four positions per thread
        if (quad) ACH_LAUNCH(ach::train_bn_relu_fwd4_kernel, dim3(unsigned(ach::cdivl(long(N) / 4, 256)), unsigned(long(B) * C)), dim3(256), st, p);
        else ACH_TRAIN_1D(ach::train_bn_relu_fwd_kernel, p, long(B) * C * N);
    });
}
int ach_train_bn_relu_bwd(const float* z, const float* y, const float* dy, const float* mean, const float* var, const float* gamma, float* dgamma,
                          float* dbeta, float* dz, int32_t B, int32_t C, int32_t N, float eps, int32_t relu, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        if (!z || !y || !dy || !mean || !var || !gamma || !dgamma || !dbeta || !dz || B <= 0 || C <= 0 || N <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_relu_bwd arguments"};
        ach::BnReluBwdParams p{z, y, dy, mean, var, gamma, dgamma, dbeta, dz, B, C, N, eps, relu, 1, nullptr};
        p.S = train_sliced(long(B) * N, C, size_t(2) * C, p.ws);
        ACH_LAUNCH(ach::train_bn_relu_bwd_reduce_kernel, dim3(unsigned(C), unsigned(p.S)), dim3(256), st, p);
        if (p.S > 1) ACH_TRAIN_1D(ach::train_bn_relu_bwd_finalize_kernel, p, C);
        const bool quad = quad_ok(N, z, y, dy, dz) && long(B) * C <= 65535;
        if (quad) ACH_LAUNCH(ach::train_bn_relu_bwd_apply4_kernel, dim3(unsigned(ach::cdivl(long(N) / 4, 256)), unsigned(long(B) * C)), dim3(256), st, p);
        else ACH_TRAIN_1D(ach::train_bn_relu_bwd_apply_kernel, p, long(B) * C * N);
    });
}

int ach_train_max_points(const float* x, float* y, int32_t* idx, const float* dy, float* dx, int64_t rows, int32_t N, void* stream) {
    return stateless(stream, [&](hipStream_t st) {                                 /* forward when dy == NULL, backward otherwise */
        if (rows <= 0 || N <= 0 || !idx) throw ach::AchError{ACH_ERR_INVALID, "bad train_max_points arguments"};
        if (!dy) {
            if (!x || !y) throw ach::AchError{ACH_ERR_INVALID, "bad train_max_points arguments"};
            ach::MaxPtsParams p{x, y, idx, long(rows), N};
            ACH_TRAIN_ROWS(ach::train_max_points_fwd_kernel, p, ach::cdivl(long(rows), 4));
        } else {
            if (!dx) throw ach::AchError{ACH_ERR_INVALID, "bad train_max_points arguments"};
            ach::MaxPtsBwdParams p{dy, idx, dx, long(rows), N};
            ACH_TRAIN_1D(ach::train_max_points_bwd_kernel, p, long(rows) * N);
        }
    });
}
int ach_train_log_softmax(const float* z, float* y, const float* dy, float* dz, int32_t B, int32_t K, int32_t N, void* stream) {
    return stateless(stream, [&](hipStream_t st) {                                 /* forward when dy == NULL (z -> y [B,N,K]); backward: y, dy -> dz [B,K,N] */
        if (B <= 0 || K <= 0 || N <= 0 || !y) throw ach::AchError{ACH_ERR_INVALID, "bad train_log_softmax arguments"};
        ach::LsmTrainParams p{z, y, dy, dz, B, K, N};
        if (!(dy ? dz : z)) throw ach::AchError{ACH_ERR_INVALID, "bad train_log_softmax arguments"};
        if (!dy) ACH_TRAIN_1D(ach::train_log_softmax_fwd_kernel, p, long(B) * N);
        else ACH_TRAIN_1D(ach::train_log_softmax_bwd_kernel, p, long(B) * N);
    });
}

// ---- training-mode primitives of k_train2.h
int ach_train_act(const float* x, const float* dy, float* out, int64_t n, int32_t kind, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && out && n > 0 && kind >= 0 && kind <= 3, "ach_train_act");
        ach::TrainActParams p{x, dy, out, long(n), kind};
        if (quad_ok(n, x, dy, out)) ACH_TRAIN_1D(ach::train_act4_kernel, p, long(n) / 4);
        else ACH_TRAIN_1D(ach::train_act_kernel, p, long(n));
    });
}
int ach_train_mul(const float* a, const float* b, float* out, int64_t n, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(a && b && out && n > 0, "ach_train_mul");
        ach::TrainMulParams p{a, b, out, long(n)};
        ACH_TRAIN_1D(ach::train_mul_kernel, p, long(n));
    });
}
int ach_train_layernorm(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows, int32_t C, int64_t inner,
                        float eps, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && gamma && beta && y && mean && rstd && rows > 0 && C > 0 && inner > 0, "ach_train_layernorm");
        ach::TrainLnParams p{x, gamma, beta, y, mean, rstd, long(rows), C, long(inner), eps};
        if (quad_ok(inner, x, y, mean, rstd)) ACH_TRAIN_1D(ach::train_ln_fwd4_kernel, p, long(rows) * (inner / 4));
        else ACH_TRAIN_1D(ach::train_ln_fwd_kernel, p, long(rows) * inner);
    });
}
int ach_train_layernorm_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                            int64_t rows, int32_t C, int64_t inner, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && dy && gamma && mean && rstd && dx && dgamma && dbeta && rows > 0 && C > 0 && inner > 0, "ach_train_layernorm_bwd");
        ach::TrainLnBwdParams p{x, dy, gamma, mean, rstd, dx, dgamma, dbeta, long(rows), C, long(inner), 1, nullptr};
        if (quad_ok(inner, x, dy, dx, mean, rstd)) ACH_TRAIN_1D(ach::train_ln_bwd_dx4_kernel, p, long(rows) * (inner / 4));
        else ACH_TRAIN_1D(ach::train_ln_bwd_dx_kernel, p, long(rows) * inner);
        p.S = train_sliced(long(rows) * inner, C, size_t(2) * C, p.ws);
        ACH_LAUNCH(ach::train_ln_bwd_param_kernel, dim3(unsigned(C), unsigned(p.S)), dim3(256), st, p);
        if (p.S > 1) ACH_TRAIN_1D(ach::train_ln_bwd_param_finalize_kernel, p, C);
    });
}
int ach_train_dwconv(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, int32_t flip, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && w && y && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && (k & 1), "ach_train_dwconv");
        ach::TrainDwParams p{x, w, bias, y, B, C, H, W, k, flip};
        const bool quad = quad_ok(W, y) && long(B) * C <= 65535;      // four outputs of a row per thread (k_train2.h)
        const dim3 gq(unsigned(ach::cdivl(long(H) * (W / 4), 256)), unsigned(long(B) * C));
        const long total = long(B) * C * H * W;
        if (quad && odd_k(k, [&](auto K) { ACH_LAUNCH(ach::train_dwconv4_kernel<decltype(K)::value>, gq, dim3(256), st, p); })) return;
        if (!odd_k(k, [&](auto K) { ACH_TRAIN_1D(ach::train_dwconv_kernel<decltype(K)::value>, p, total); })) ACH_TRAIN_1D(ach::train_dwconv_kernel<0>, p, total);
    });
}
int ach_train_dwconv_wgrad(const float* x, const float* dz, float* dw, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && dz && dw && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && (k & 1), "ach_train_dwconv_wgrad");
        ach::TrainDwWgradParams p{x, dz, dw, B, C, H, W, k, 1, nullptr};
        const bool taps = odd_k(k, [](auto) {}) && long(B) * H * W < (1L << 31);      // all taps of a channel in one pass (k_train2.h)
        p.S = train_sliced(long(B) * H * W, taps ? C : C * k * k, size_t(C) * k * k, p.ws);
        const dim3 gt(unsigned(C), unsigned(p.S));
        if (!(taps && odd_k(k, [&](auto K) { ACH_LAUNCH(ach::train_dwconv_wgrad_taps_kernel<decltype(K)::value>, gt, dim3(256), st, p); })))
            ACH_LAUNCH(ach::train_dwconv_wgrad_kernel, dim3(unsigned(C * k * k), unsigned(p.S)), dim3(256), st, p);
        if (p.S > 1) ACH_TRAIN_1D(ach::train_dwconv_wgrad_finalize_kernel, p, C * k * k);
    });
}
int ach_train_im2col(const float* src, float* dst, int32_t B, int32_t C, int32_t H, int32_t W, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                     int32_t Ho, int32_t Wo, int32_t backward, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && Ho > 0 && Wo > 0, "ach_train_im2col");
        ach::TrainColParams p{src, dst, B, C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo};
        if (!backward) ACH_TRAIN_1D(ach::train_im2col_kernel, p, long(B) * C * kh * kw * Ho * Wo);
        else ACH_TRAIN_1D(ach::train_col2im_kernel, p, long(B) * C * H * W);
    });
}
int ach_train_softmax(const float* x, float* y, const float* dy, float* dx, int64_t rows, int32_t d, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(y && rows > 0 && d > 0 && (dy ? dx != nullptr : x != nullptr), "ach_train_softmax");
        ach::TrainSoftmaxParams p{x, y, dy, dx, long(rows), d};
        ACH_TRAIN_1D(ach::train_softmax_kernel, p, long(rows));
    });
}
int ach_train_upsample2x(const float* src, float* dst, int64_t planes, int32_t h, int32_t w, int32_t backward, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(src && dst && planes > 0 && h > 0 && w > 0, "ach_train_upsample2x");
        ach::TrainUpParams p{src, dst, long(planes), h, w, h > 1 ? float(h - 1) / float(2 * h - 1) : 0.f, w > 1 ? float(w - 1) / float(2 * w - 1) : 0.f};
        if (!backward) ACH_TRAIN_1D(ach::train_up2_fwd_kernel, p, long(planes) * 4 * h * w);
        else ACH_TRAIN_1D(ach::train_up2_bwd_kernel, p, long(planes) * h * w);
    });
}
int ach_train_maxpool(const float* x, float* y, int32_t* idx, const float* dy, float* dx, int64_t planes, int32_t H, int32_t W, int32_t k, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(idx && planes > 0 && H > 0 && W > 0 && k > 0 && (k & 1) && (dy ? dx != nullptr : (x && y)), "ach_train_maxpool");
        ach::TrainPoolParams p{x, y, idx, dy, dx, long(planes), H, W, k};
        ACH_TRAIN_1D(ach::train_maxpool_kernel, p, long(planes) * H * W);
    });
}
int ach_train_avgpool3(const float* x, float* y, int64_t planes, int32_t H, int32_t W, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && y && planes > 0 && H > 0 && W > 0, "ach_train_avgpool3");
        ach::TrainPoolParams p{x, y, nullptr, nullptr, nullptr, long(planes), H, W, 3};
        ACH_TRAIN_1D(ach::train_avgpool3_kernel, p, long(planes) * H * W);
    });
}
int ach_train_row_reduce(const float* a, const float* b, float* out, int64_t rows, int64_t n, float scale, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(a && out && rows > 0 && n > 0, "ach_train_row_reduce");
        ach::TrainRowParams p{a, b, out, long(rows), long(n), 1, scale};
        ACH_TRAIN_ROWS(ach::train_row_reduce_kernel, p, rows);
    });
}
int ach_train_row_scale(const float* x, const float* s, float* out, int64_t rows, int64_t n, int64_t period, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(s && out && rows > 0 && n > 0 && period > 0, "ach_train_row_scale");
        ach::TrainRowParams p{x, s, out, long(rows), long(n), long(period), 1.f};
        ACH_TRAIN_1D(ach::train_row_scale_kernel, p, long(rows) * n);
    });
}
int ach_train_col_reduce(const float* a, const float* b, float* out, int64_t rows, int64_t cols, float scale, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(a && out && rows > 0 && cols > 0, "ach_train_col_reduce");
        ach::TrainRowParams p{a, b, out, long(rows), long(cols), 1, scale};
        ACH_TRAIN_ROWS(ach::train_col_reduce_kernel, p, cols);
    });
}
int ach_train_col_scale(const float* x, const float* g, float* out, int64_t rows, int64_t cols, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && g && out && rows > 0 && cols > 0, "ach_train_col_scale");
        ach::TrainRowParams p{x, g, out, long(rows), long(cols), 1, 1.f};
        ACH_TRAIN_1D(ach::train_col_scale_kernel, p, long(rows) * cols);
    });
}
int ach_train_instnorm(const float* x, const float* dy, const float* gamma, const float* beta, float* y, float* mean, float* rstd, float* dx, float* dgamma_rows,
                       float* dbeta_rows, int64_t rows, int64_t n, int32_t C, float eps, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && gamma && mean && rstd && rows > 0 && n > 0 && C > 0 && (dy ? (dx && dgamma_rows && dbeta_rows) : (y && beta)), "ach_train_instnorm");
        ach::TrainInParams p{x, dy, gamma, beta, y, mean, rstd, dx, dgamma_rows, dbeta_rows, long(rows), long(n), C, eps};
        ACH_TRAIN_ROWS(ach::train_instnorm_kernel, p, rows);
    });
}
int ach_train_l2norm(const float* x, float* y, float* norm, const float* dy, float* dx, int64_t rows, int64_t n, float eps, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && norm && rows > 0 && n > 0 && (dy ? dx != nullptr : y != nullptr), "ach_train_l2norm");
        ach::TrainL2Params p{x, y, norm, dy, dx, long(rows), long(n), eps};
        ACH_TRAIN_ROWS(ach::train_l2norm_kernel, p, rows);
    });
}
int ach_train_deform_im2col(const float* x, const float* offset, const float* mask, float* col, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                            int32_t stride, int32_t pad, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && offset && mask && col && B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && stride > 0, "ach_train_deform_im2col");
        ach::TrainDeformParams p{x, offset, mask, col, nullptr, nullptr, nullptr, nullptr, B, C, H, W, Ho, Wo, stride, pad};
        ACH_TRAIN_1D(ach::train_deform_im2col_kernel, p, long(B) * C * 9 * Ho * Wo);
    });
}
int ach_train_deform_bwd(const float* x, const float* offset, const float* mask, const float* dcol, float* dx_zeroed, float* doffset, float* dmask, int32_t B,
                         int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t stride, int32_t pad, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(x && offset && mask && dcol && doffset && dmask && B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && stride > 0, "ach_train_deform_bwd");
        ach::TrainDeformParams p{x, offset, mask, nullptr, dcol, dx_zeroed, doffset, dmask, B, C, H, W, Ho, Wo, stride, pad};
        ACH_TRAIN_1D(ach::train_deform_bwd_coord_kernel, p, long(B) * 9 * Ho * Wo);
        // (dx_zeroed = NULL: the input needs no gradient — the first RCBlock reads the pooled radar map.  An LDS-combining form of this scatter — a workgroup per 16 x 16 tile of
        //  positions, LDS atomics, one L2 atomic per touched input pixel instead of 36 per position — was measured 4x SLOWER end to end (batch-32 step 64.5 -> 86.7 ms) and is not kept.)
        if (dx_zeroed) ACH_TRAIN_1D(ach::train_deform_bwd_input_kernel, p, long(B) * C * 9 * Ho * Wo);
    });
}
// ---- PointNet++ in training mode (k_train3.h): the inference engine's geometry kernels at fp32 + the two scatter-form adjoints
int ach_train_pn2_fps(const float* xyz, int32_t B, int32_t n, int32_t npoint, int32_t* idx, float* new_xyz, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(xyz && idx && new_xyz && B > 0 && n > 0 && npoint > 0 && npoint <= n && n <= 64 * ach::PN2_FPS_MAX_PPT, "ach_train_pn2_fps");
        ach::launch_pn2_fps(ach::FpsParams{xyz, n, npoint, idx, new_xyz}, B, st);
    });
}
int ach_train_pn2_group(const float* xyz, const float* new_xyz, const float* feats, int32_t C, int32_t B, int32_t n, int32_t S, int32_t nsample, float radius2,
                        float* grouped, int32_t* group_idx, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(xyz && new_xyz && (feats || C == 0) && grouped && group_idx && C >= 0 && B > 0 && n > 0 && S > 0 && nsample > 0 && nsample <= ach::PN2_MAX_NSAMPLE, "ach_train_pn2_group");
        ach::GroupParams q{xyz, new_xyz, feats, long(C), C, grouped, long(3 + C), group_idx, B, n, S, nsample, radius2, 1};
        ACH_TRAIN_ROWS(ach::pn2_group_kernel<float>, q, ach::cdivl(long(B) * S, 4));
    });
}
int ach_train_pn2_group_bwd(const int32_t* group_idx, const float* dgrouped, float* dfeats_zeroed, int32_t C, int32_t B, int32_t n, int32_t S, int32_t nsample, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(group_idx && dgrouped && dfeats_zeroed && C > 0 && B > 0 && n > 0 && S > 0 && nsample > 0, "ach_train_pn2_group_bwd");
        ach::Pn2GroupBwdParams q{group_idx, dgrouped, long(3 + C), dfeats_zeroed, C, B, n, S, nsample};
        ACH_TRAIN_1D(ach::train_pn2_group_bwd_kernel, q, long(B) * S * nsample * C);
    });
}
int ach_train_pn2_interp(const float* xyz1, const float* xyz2, const float* skip, int32_t C1, const float* sparse, int32_t C2, float* out, float* dskip, float* dsparse_zeroed,
                         const float* dout, int32_t B, int32_t n, int32_t s, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(xyz1 && xyz2 && C1 >= 0 && C2 > 0 && B > 0 && n > 0 && s >= 3 && s <= 64 * ach::PN2_INTERP_SPL, "ach_train_pn2_interp");
        const dim3 grid(unsigned(ach::cdivl(long(B) * n, 4))), block(256);
        if (!dout) {
            need((skip || C1 == 0) && sparse && out, "ach_train_pn2_interp (forward)");
            ach::InterpParams q{xyz1, xyz2, skip, long(C1), C1, sparse, long(C2), C2, out, long(C1 + C2), B, n, s};
            ACH_LAUNCH(ach::pn2_interp_kernel<float>, grid, block, st, q);
        } else {
            need((dskip || C1 == 0) && dsparse_zeroed, "ach_train_pn2_interp (backward)");
            ach::InterpParams q{xyz1, xyz2, nullptr, long(C1), C1, nullptr, long(C2), C2, nullptr, long(C1 + C2), B, n, s};
            ACH_LAUNCH(ach::train_pn2_interp_bwd_kernel, grid, block, st, q, dout, dskip, dsparse_zeroed);
        }
    });
}

// ---- training losses (k_loss.h): stateless, fp32, no host read — capturable.  Workspaces are the caller's.
int ach_train_yolo_loss(const float* raw0, const float* raw1, const float* raw2, const float* boxes, const int32_t* counts, int32_t B, int32_t C, int32_t G,
                        int32_t H0, int32_t W0, int32_t H1, int32_t W1, int32_t H2, int32_t W2, float s0, float s1, float s2, int32_t* claim_anchor, float* claim_cost,
                        float* claim_iou, int32_t* matched, float* pred_iou, int32_t* num_fg, float* grad, float* partial, float* loss, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(raw0 && raw1 && raw2 && boxes && counts && claim_anchor && claim_cost && claim_iou && matched && pred_iou && num_fg && grad && partial && loss, "ach_train_yolo_loss");
        need(B > 0 && B <= 65535 && C > 0 && G > 0 && G <= ach::YL_MAXG && H0 > 0 && W0 > 0 && H1 > 0 && W1 > 0 && H2 > 0 && W2 > 0, "ach_train_yolo_loss");
        const long n0 = long(H0) * W0, n1 = long(H1) * W1, n2 = long(H2) * W2, A = n0 + n1 + n2;
        need(A <= ach::YL_MAXA, "ach_train_yolo_loss: more anchors than the assignment holds (inputs up to 512 x 512)");
        ach::YoloLossParams p{};
        p.raw0 = raw0; p.raw1 = raw1; p.raw2 = raw2;
        p.W0 = W0; p.W1 = W1; p.W2 = W2; p.off1 = int(n0); p.off2 = int(n0 + n1); p.A = int(A);
        p.s0 = s0; p.s1 = s1; p.s2 = s2;
        p.boxes = boxes; p.counts = counts; p.B = B; p.C = C; p.G = G;
        p.claim_a = claim_anchor; p.claim_cost = claim_cost; p.claim_iou = claim_iou;
        p.matched = matched; p.pred_iou = pred_iou; p.num_fg = num_fg;
        p.grad = grad; p.g1 = long(B) * (5 + C) * n0; p.g2 = p.g1 + long(B) * (5 + C) * n1;
        const unsigned ablocks = unsigned((A + 255) / 256);
        p.partial = partial; p.loss = loss; p.nblk = int(ablocks) * B;
        ACH_LAUNCH(ach::yolo_assign_kernel, dim3(unsigned(G), unsigned(B)), dim3(256), st, p);
        ACH_TRAIN_ROWS(ach::yolo_resolve_kernel, p, B);
        ACH_LAUNCH(ach::yolo_loss_kernel, dim3(ablocks, unsigned(B)), dim3(256), st, p);
        ACH_TRAIN_ROWS(ach::yolo_reduce_kernel, p, 1);
    });
}
int ach_train_loss_scale(const float* g, const float* scale, float* out, int64_t n, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(g && scale && out && n > 0, "ach_train_loss_scale");
        ach::LossScaleParams p{g, scale, out, long(n)};
        ACH_TRAIN_1D(ach::loss_scale_kernel, p, long(n));
    });
}
// workgroups of the segmentation-loss kernels: 256 threads x V pixels each, grid-stride above 768 = three resident workgroups on each of the 256 compute units
// (measured at batch 32, 9 classes: 0.180 ms forward + backward against 0.192 with 1024 and 0.204 with 512; the caller's `partial` holds 1024 rows)
static int seg_loss_blocks(long items) { return int(std::max<long>(1, std::min<long>(ach::cdivl(items, 256), 768))); }
int ach_train_seg_loss(const float* logits, const void* labels, int32_t label_kind, const float* weights, int32_t B, int32_t C, int64_t HW, int32_t mode, int32_t dice,
                       float alpha, float gamma, float beta, float smooth, float* partial, float* stats, const float* cot, float* dlogits, void* stream) {
    return stateless(stream, [&](hipStream_t st) {                                 /* forward when cot == NULL (-> stats), backward otherwise (stats, cot -> dlogits) */
        need(logits && labels && partial && stats && B > 0 && C > 0 && C <= ach::SEG_MAXC && HW > 0 && label_kind >= 0 && label_kind <= 2 && mode >= 0 && mode <= 2, "ach_train_seg_loss");
        need(mode == 2 || weights != nullptr, "ach_train_seg_loss: class weights");
        need(cot ? dlogits != nullptr : true, "ach_train_seg_loss");
        ach::SegLossParams p{logits, labels, label_kind, weights, B, C, long(HW), mode, dice, alpha, gamma, beta, smooth, partial, 0, stats, cot, dlogits};
        const bool quad = quad_ok(HW, logits, dlogits);
        p.nblk = seg_loss_blocks(long(B) * (quad ? HW / 4 : HW));
        if (quad) ach::seg_loss_launch<4>(p, cot != nullptr, st); else ach::seg_loss_launch<1>(p, cot != nullptr, st);
        if (!cot) ACH_TRAIN_ROWS(ach::seg_reduce_kernel, p, 1);
    });
}

// ---- validation metrics (k_metrics.h): stateless, no host read, no synchronisation — one launch each.  Every buffer is the caller's.
int ach_eval_confusion(const void* pred, int32_t pred_kind, int32_t layout, const void* labels, int32_t label_kind, int32_t B, int32_t n, int64_t HW, uint64_t* hist,
                       void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(pred && labels && hist && B > 0 && HW > 0 && pred_kind >= 0 && pred_kind <= 3 && (layout == 0 || layout == 1) && label_kind >= 0 && label_kind <= 2, "ach_eval_confusion");
        need(n >= 1 && n <= ach::CONF_MAXN, "ach_eval_confusion: 1 <= n <= 16 classes");
        ach::ConfusionParams p{pred, layout, labels, label_kind, B, n, long(HW), reinterpret_cast<unsigned long long*>(hist)};
        const int V = ach::conf_vec(pred_kind);
        const bool vec = (pred_kind == ach::CONF_MAP_U8 || layout == 0) && HW % V == 0 && aligned16(pred, labels);
        const long items = long(B) * (vec ? HW / V : HW);
        const int nblk = int(std::max<long>(1, std::min<long>(ach::cdivl(items, 256), ach::CONF_BLOCKS)));
        need(ach::cdivl(long(B) * HW, nblk) < (1L << 31), "ach_eval_confusion: too many pixels for one call (the per-workgroup bins are 32-bit)");
        by_kind<ach::conf_u8>(pred_kind, [&](auto e) { ach::confusion_launch<typename decltype(e)::type>(p, vec, nblk, st); });
    });
}
int ach_eval_match(const float* rows, const int32_t* counts, int32_t yx_order, int32_t truncate, const float* gt, const uint8_t* difficult, const int32_t* gt_counts,
                   int32_t B, int32_t max_det, int32_t G, int32_t C, const double* thresholds, int32_t T, uint8_t* flags, int32_t* match, double* iou, float* score,
                   uint64_t* gt_per_class, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(rows && counts && gt && gt_counts && thresholds && flags && match && iou && score && gt_per_class, "ach_eval_match");
        need(B > 0 && max_det > 0 && max_det <= ach::MATCH_MAXD && G > 0 && G <= ach::MATCH_MAXG && C > 0 && T > 0 && T <= ach::MATCH_MAXT, "ach_eval_match: max_det <= 1024, G <= 128, T <= 10");
        ach::MatchParams p{};
        p.rows = rows; p.counts = counts; p.yx_order = yx_order != 0; p.truncate = truncate != 0;
        p.gt = gt; p.difficult = difficult; p.gt_counts = gt_counts;
        p.B = B; p.D = max_det; p.G = G; p.C = C; p.T = T;
        for (int t = 0; t < T; ++t) p.thr[t] = thresholds[t];
        p.flags = flags; p.match = match; p.iou = iou; p.score = score; p.gt_per_class = reinterpret_cast<unsigned long long*>(gt_per_class);
        ACH_TRAIN_ROWS(ach::match_kernel, p, B);
    });
}

// ---- optimizer step and weight EMA (k_optim.h, include/achelous_optim.h): stateless, every buffer the caller's.  The kernels index by chunk number below `chunks` only.
int ach_optim_tick(double* hyper, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(hyper && (reinterpret_cast<uintptr_t>(hyper) & 7u) == 0, "ach_optim_tick");
        ACH_LAUNCH(ach::optim_tick_kernel, dim3(1), dim3(64), st, hyper);
    });
}
// workgroups of the step: four chunks (4 KB of every arena) per workgroup and iteration, grid-stride above 2048 = eight resident workgroups on each of the 256 compute
// units, enough 16-byte requests in flight to stream from HBM
static int optim_blocks(long chunks) { return int(std::max<long>(1, std::min<long>(ach::cdivl(chunks, 4), 2048))); }
int ach_optim_step(float* state, float* ema, const float* grad, float* m1, float* m2, const int32_t* flags, int32_t* t, const double* hyper, int64_t chunks,
                   int64_t param_chunks, int32_t kind, int32_t nesterov, double momentum, double beta1, double beta2, double eps, void* stream) {
    return stateless(stream, [&](hipStream_t st) {
        need(state && grad && flags && hyper, "ach_optim_step: state, grad, flags and hyper");
        need(chunks > 0 && param_chunks > 0 && param_chunks <= chunks && chunks <= (int64_t(1) << 30), "ach_optim_step: 0 < param_chunks <= chunks <= 2^30");
        need(kind >= ach::OPT_SGD && kind <= ach::OPT_ADAMW, "ach_optim_step: kind 0 (sgd), 1 (adam) or 2 (adamw)");
        need(kind == ach::OPT_SGD ? (momentum == 0.0 || m1 != nullptr) : (m1 && m2 && t), "ach_optim_step: m1 for momentum; m1, m2 and t for Adam");
        need(kind == ach::OPT_SGD || (beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0), "ach_optim_step: betas in [0, 1), eps >= 0");
        need(aligned16(state, ema, grad, m1, m2) && (reinterpret_cast<uintptr_t>(hyper) & 7u) == 0 && ((reinterpret_cast<uintptr_t>(flags) | reinterpret_cast<uintptr_t>(t)) & 3u) == 0,
             "ach_optim_step: arenas 16-byte aligned");
        ach::OptimStepParams p{state, ema, grad, m1, m2, flags, t, hyper, int(chunks), int(param_chunks), kind, nesterov != 0, float(momentum), beta1, beta2, eps};
        ACH_LAUNCH(ach::optim_step_kernel, dim3(unsigned(optim_blocks(long(chunks)))), dim3(256), st, p);
    });
}

}  // extern "C"
