// api.cpp — the extern "C" boundary of libachelous_hip.so (declared in include/achelous.h).
// No exception crosses it: every failure becomes a negative code + a message retrievable with ach_last_error().
#include <atomic>
#include <cstring>
#include <functional>
#include <string>

#include "engine.h"
#include <map>
#include <mutex>
#include <algorithm>
#include "k_detect.h"
#include "k_prepost.h"
#include "k_train.h"
#include "k_train2.h"
#include "k_train3.h"
#include "k_loss.h"
#include "k_metrics.h"
#include "k_data.h"
#include "k_radarmap.h"
#include "k_serve.h"
#include "k_draw.h"

struct ach_handle {
    ach::EngineBase* eng = nullptr;
    std::string err;
};

static thread_local std::string g_create_error;

template <class F>
static int guarded(ach_handle* h, F&& f) {
    if (!h || !h->eng) return ACH_ERR_INVALID;
    try {
        f();
        return ACH_OK;
    } catch (const ach::AchError& e) {
        h->err = e.msg;
        return e.code;
    } catch (const std::exception& e) {
        h->err = e.what();
        return ACH_ERR_INVALID;
    } catch (...) {
        h->err = "unknown error";
        return ACH_ERR_INVALID;
    }
}

extern "C" {

int ach_create(const ach_config* cfg, ach_handle** out) {
    if (!cfg || !out) return ACH_ERR_INVALID;
    try {
        if (cfg->backbone != ACH_BACKBONE_EDGENEXT && cfg->backbone != ACH_BACKBONE_MOBILEVIT)
            throw ach::AchError{ACH_ERR_UNSUPPORTED, "backbone must be 'en' or 'mv'"};
        if (cfg->phi < ACH_PHI_S0 || cfg->phi > ACH_PHI_S2) throw ach::AchError{ACH_ERR_UNSUPPORTED, "phi must be S0, S1 or S2"};
        if (cfg->neck != ACH_NECK_GDF && cfg->neck != ACH_NECK_CDF) throw ach::AchError{ACH_ERR_UNSUPPORTED, "neck must be 'gdf' or 'cdf'"};
        if (cfg->pc_seg != ACH_PCSEG_PN && cfg->pc_seg != ACH_PCSEG_PN2 && cfg->pc_seg != ACH_PCSEG_NONE && cfg->pc_seg != ACH_PCSEG_PN2_MSG)
            throw ach::AchError{ACH_ERR_UNSUPPORTED, "pc_seg must be 'pn', 'pn2', 'pn2_msg' or none (Achelous3T)"};
        if (cfg->num_det < 1 || cfg->num_det > 59 || cfg->num_seg < 1 || (cfg->pc_seg != ACH_PCSEG_NONE && (cfg->pc_classes < 1 || cfg->pc_channels < 3)))
            throw ach::AchError{ACH_ERR_INVALID, "bad class / channel counts"};
        ach_handle* h = new ach_handle();
        h->eng = ach::make_engine(*cfg);
        *out = h;
        return ACH_OK;
    } catch (const ach::AchError& e) {
        g_create_error = e.msg;
        return e.code;
    } catch (...) {
        g_create_error = "allocation failure";
        return ACH_ERR_NOMEM;
    }
}

void ach_destroy(ach_handle* h) {
    if (!h) return;
    delete h->eng;
    delete h;
}

const char* ach_last_error(const ach_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ach_load_weights(ach_handle* h, const ach_tensor_desc* tensors, size_t n) {
    return guarded(h, [&] { h->eng->load(tensors, n); });
}

// options: lookups in the table of engine_options.h (engine.cpp).  ach_get_option reads the engine only; a failure still sets the handle's last error.
int ach_set_option(ach_handle* h, const char* key, int32_t value) { return guarded(h, [&] { h->eng->set_option(key, value); }); }
int ach_get_option(const ach_handle* h, const char* key, int32_t* value) {
    return guarded(const_cast<ach_handle*>(h), [&] { if (!value) throw ach::AchError{ACH_ERR_INVALID, "null option value"}; *value = h->eng->get_option(key); });
}
const char* ach_option_key(int32_t index) { return ach::EngineBase::option_key(index); }

int ach_plan(ach_handle* h, int32_t batch) {
    return guarded(h, [&] { h->eng->plan(batch); });
}

size_t ach_arena_bytes(const ach_handle* h) { return (h && h->eng) ? h->eng->aarena_used + h->eng->warena_used : 0; }

int ach_forward(ach_handle* h, const void* image, const void* radar, const void* points, void* det3, void* det4, void* det5,
                void* se_seg, void* lane_seg, void* pc_seg, void* stream) {
    return guarded(h, [&] {
        if (h->eng->ops.empty()) throw ach::AchError{ACH_ERR_INVALID, "ach_plan must precede ach_forward"};
        if (!image || !radar || !det3 || !det4 || !det5 || !se_seg || !lane_seg || (h->eng->cfg.pc_seg != ACH_PCSEG_NONE && (!points || !pc_seg)))
            throw ach::AchError{ACH_ERR_INVALID, "null input/output pointer"};
        ach::IoPtrs& io = h->eng->io;
        io.image = image; io.radar = radar; io.points = points;
        io.det[0] = det3; io.det[1] = det4; io.det[2] = det5; io.se = se_seg; io.lane = lane_seg; io.pc = pc_seg;
        h->eng->run(static_cast<hipStream_t>(stream));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) throw ach::AchError{ACH_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e)};
    });
}

int ach_forward_detect(ach_handle* h, const void* image, const void* radar, const void* points, void* det3, void* det4, void* det5,
                       void* se_seg, void* lane_seg, void* pc_seg, float* decoded, float conf_thres, float nms_thres, int32_t max_det,
                       float* out_rows, int32_t* out_idx, int32_t* out_count, void* workspace, void* stream) {
    return guarded(h, [&] {
        if (h->eng->ops.empty()) throw ach::AchError{ACH_ERR_INVALID, "ach_plan must precede ach_forward_detect"};
        if (!image || !radar || !det3 || !det4 || !det5 || !se_seg || !lane_seg || (h->eng->cfg.pc_seg != ACH_PCSEG_NONE && (!points || !pc_seg)))
            throw ach::AchError{ACH_ERR_INVALID, "null input/output pointer"};
        if (max_det <= 0 || !decoded || !out_rows || !out_idx || !out_count || !workspace)
            throw ach::AchError{ACH_ERR_INVALID, "bad detect arguments"};
        ach::IoPtrs& io = h->eng->io;
        io.image = image; io.radar = radar; io.points = points;
        io.det[0] = det3; io.det[1] = det4; io.det[2] = det5; io.se = se_seg; io.lane = lane_seg; io.pc = pc_seg;
        ach::EngineBase* e = h->eng;
        const int B = e->batch;
        e->detect_tail = [=](hipStream_t st) {
            e->decode(B, det3, det4, det5, decoded, st);
            e->nms(B, decoded, conf_thres, nms_thres, max_det, out_rows, out_idx, out_count, workspace, st);
        };
        struct Clear { ach::EngineBase* e; ~Clear() { e->detect_tail = nullptr; } } clear{e};
        e->run_eager(static_cast<hipStream_t>(stream));          // the tail carries per-call arguments: never replayed from a graph
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) throw ach::AchError{ACH_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(err)};
    });
}

int ach_join(ach_handle* h, void* stream) { return guarded(h, [&] { h->eng->join(static_cast<hipStream_t>(stream)); }); }
int ach_forwards_in_flight(const ach_handle* h) { return (h && h->eng) ? int(h->eng->forwards_in_flight()) : 0; }

int ach_decode(ach_handle* h, int32_t batch, const void* det3, const void* det4, const void* det5, float* decoded, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || !det3 || !det4 || !det5 || !decoded) throw ach::AchError{ACH_ERR_INVALID, "bad decode arguments"};
        h->eng->decode(batch, det3, det4, det5, decoded, static_cast<hipStream_t>(stream));
    });
}

size_t ach_nms_workspace_bytes(const ach_handle* h, int32_t batch) { return (h && h->eng) ? h->eng->nms_workspace_bytes(batch) : 0; }

int ach_nms(ach_handle* h, int32_t batch, const float* decoded, float conf_thres, float nms_thres, int32_t max_det,
            float* out_rows, int32_t* out_idx, int32_t* out_count, void* workspace, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || max_det <= 0 || !decoded || !out_rows || !out_idx || !out_count || !workspace)
            throw ach::AchError{ACH_ERR_INVALID, "bad nms arguments"};
        h->eng->nms(batch, decoded, conf_thres, nms_thres, max_det, out_rows, out_idx, out_count, workspace, static_cast<hipStream_t>(stream));
    });
}

int ach_preprocess_radar(ach_handle* h, int32_t batch, int32_t channels, const float* in, void* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || channels <= 0 || !in || !out) throw ach::AchError{ACH_ERR_INVALID, "bad preprocess_radar arguments"};
        h->eng->preprocess_radar(batch, channels, in, out, static_cast<hipStream_t>(stream));
    });
}
int ach_normalize_points(ach_handle* h, int32_t batch, int32_t n, int32_t d, const float* in, void* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || n <= 0 || d <= 0 || !in || !out) throw ach::AchError{ACH_ERR_INVALID, "bad normalize_points arguments"};
        h->eng->normalize_points(batch, n, d, in, out, static_cast<hipStream_t>(stream));
    });
}
int ach_preprocess_image(ach_handle* h, int32_t batch, const uint8_t* in, void* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || !in || !out) throw ach::AchError{ACH_ERR_INVALID, "bad preprocess_image arguments"};
        h->eng->preprocess_image(batch, in, out, static_cast<hipStream_t>(stream));
    });
}
int ach_seg_argmax(ach_handle* h, int32_t batch, int32_t channels, const void* seg, uint8_t* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || channels <= 0 || channels > 255 || !seg || !out) throw ach::AchError{ACH_ERR_INVALID, "bad seg_argmax arguments"};
        h->eng->seg_argmax(batch, channels, seg, out, static_cast<hipStream_t>(stream));
    });
}

int ach_seg_resize_argmax(ach_handle* h, int32_t batch, int32_t channels, const void* seg, int32_t out_h, int32_t out_w, float* prob_workspace,
                          uint8_t* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || channels <= 0 || channels > 255 || out_h <= 0 || out_w <= 0 || !seg || !prob_workspace || !out)
            throw ach::AchError{ACH_ERR_INVALID, "bad seg_resize_argmax arguments"};
        h->eng->seg_resize_argmax(batch, channels, seg, out_h, out_w, prob_workspace, out, static_cast<hipStream_t>(stream));
    });
}
int ach_correct_boxes(ach_handle* h, int32_t batch, int32_t max_det, const float* rows, const int32_t* count, int32_t image_h, int32_t image_w,
                      int32_t letterbox, float* out_rows, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || max_det <= 0 || image_h <= 0 || image_w <= 0 || !rows || !count || !out_rows) throw ach::AchError{ACH_ERR_INVALID, "bad correct_boxes arguments"};
        h->eng->correct_boxes(batch, max_det, rows, count, image_h, image_w, letterbox, out_rows, static_cast<hipStream_t>(stream));
    });
}

// ---- multi-GPU: the one exchange step of the path — an all-gather of the shards' fixed-size detection records over RCCL.
// RCCL is resolved at first use (dlopen of librccl.so; ACH_RCCL_LIBRARY overrides the name): the library itself does not link against it, so a
// single-GPU consumer needs no RCCL at all.  `comm` is an ncclComm_t the caller created with RCCL's own API (one rank per GPU).
#if !defined(ACH_HOSTEMU)
#include <dlfcn.h>
#endif
size_t ach_record_words(int32_t batch, int32_t max_det) { return (batch > 0 && max_det > 0) ? size_t(batch) * (size_t(max_det) * 8 + 1) : 0; }
int ach_all_gather_records(ach_handle* h, void* comm, const int32_t* send_record, int32_t* recv_records, int32_t batch, int32_t max_det, void* stream) {
    return guarded(h, [&] {
        if (!comm || !send_record || !recv_records || batch <= 0 || max_det <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad all-gather arguments"};
#if defined(ACH_HOSTEMU)
        throw ach::AchError{ACH_ERR_UNSUPPORTED, "the CPU emulation has no RCCL"};
#else
        typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
        static allgather_fn fn = nullptr;
        if (!fn) {
            const char* name = std::getenv("ACH_RCCL_LIBRARY");
            void* lib = dlopen(name ? name : "librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (!lib && !name) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!lib) throw ach::AchError{ACH_ERR_DEVICE, std::string("RCCL library not found: ") + dlerror()};
            fn = reinterpret_cast<allgather_fn>(dlsym(lib, "ncclAllGather"));
            if (!fn) throw ach::AchError{ACH_ERR_DEVICE, "ncclAllGather not found in the RCCL library"};
        }
        const int rc = fn(send_record, recv_records, ach_record_words(batch, max_det), /* ncclInt32 */ 2, comm, static_cast<hipStream_t>(stream));
        if (rc != 0) throw ach::AchError{ACH_ERR_DEVICE, "ncclAllGather failed with code " + std::to_string(rc)};
#endif
    });
}

// ---- one pass of the 8-bit PIL resample (k_prepost.h): stateless
int ach_resample_pass_u8(const uint8_t* src, uint8_t* dst, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, int32_t h_in, int32_t w_in,
                         int32_t h_out, int32_t w_out, int32_t channels, int32_t vertical, int64_t src_pitch, int64_t dst_pitch, void* stream) {
    try {
        if (!src || !dst || !bounds || !coeffs || ksize <= 0 || h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0 || channels <= 0 ||
            (vertical ? w_out != w_in : h_out != h_in))
            throw ach::AchError{ACH_ERR_INVALID, "bad resample_pass arguments"};
        ach::ResamplePassParams p{src, dst, bounds, coeffs, ksize, h_in, w_in, h_out, w_out, channels, vertical, long(src_pitch), long(dst_pitch)};
        ACH_LAUNCH(ach::resample_pass_kernel, dim3(unsigned(ach::cdivl(long(h_out) * w_out * channels, 256))), dim3(256), static_cast<hipStream_t>(stream), p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { g_create_error = std::string("kernel launch: ") + hipGetErrorString(e); return ACH_ERR_DEVICE; }
        return ACH_OK;
    } catch (const ach::AchError& e) { g_create_error = e.msg; return e.code; }
}

// ---- training-mode kernels (k_train.h): stateless, fp32, no handle
static int train_guard(const std::function<void()>& fn) {
    try { fn(); hipError_t e = hipGetLastError(); if (e != hipSuccess) { g_create_error = std::string("kernel launch: ") + hipGetErrorString(e); return ACH_ERR_DEVICE; } return ACH_OK; }
    catch (const ach::AchError& e) { g_create_error = e.msg; return e.code; }
    catch (const std::exception& e) { g_create_error = e.what(); return ACH_ERR_INVALID; }
}
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
    return train_guard([&] {
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
        const hipStream_t st = static_cast<hipStream_t>(stream);
        const bool h16 = (precision >= 0 ? precision : g_train_gemm_precision.load(std::memory_order_relaxed)) == 1;
#define ACH_TG_LAUNCH(TM, TN) { if (h16) ACH_LAUNCH((ach::train_gemm_kernel<ach::bf16_t, TM, TN>), grid, dim3(256), st, p); else ACH_LAUNCH((ach::train_gemm_kernel<float, TM, TN>), grid, dim3(256), st, p); }
        if (tm == 32 && tn == 32) ACH_TG_LAUNCH(32, 32)
        else if (tm == 32) ACH_TG_LAUNCH(32, 64)
        else if (tn == 32) ACH_TG_LAUNCH(64, 32)
        else ACH_TG_LAUNCH(64, 64)
#undef ACH_TG_LAUNCH
        if (p.ksplit > 1) ACH_LAUNCH(ach::train_gemm_reduce_kernel, dim3(unsigned(ach::cdivl(long(M) * N, 16))), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
int ach_train_bn_stats(const float* z, float* mean, float* var, int32_t B, int32_t C, int32_t N, void* stream) {
    return train_guard([&] {
        if (!z || !mean || !var || B <= 0 || C <= 0 || N <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_stats arguments"};
        const int S = train_slices(long(B) * N, C);
        if (S > 1) {
            ach::BnSliceParams q{z, train_workspace(size_t(2) * C * S * sizeof(float)), mean, var, B, C, N, S};
            ACH_LAUNCH(ach::train_bn_slice2_kernel, dim3(unsigned(C), unsigned(S)), dim3(256), static_cast<hipStream_t>(stream), q);          // both passes of a slice, the second out of the L2
            ACH_LAUNCH(ach::train_bn_slice2_finalize_kernel, dim3(unsigned((C + 255) / 256)), dim3(256), static_cast<hipStream_t>(stream), q);
            return;
        }
        ach::BnStatsParams p{z, mean, var, B, C, N};
        ACH_LAUNCH(ach::train_bn_stats_kernel, dim3(unsigned(C)), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
int ach_train_bn_running(const float* mean, const float* var, float* running_mean, float* running_var, int32_t C, float momentum, float unbias, void* stream) {
    return train_guard([&] {
        if (!mean || !var || !running_mean || !running_var || C <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_running arguments"};
        ach::BnRunningParams p{mean, var, running_mean, running_var, C, momentum, unbias};
        ACH_LAUNCH(ach::train_bn_running_kernel, dim3(unsigned((C + 255) / 256)), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
int ach_train_bn_relu_fwd(const float* z, const float* mean, const float* var, const float* gamma, const float* beta, float* y, int32_t B, int32_t C,
                          int32_t N, float eps, int32_t relu, void* stream) {
    return train_guard([&] {
        if (!z || !mean || !var || !gamma || !beta || !y || B <= 0 || C <= 0 || N <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_relu_fwd arguments"};
        ach::BnReluFwdParams p{z, mean, var, gamma, beta, y, B, C, N, eps, relu};
        const bool quad = (N & 3) == 0 && long(B) * C <= 65535 && ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;      // a plane per blockIdx.y, four positions per thread
        if (quad) ACH_LAUNCH(ach::train_bn_relu_fwd4_kernel, dim3(unsigned(ach::cdivl(long(N) / 4, 256)), unsigned(long(B) * C)), dim3(256), static_cast<hipStream_t>(stream), p);
        else
        ACH_LAUNCH(ach::train_bn_relu_fwd_kernel, dim3(unsigned(ach::cdivl(long(B) * C * N, 256))), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
int ach_train_bn_relu_bwd(const float* z, const float* y, const float* dy, const float* mean, const float* var, const float* gamma, float* dgamma,
                          float* dbeta, float* dz, int32_t B, int32_t C, int32_t N, float eps, int32_t relu, void* stream) {
    return train_guard([&] {
        if (!z || !y || !dy || !mean || !var || !gamma || !dgamma || !dbeta || !dz || B <= 0 || C <= 0 || N <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_bn_relu_bwd arguments"};
        ach::BnReluBwdParams p{z, y, dy, mean, var, gamma, dgamma, dbeta, dz, B, C, N, eps, relu, 1, nullptr};
        p.S = train_slices(long(B) * N, C);
        if (p.S > 1) p.ws = train_workspace(size_t(2) * C * p.S * sizeof(float));
        ACH_LAUNCH(ach::train_bn_relu_bwd_reduce_kernel, dim3(unsigned(C), unsigned(p.S)), dim3(256), static_cast<hipStream_t>(stream), p);
        if (p.S > 1) ACH_LAUNCH(ach::train_bn_relu_bwd_finalize_kernel, dim3(unsigned((C + 255) / 256)), dim3(256), static_cast<hipStream_t>(stream), p);
        const bool quad = (N & 3) == 0 && long(B) * C <= 65535 &&
                          ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dz)) & 15u) == 0;
        if (quad) ACH_LAUNCH(ach::train_bn_relu_bwd_apply4_kernel, dim3(unsigned(ach::cdivl(long(N) / 4, 256)), unsigned(long(B) * C)), dim3(256), static_cast<hipStream_t>(stream), p);
        else
        ACH_LAUNCH(ach::train_bn_relu_bwd_apply_kernel, dim3(unsigned(ach::cdivl(long(B) * C * N, 256))), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}

int ach_train_dw3x3(const float* x, const float* w, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t flip, void* stream) {
    return train_guard([&] {
        if (!x || !w || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_dw3x3 arguments"};
        ach::DwTrainParams p{x, w, y, B, C, H, W, flip};
        ACH_LAUNCH(ach::train_dw3x3_kernel, dim3(unsigned(ach::cdivl(long(B) * C * H * W, 256))), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
int ach_train_dw3x3_wgrad(const float* x, const float* dz, float* dw, int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
    return train_guard([&] {
        if (!x || !dz || !dw || B <= 0 || C <= 0 || H <= 0 || W <= 0) throw ach::AchError{ACH_ERR_INVALID, "bad train_dw3x3_wgrad arguments"};
        ach::DwWgradParams p{x, dz, dw, B, C, H, W};
        ACH_LAUNCH(ach::train_dw3x3_wgrad_kernel, dim3(unsigned(C)), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}

int ach_train_max_points(const float* x, float* y, int32_t* idx, const float* dy, float* dx, int64_t rows, int32_t N, void* stream) {
    return train_guard([&] {                                 /* forward when dy == NULL, backward otherwise */
        if (rows <= 0 || N <= 0 || !idx) throw ach::AchError{ACH_ERR_INVALID, "bad train_max_points arguments"};
        if (!dy) {
            if (!x || !y) throw ach::AchError{ACH_ERR_INVALID, "bad train_max_points arguments"};
            ach::MaxPtsParams p{x, y, idx, long(rows), N};
            ACH_LAUNCH(ach::train_max_points_fwd_kernel, dim3(unsigned(ach::cdivl(long(rows), 4))), dim3(256), static_cast<hipStream_t>(stream), p);
        } else {
            if (!dx) throw ach::AchError{ACH_ERR_INVALID, "bad train_max_points arguments"};
            ach::MaxPtsBwdParams p{dy, idx, dx, long(rows), N};
            ACH_LAUNCH(ach::train_max_points_bwd_kernel, dim3(unsigned(ach::cdivl(long(rows) * N, 256))), dim3(256), static_cast<hipStream_t>(stream), p);
        }
    });
}
int ach_train_log_softmax(const float* z, float* y, const float* dy, float* dz, int32_t B, int32_t K, int32_t N, void* stream) {
    return train_guard([&] {                                 /* forward when dy == NULL (z -> y [B,N,K]); backward: y, dy -> dz [B,K,N] */
        if (B <= 0 || K <= 0 || N <= 0 || !y) throw ach::AchError{ACH_ERR_INVALID, "bad train_log_softmax arguments"};
        ach::LsmTrainParams p{z, y, dy, dz, B, K, N};
        const dim3 grid(unsigned(ach::cdivl(long(B) * N, 256)));
        if (!dy) { if (!z) throw ach::AchError{ACH_ERR_INVALID, "bad train_log_softmax arguments"}; ACH_LAUNCH(ach::train_log_softmax_fwd_kernel, grid, dim3(256), static_cast<hipStream_t>(stream), p); }
        else { if (!dz) throw ach::AchError{ACH_ERR_INVALID, "bad train_log_softmax arguments"}; ACH_LAUNCH(ach::train_log_softmax_bwd_kernel, grid, dim3(256), static_cast<hipStream_t>(stream), p); }
    });
}

// ---- training-mode primitives of k_train2.h
#define ACH_TRAIN_1D(kern, p, total) ACH_LAUNCH(kern, dim3(unsigned(ach::cdivl((total), 256))), dim3(256), static_cast<hipStream_t>(stream), p)
#define ACH_TRAIN_ROWS(kern, p, nblocks) ACH_LAUNCH(kern, dim3(unsigned(nblocks)), dim3(256), static_cast<hipStream_t>(stream), p)
static void train_need(bool ok, const char* what) { if (!ok) throw ach::AchError{ACH_ERR_INVALID, std::string("bad arguments: ") + what}; }
int ach_train_act(const float* x, const float* dy, float* out, int64_t n, int32_t kind, void* stream) {
    return train_guard([&] {
        train_need(x && out && n > 0 && kind >= 0 && kind <= 3, "ach_train_act");
        ach::TrainActParams p{x, dy, out, long(n), kind};
        const bool quad = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
        if (quad) ACH_TRAIN_1D(ach::train_act4_kernel, p, long(n) / 4);
        else ACH_TRAIN_1D(ach::train_act_kernel, p, long(n));
    });
}
int ach_train_mul(const float* a, const float* b, float* out, int64_t n, void* stream) {
    return train_guard([&] {
        train_need(a && b && out && n > 0, "ach_train_mul");
        ach::TrainMulParams p{a, b, out, long(n)};
        ACH_TRAIN_1D(ach::train_mul_kernel, p, long(n));
    });
}
int ach_train_layernorm(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows, int32_t C, int64_t inner,
                        float eps, void* stream) {
    return train_guard([&] {
        train_need(x && gamma && beta && y && mean && rstd && rows > 0 && C > 0 && inner > 0, "ach_train_layernorm");
        ach::TrainLnParams p{x, gamma, beta, y, mean, rstd, long(rows), C, long(inner), eps};
        const bool quad = (inner & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(rstd)) & 15u) == 0;
        if (quad) ACH_TRAIN_1D(ach::train_ln_fwd4_kernel, p, long(rows) * (inner / 4));
        else ACH_TRAIN_1D(ach::train_ln_fwd_kernel, p, long(rows) * inner);
    });
}
int ach_train_layernorm_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                            int64_t rows, int32_t C, int64_t inner, void* stream) {
    return train_guard([&] {
        train_need(x && dy && gamma && mean && rstd && dx && dgamma && dbeta && rows > 0 && C > 0 && inner > 0, "ach_train_layernorm_bwd");
        ach::TrainLnBwdParams p{x, dy, gamma, mean, rstd, dx, dgamma, dbeta, long(rows), C, long(inner), 1, nullptr};
        const bool quad = (inner & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(rstd)) & 15u) == 0;
        if (quad) ACH_TRAIN_1D(ach::train_ln_bwd_dx4_kernel, p, long(rows) * (inner / 4));
        else ACH_TRAIN_1D(ach::train_ln_bwd_dx_kernel, p, long(rows) * inner);
        p.S = train_slices(long(rows) * inner, C);
        if (p.S > 1) p.ws = train_workspace(size_t(2) * C * p.S * sizeof(float));
        ACH_LAUNCH(ach::train_ln_bwd_param_kernel, dim3(unsigned(C), unsigned(p.S)), dim3(256), static_cast<hipStream_t>(stream), p);
        if (p.S > 1) ACH_LAUNCH(ach::train_ln_bwd_param_finalize_kernel, dim3(unsigned((C + 255) / 256)), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
int ach_train_dwconv(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, int32_t flip, void* stream) {
    return train_guard([&] {
        train_need(x && w && y && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && (k & 1), "ach_train_dwconv");
        ach::TrainDwParams p{x, w, bias, y, B, C, H, W, k, flip};
        const bool quad = (W & 3) == 0 && long(B) * C <= 65535 && (reinterpret_cast<uintptr_t>(y) & 15u) == 0;      // four outputs of a row per thread (k_train2.h)
        const dim3 gq(unsigned(ach::cdivl(long(H) * (W / 4), 256)), unsigned(long(B) * C)), bq(256);
        const hipStream_t st = static_cast<hipStream_t>(stream);
        if (quad && k == 3) ACH_LAUNCH(ach::train_dwconv4_kernel<3>, gq, bq, st, p);
        else if (quad && k == 5) ACH_LAUNCH(ach::train_dwconv4_kernel<5>, gq, bq, st, p);
        else if (quad && k == 7) ACH_LAUNCH(ach::train_dwconv4_kernel<7>, gq, bq, st, p);
        else if (quad && k == 9) ACH_LAUNCH(ach::train_dwconv4_kernel<9>, gq, bq, st, p);
        else
        if (k == 3) ACH_TRAIN_1D(ach::train_dwconv_kernel<3>, p, long(B) * C * H * W);
        else if (k == 5) ACH_TRAIN_1D(ach::train_dwconv_kernel<5>, p, long(B) * C * H * W);
        else if (k == 7) ACH_TRAIN_1D(ach::train_dwconv_kernel<7>, p, long(B) * C * H * W);
        else if (k == 9) ACH_TRAIN_1D(ach::train_dwconv_kernel<9>, p, long(B) * C * H * W);
        else ACH_TRAIN_1D(ach::train_dwconv_kernel<0>, p, long(B) * C * H * W);
    });
}
int ach_train_dwconv_wgrad(const float* x, const float* dz, float* dw, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, void* stream) {
    return train_guard([&] {
        train_need(x && dz && dw && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && (k & 1), "ach_train_dwconv_wgrad");
        ach::TrainDwWgradParams p{x, dz, dw, B, C, H, W, k, 1, nullptr};
        const bool taps = (k == 3 || k == 5 || k == 7 || k == 9) && long(B) * H * W < (1L << 31);      // all taps of a channel in one pass (k_train2.h)
        p.S = train_slices(long(B) * H * W, taps ? C : C * k * k);
        if (p.S > 1) p.ws = train_workspace(size_t(C) * k * k * p.S * sizeof(float));
        const hipStream_t st = static_cast<hipStream_t>(stream);
        const dim3 gt(unsigned(C), unsigned(p.S));
        if (taps && k == 3) ACH_LAUNCH(ach::train_dwconv_wgrad_taps_kernel<3>, gt, dim3(256), st, p);
        else if (taps && k == 5) ACH_LAUNCH(ach::train_dwconv_wgrad_taps_kernel<5>, gt, dim3(256), st, p);
        else if (taps && k == 7) ACH_LAUNCH(ach::train_dwconv_wgrad_taps_kernel<7>, gt, dim3(256), st, p);
        else if (taps) ACH_LAUNCH(ach::train_dwconv_wgrad_taps_kernel<9>, gt, dim3(256), st, p);
        else
        ACH_LAUNCH(ach::train_dwconv_wgrad_kernel, dim3(unsigned(C * k * k), unsigned(p.S)), dim3(256), static_cast<hipStream_t>(stream), p);
        if (p.S > 1) ACH_LAUNCH(ach::train_dwconv_wgrad_finalize_kernel, dim3(unsigned((C * k * k + 255) / 256)), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
int ach_train_im2col(const float* src, float* dst, int32_t B, int32_t C, int32_t H, int32_t W, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                     int32_t Ho, int32_t Wo, int32_t backward, void* stream) {
    return train_guard([&] {
        train_need(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && Ho > 0 && Wo > 0, "ach_train_im2col");
        ach::TrainColParams p{src, dst, B, C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo};
        if (!backward) ACH_TRAIN_1D(ach::train_im2col_kernel, p, long(B) * C * kh * kw * Ho * Wo);
        else ACH_TRAIN_1D(ach::train_col2im_kernel, p, long(B) * C * H * W);
    });
}
int ach_train_softmax(const float* x, float* y, const float* dy, float* dx, int64_t rows, int32_t d, void* stream) {
    return train_guard([&] {
        train_need(y && rows > 0 && d > 0 && (dy ? dx != nullptr : x != nullptr), "ach_train_softmax");
        ach::TrainSoftmaxParams p{x, y, dy, dx, long(rows), d};
        ACH_TRAIN_1D(ach::train_softmax_kernel, p, long(rows));
    });
}
int ach_train_upsample2x(const float* src, float* dst, int64_t planes, int32_t h, int32_t w, int32_t backward, void* stream) {
    return train_guard([&] {
        train_need(src && dst && planes > 0 && h > 0 && w > 0, "ach_train_upsample2x");
        ach::TrainUpParams p{src, dst, long(planes), h, w, h > 1 ? float(h - 1) / float(2 * h - 1) : 0.f, w > 1 ? float(w - 1) / float(2 * w - 1) : 0.f};
        if (!backward) ACH_TRAIN_1D(ach::train_up2_fwd_kernel, p, long(planes) * 4 * h * w);
        else ACH_TRAIN_1D(ach::train_up2_bwd_kernel, p, long(planes) * h * w);
    });
}
int ach_train_maxpool(const float* x, float* y, int32_t* idx, const float* dy, float* dx, int64_t planes, int32_t H, int32_t W, int32_t k, void* stream) {
    return train_guard([&] {
        train_need(idx && planes > 0 && H > 0 && W > 0 && k > 0 && (k & 1) && (dy ? dx != nullptr : (x && y)), "ach_train_maxpool");
        ach::TrainPoolParams p{x, y, idx, dy, dx, long(planes), H, W, k};
        ACH_TRAIN_1D(ach::train_maxpool_kernel, p, long(planes) * H * W);
    });
}
int ach_train_avgpool3(const float* x, float* y, int64_t planes, int32_t H, int32_t W, void* stream) {
    return train_guard([&] {
        train_need(x && y && planes > 0 && H > 0 && W > 0, "ach_train_avgpool3");
        ach::TrainPoolParams p{x, y, nullptr, nullptr, nullptr, long(planes), H, W, 3};
        ACH_TRAIN_1D(ach::train_avgpool3_kernel, p, long(planes) * H * W);
    });
}
int ach_train_row_reduce(const float* a, const float* b, float* out, int64_t rows, int64_t n, float scale, void* stream) {
    return train_guard([&] {
        train_need(a && out && rows > 0 && n > 0, "ach_train_row_reduce");
        ach::TrainRowParams p{a, b, out, long(rows), long(n), 1, scale};
        ACH_TRAIN_ROWS(ach::train_row_reduce_kernel, p, rows);
    });
}
int ach_train_row_scale(const float* x, const float* s, float* out, int64_t rows, int64_t n, int64_t period, void* stream) {
    return train_guard([&] {
        train_need(s && out && rows > 0 && n > 0 && period > 0, "ach_train_row_scale");
        ach::TrainRowParams p{x, s, out, long(rows), long(n), long(period), 1.f};
        ACH_TRAIN_1D(ach::train_row_scale_kernel, p, long(rows) * n);
    });
}
int ach_train_col_reduce(const float* a, const float* b, float* out, int64_t rows, int64_t cols, float scale, void* stream) {
    return train_guard([&] {
        train_need(a && out && rows > 0 && cols > 0, "ach_train_col_reduce");
        ach::TrainRowParams p{a, b, out, long(rows), long(cols), 1, scale};
        ACH_TRAIN_ROWS(ach::train_col_reduce_kernel, p, cols);
    });
}
int ach_train_col_scale(const float* x, const float* g, float* out, int64_t rows, int64_t cols, void* stream) {
    return train_guard([&] {
        train_need(x && g && out && rows > 0 && cols > 0, "ach_train_col_scale");
        ach::TrainRowParams p{x, g, out, long(rows), long(cols), 1, 1.f};
        ACH_TRAIN_1D(ach::train_col_scale_kernel, p, long(rows) * cols);
    });
}
int ach_train_instnorm(const float* x, const float* dy, const float* gamma, const float* beta, float* y, float* mean, float* rstd, float* dx, float* dgamma_rows,
                       float* dbeta_rows, int64_t rows, int64_t n, int32_t C, float eps, void* stream) {
    return train_guard([&] {
        train_need(x && gamma && mean && rstd && rows > 0 && n > 0 && C > 0 && (dy ? (dx && dgamma_rows && dbeta_rows) : (y && beta)), "ach_train_instnorm");
        ach::TrainInParams p{x, dy, gamma, beta, y, mean, rstd, dx, dgamma_rows, dbeta_rows, long(rows), long(n), C, eps};
        ACH_TRAIN_ROWS(ach::train_instnorm_kernel, p, rows);
    });
}
int ach_train_l2norm(const float* x, float* y, float* norm, const float* dy, float* dx, int64_t rows, int64_t n, float eps, void* stream) {
    return train_guard([&] {
        train_need(x && norm && rows > 0 && n > 0 && (dy ? dx != nullptr : y != nullptr), "ach_train_l2norm");
        ach::TrainL2Params p{x, y, norm, dy, dx, long(rows), long(n), eps};
        ACH_TRAIN_ROWS(ach::train_l2norm_kernel, p, rows);
    });
}
int ach_train_deform_im2col(const float* x, const float* offset, const float* mask, float* col, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                            int32_t stride, int32_t pad, void* stream) {
    return train_guard([&] {
        train_need(x && offset && mask && col && B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && stride > 0, "ach_train_deform_im2col");
        ach::TrainDeformParams p{x, offset, mask, col, nullptr, nullptr, nullptr, nullptr, B, C, H, W, Ho, Wo, stride, pad};
        ACH_TRAIN_1D(ach::train_deform_im2col_kernel, p, long(B) * C * 9 * Ho * Wo);
    });
}
int ach_train_deform_bwd(const float* x, const float* offset, const float* mask, const float* dcol, float* dx_zeroed, float* doffset, float* dmask, int32_t B,
                         int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t stride, int32_t pad, void* stream) {
    return train_guard([&] {
        train_need(x && offset && mask && dcol && doffset && dmask && B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && stride > 0, "ach_train_deform_bwd");
        ach::TrainDeformParams p{x, offset, mask, nullptr, dcol, dx_zeroed, doffset, dmask, B, C, H, W, Ho, Wo, stride, pad};
        ACH_TRAIN_1D(ach::train_deform_bwd_coord_kernel, p, long(B) * 9 * Ho * Wo);
        // (dx_zeroed = NULL: the input needs no gradient — the first RCBlock reads the pooled radar map.  An LDS-combining form of this scatter — a workgroup per 16 x 16 tile of
        //  positions, LDS atomics, one L2 atomic per touched input pixel instead of 36 per position — was measured 4x SLOWER end to end (batch-32 step 64.5 -> 86.7 ms) and is not kept.)
        if (dx_zeroed) ACH_TRAIN_1D(ach::train_deform_bwd_input_kernel, p, long(B) * C * 9 * Ho * Wo);
    });
}
// ---- PointNet++ in training mode (k_train3.h): the inference engine's geometry kernels at fp32 + the two scatter-form adjoints
int ach_train_pn2_fps(const float* xyz, int32_t B, int32_t n, int32_t npoint, int32_t* idx, float* new_xyz, void* stream) {
    return train_guard([&] {
        train_need(xyz && idx && new_xyz && B > 0 && n > 0 && npoint > 0 && npoint <= n && n <= 64 * ach::PN2_FPS_MAX_PPT, "ach_train_pn2_fps");
        ach::launch_pn2_fps(ach::FpsParams{xyz, n, npoint, idx, new_xyz}, B, static_cast<hipStream_t>(stream));
    });
}
int ach_train_pn2_group(const float* xyz, const float* new_xyz, const float* feats, int32_t C, int32_t B, int32_t n, int32_t S, int32_t nsample, float radius2,
                        float* grouped, int32_t* group_idx, void* stream) {
    return train_guard([&] {
        train_need(xyz && new_xyz && (feats || C == 0) && grouped && group_idx && C >= 0 && B > 0 && n > 0 && S > 0 && nsample > 0 && nsample <= ach::PN2_MAX_NSAMPLE, "ach_train_pn2_group");
        ach::GroupParams q{xyz, new_xyz, feats, long(C), C, grouped, long(3 + C), group_idx, B, n, S, nsample, radius2, 1};
        ACH_LAUNCH(ach::pn2_group_kernel<float>, dim3(unsigned(ach::cdivl(long(B) * S, 4))), dim3(256), static_cast<hipStream_t>(stream), q);
    });
}
int ach_train_pn2_group_bwd(const int32_t* group_idx, const float* dgrouped, float* dfeats_zeroed, int32_t C, int32_t B, int32_t n, int32_t S, int32_t nsample, void* stream) {
    return train_guard([&] {
        train_need(group_idx && dgrouped && dfeats_zeroed && C > 0 && B > 0 && n > 0 && S > 0 && nsample > 0, "ach_train_pn2_group_bwd");
        ach::Pn2GroupBwdParams q{group_idx, dgrouped, long(3 + C), dfeats_zeroed, C, B, n, S, nsample};
        ACH_TRAIN_1D(ach::train_pn2_group_bwd_kernel, q, long(B) * S * nsample * C);
    });
}
int ach_train_pn2_interp(const float* xyz1, const float* xyz2, const float* skip, int32_t C1, const float* sparse, int32_t C2, float* out, float* dskip, float* dsparse_zeroed,
                         const float* dout, int32_t B, int32_t n, int32_t s, void* stream) {
    return train_guard([&] {
        train_need(xyz1 && xyz2 && C1 >= 0 && C2 > 0 && B > 0 && n > 0 && s >= 3 && s <= 64 * ach::PN2_INTERP_SPL, "ach_train_pn2_interp");
        const dim3 grid(unsigned(ach::cdivl(long(B) * n, 4))), block(256);
        if (!dout) {
            train_need((skip || C1 == 0) && sparse && out, "ach_train_pn2_interp (forward)");
            ach::InterpParams q{xyz1, xyz2, skip, long(C1), C1, sparse, long(C2), C2, out, long(C1 + C2), B, n, s};
            ACH_LAUNCH(ach::pn2_interp_kernel<float>, grid, block, static_cast<hipStream_t>(stream), q);
        } else {
            train_need((dskip || C1 == 0) && dsparse_zeroed, "ach_train_pn2_interp (backward)");
            ach::InterpParams q{xyz1, xyz2, nullptr, long(C1), C1, nullptr, long(C2), C2, nullptr, long(C1 + C2), B, n, s};
            ACH_LAUNCH(ach::train_pn2_interp_bwd_kernel, grid, block, static_cast<hipStream_t>(stream), q, dout, dskip, dsparse_zeroed);
        }
    });
}
#undef ACH_TRAIN_1D
#undef ACH_TRAIN_ROWS

int ach_tap_count(const ach_handle* h) { return (h && h->eng) ? int(h->eng->tap_order.size()) : 0; }
const char* ach_tap_name(const ach_handle* h, int i) {
    if (!h || !h->eng || i < 0 || i >= int(h->eng->tap_order.size())) return nullptr;
    return h->eng->tap_order[size_t(i)].c_str();
}
int ach_tap_shape(const ach_handle* hc, const char* name, int64_t shape[4], int32_t* ndim) {
    ach_handle* h = const_cast<ach_handle*>(hc);
    return guarded(h, [&] {
        if (!name || !shape || !ndim) throw ach::AchError{ACH_ERR_INVALID, "bad tap arguments"};
        std::vector<long> s = h->eng->tap_shape(name);
        *ndim = int32_t(s.size());
        for (size_t i = 0; i < s.size() && i < 4; ++i) shape[i] = s[i];
    });
}
int ach_read_tap(ach_handle* h, const char* name, float* host_out, size_t capacity_elems) {
    return guarded(h, [&] {
        if (!name || !host_out) throw ach::AchError{ACH_ERR_INVALID, "bad tap arguments"};
        h->eng->read_tap(name, host_out, capacity_elems);
    });
}
int ach_count_saturated(ach_handle* h, void* stream, uint64_t* count) {
    return guarded(h, [&] {
        if (!count) throw ach::AchError{ACH_ERR_INVALID, "null count"};
        *count = uint64_t(h->eng->count_saturated(static_cast<hipStream_t>(stream)));
    });
}
int ach_plan_launches(const ach_handle* h) { return (h && h->eng) ? int(h->eng->ops.size()) : 0; }
const char* ach_op_name(const ach_handle* h, int i) {
    if (!h || !h->eng || i < 0 || i >= int(h->eng->ops.size())) return nullptr;
    return h->eng->ops[size_t(i)].name.c_str();
}
double ach_op_bytes(const ach_handle* h, int i) {
    if (!h || !h->eng || i < 0 || i >= int(h->eng->ops.size())) return 0;
    return h->eng->ops[size_t(i)].bytes;
}
double ach_op_layout_bytes(const ach_handle* h, int i) {
    if (!h || !h->eng || i < 0 || i >= int(h->eng->ops.size())) return 0;
    return h->eng->ops[size_t(i)].layout_bytes;
}
int ach_op_stream(const ach_handle* h, int i) {
    if (!h || !h->eng || i < 0 || i >= int(h->eng->ops.size())) return -1;
    return h->eng->ops[size_t(i)].stream;
}
double ach_op_flops(const ach_handle* h, int i) {
    if (!h || !h->eng || i < 0 || i >= int(h->eng->ops.size())) return 0;
    return h->eng->ops[size_t(i)].flops;
}
int ach_forward_profiled(ach_handle* h, const void* image, const void* radar, const void* points, void* det3, void* det4,
                         void* det5, void* se_seg, void* lane_seg, void* pc_seg, void* stream, float* op_ms, size_t capacity) {
    return guarded(h, [&] {
        if (h->eng->ops.empty()) throw ach::AchError{ACH_ERR_INVALID, "ach_plan must precede ach_forward"};
        if (!image || !radar || !det3 || !det4 || !det5 || !se_seg || !lane_seg || !op_ms || (h->eng->cfg.pc_seg != ACH_PCSEG_NONE && (!points || !pc_seg)))
            throw ach::AchError{ACH_ERR_INVALID, "null pointer"};
        ach::IoPtrs& io = h->eng->io;
        io.image = image; io.radar = radar; io.points = points;
        io.det[0] = det3; io.det[1] = det4; io.det[2] = det5; io.se = se_seg; io.lane = lane_seg; io.pc = pc_seg;
        h->eng->run_profiled(static_cast<hipStream_t>(stream), op_ms, capacity);
    });
}
int ach_bench_gemm(ach_handle* h, int M, int K, int N, int act, int ln, int residual, int P, int iters, void* stream, float* ms) {
    return guarded(h, [&] {
        if (M <= 0 || K <= 0 || N <= 0 || iters <= 0 || !ms) throw ach::AchError{ACH_ERR_INVALID, "bad bench arguments"};
        *ms = h->eng->bench_gemm(M, K, N, act, ln, residual, P, iters, static_cast<hipStream_t>(stream));
    });
}
int ach_set_probe(ach_handle* h, int op_index) { return guarded(h, [&] { h->eng->set_probe(op_index); }); }
int ach_set_probe_range(ach_handle* h, int slot, int first, int last) { return guarded(h, [&] { h->eng->set_probe_range(slot, first, last); }); }
int ach_read_probe_slot(ach_handle* h, int slot, float* avg_ms, int* samples) {
    return guarded(h, [&] {
        if (!avg_ms || !samples) throw ach::AchError{ACH_ERR_INVALID, "null probe outputs"};
        h->eng->read_probe_slot(slot, avg_ms, samples);
    });
}
int ach_read_probe(ach_handle* h, float* avg_ms, int* samples) {
    return guarded(h, [&] {
        if (!avg_ms || !samples) throw ach::AchError{ACH_ERR_INVALID, "null pointer"};
        h->eng->read_probe(avg_ms, samples);
    });
}

// ---- training losses (k_loss.h): stateless, fp32, no host read — capturable.  Workspaces are the caller's.
int ach_train_yolo_loss(const float* raw0, const float* raw1, const float* raw2, const float* boxes, const int32_t* counts, int32_t B, int32_t C, int32_t G,
                        int32_t H0, int32_t W0, int32_t H1, int32_t W1, int32_t H2, int32_t W2, float s0, float s1, float s2, int32_t* claim_anchor, float* claim_cost,
                        float* claim_iou, int32_t* matched, float* pred_iou, int32_t* num_fg, float* grad, float* partial, float* loss, void* stream) {
    return train_guard([&] {
        train_need(raw0 && raw1 && raw2 && boxes && counts && claim_anchor && claim_cost && claim_iou && matched && pred_iou && num_fg && grad && partial && loss, "ach_train_yolo_loss");
        train_need(B > 0 && B <= 65535 && C > 0 && G > 0 && G <= ach::YL_MAXG && H0 > 0 && W0 > 0 && H1 > 0 && W1 > 0 && H2 > 0 && W2 > 0, "ach_train_yolo_loss");
        const long n0 = long(H0) * W0, n1 = long(H1) * W1, n2 = long(H2) * W2, A = n0 + n1 + n2;
        train_need(A <= ach::YL_MAXA, "ach_train_yolo_loss: more anchors than the assignment holds (inputs up to 512 x 512)");
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
        hipStream_t s = static_cast<hipStream_t>(stream);
        ACH_LAUNCH(ach::yolo_assign_kernel, dim3(unsigned(G), unsigned(B)), dim3(256), s, p);
        ACH_LAUNCH(ach::yolo_resolve_kernel, dim3(unsigned(B)), dim3(256), s, p);
        ACH_LAUNCH(ach::yolo_loss_kernel, dim3(ablocks, unsigned(B)), dim3(256), s, p);
        ACH_LAUNCH(ach::yolo_reduce_kernel, dim3(1), dim3(256), s, p);
    });
}
int ach_train_loss_scale(const float* g, const float* scale, float* out, int64_t n, void* stream) {
    return train_guard([&] {
        train_need(g && scale && out && n > 0, "ach_train_loss_scale");
        ach::LossScaleParams p{g, scale, out, long(n)};
        ACH_LAUNCH(ach::loss_scale_kernel, dim3(unsigned(ach::cdivl(long(n), 256))), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}
// workgroups of the segmentation-loss kernels: 256 threads x V pixels each, grid-stride above 768 = three resident workgroups on each of the 256 compute units
// (measured at batch 32, 9 classes: 0.180 ms forward + backward against 0.192 with 1024 and 0.204 with 512; the caller's `partial` holds 1024 rows)
static int seg_loss_blocks(long items) { return int(std::max<long>(1, std::min<long>(ach::cdivl(items, 256), 768))); }
int ach_train_seg_loss(const float* logits, const void* labels, int32_t label_kind, const float* weights, int32_t B, int32_t C, int64_t HW, int32_t mode, int32_t dice,
                       float alpha, float gamma, float beta, float smooth, float* partial, float* stats, const float* cot, float* dlogits, void* stream) {
    return train_guard([&] {                                 /* forward when cot == NULL (-> stats), backward otherwise (stats, cot -> dlogits) */
        train_need(logits && labels && partial && stats && B > 0 && C > 0 && C <= ach::SEG_MAXC && HW > 0 && label_kind >= 0 && label_kind <= 2 && mode >= 0 && mode <= 2,
                   "ach_train_seg_loss");
        train_need(mode == 2 || weights != nullptr, "ach_train_seg_loss: class weights");
        train_need(cot ? dlogits != nullptr : true, "ach_train_seg_loss");
        ach::SegLossParams p{logits, labels, label_kind, weights, B, C, long(HW), mode, dice, alpha, gamma, beta, smooth, partial, 0, stats, cot, dlogits};
        const bool quad = (HW & 3) == 0 && ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits)) & 15u) == 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        p.nblk = seg_loss_blocks(long(B) * (quad ? HW / 4 : HW));
        if (quad) ach::seg_loss_launch<4>(p, cot != nullptr, s); else ach::seg_loss_launch<1>(p, cot != nullptr, s);
        if (!cot) ACH_LAUNCH(ach::seg_reduce_kernel, dim3(1), dim3(256), s, p);
    });
}

// ---- validation metrics (k_metrics.h): stateless, no host read, no synchronisation — one launch each.  Every buffer is the caller's.
int ach_eval_confusion(const void* pred, int32_t pred_kind, int32_t layout, const void* labels, int32_t label_kind, int32_t B, int32_t n, int64_t HW, uint64_t* hist,
                       void* stream) {
    return train_guard([&] {
        train_need(pred && labels && hist && B > 0 && HW > 0 && pred_kind >= 0 && pred_kind <= 3 && (layout == 0 || layout == 1) && label_kind >= 0 && label_kind <= 2,
                   "ach_eval_confusion");
        train_need(n >= 1 && n <= ach::CONF_MAXN, "ach_eval_confusion: 1 <= n <= 16 classes");
        ach::ConfusionParams p{pred, layout, labels, label_kind, B, n, long(HW), reinterpret_cast<unsigned long long*>(hist)};
        const int V = ach::conf_vec(pred_kind);
        const bool vec = (pred_kind == ach::CONF_MAP_U8 || layout == 0) && HW % V == 0 &&
                         ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
        const long items = long(B) * (vec ? HW / V : HW);
        const int nblk = int(std::max<long>(1, std::min<long>(ach::cdivl(items, 256), ach::CONF_BLOCKS)));
        train_need(ach::cdivl(long(B) * HW, nblk) < (1L << 31), "ach_eval_confusion: too many pixels for one call (the per-workgroup bins are 32-bit)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (pred_kind == ach::CONF_F32) ach::confusion_launch<float>(p, vec, nblk, s);
        else if (pred_kind == ach::CONF_BF16) ach::confusion_launch<ach::bf16_t>(p, vec, nblk, s);
        else if (pred_kind == ach::CONF_F16) ach::confusion_launch<ach::f16_t>(p, vec, nblk, s);
        else ach::confusion_launch<ach::conf_u8>(p, vec, nblk, s);
    });
}
int ach_eval_match(const float* rows, const int32_t* counts, int32_t yx_order, int32_t truncate, const float* gt, const uint8_t* difficult, const int32_t* gt_counts,
                   int32_t B, int32_t max_det, int32_t G, int32_t C, const double* thresholds, int32_t T, uint8_t* flags, int32_t* match, double* iou, float* score,
                   uint64_t* gt_per_class, void* stream) {
    return train_guard([&] {
        train_need(rows && counts && gt && gt_counts && thresholds && flags && match && iou && score && gt_per_class, "ach_eval_match");
        train_need(B > 0 && max_det > 0 && max_det <= ach::MATCH_MAXD && G > 0 && G <= ach::MATCH_MAXG && C > 0 && T > 0 && T <= ach::MATCH_MAXT,
                   "ach_eval_match: max_det <= 1024, G <= 128, T <= 10");
        ach::MatchParams p{};
        p.rows = rows; p.counts = counts; p.yx_order = yx_order != 0; p.truncate = truncate != 0;
        p.gt = gt; p.difficult = difficult; p.gt_counts = gt_counts;
        p.B = B; p.D = max_det; p.G = G; p.C = C; p.T = T;
        for (int t = 0; t < T; ++t) p.thr[t] = thresholds[t];
        p.flags = flags; p.match = match; p.iou = iou; p.score = score; p.gt_per_class = reinterpret_cast<unsigned long long*>(gt_per_class);
        ACH_LAUNCH(ach::match_kernel, dim3(unsigned(B)), dim3(256), static_cast<hipStream_t>(stream), p);
    });
}

// ---- training batches from ragged frames (k_data.h).  Both entries check the host copy of the frame table — every extent against its arena, every table
// offset against `tabs`, every bounds / index entry the kernels will follow — BEFORE anything is launched; a bad table is ACH_ERR_INVALID and no launch.
static void data_need_bounds(const int32_t* tabs, int64_t tabs_len, int64_t boff, int64_t koff, int64_t ks, int64_t n_out, int64_t n_in, const char* what) {
    train_need(ks >= 1 && boff >= 0 && koff >= 0 && n_out <= (tabs_len - boff) / 2 && boff + 2 * n_out <= tabs_len && n_out <= (tabs_len - koff) / ks &&
               koff + n_out * ks <= tabs_len, what);
}
int ach_data_letterbox_batch(const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const int32_t* tabs_host,
                             const int32_t* tabs_dev, int64_t tabs_len, const float* lut, int32_t B, int32_t R, uint8_t* mid, int64_t mid_bytes, void* out,
                             int32_t out_kind, void* stream) {
    return train_guard([&] {
        train_need(arena && table_host && table_dev && tabs_host && tabs_dev && mid && out && B > 0 && R > 0 && R <= 16384 && tabs_len >= 0 && mid_bytes >= 0,
                   "ach_data_letterbox_batch");
        train_need(out_kind >= ach::DATA_F32 && out_kind <= ach::DATA_U8_HWC && (lut || out_kind == ach::DATA_U8_HWC), "ach_data_letterbox_batch: out_kind 0..3, a value table unless 3");
        train_need(arena_bytes > 0 && arena_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(arena) & 15u) == 0 && (reinterpret_cast<uintptr_t>(mid) & 3u) == 0,
                   "ach_data_letterbox_batch: the image arena is 16-byte aligned and padded to 16 bytes");
        const int R4 = (R + 3) / 4 * 4;
        long max_span = 0, max_rows = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t* f = table_host + long(b) * ach::DATA_TABLE_COLS;
            const int64_t off = f[0], H = f[1], W = f[2], pitch = f[3], nw = f[4], nh = f[5], dx = f[6], dy = f[7];
            train_need(H >= 1 && W >= 1 && H < (1L << 30) && W < (1L << 30) && pitch >= 3 * W && pitch < (1L << 32) && off >= 0 && off <= arena_bytes &&
                       (H - 1) * pitch + 3 * W <= arena_bytes - off, "ach_data_letterbox_batch: a frame's extent passes the image arena");
            train_need(nw >= 1 && nh >= 1 && nw < (1L << 30) && nh < (1L << 30) && dx > -(1L << 30) && dx < (1L << 30) && dy > -(1L << 30) && dy < (1L << 30),
                       "ach_data_letterbox_batch: placement out of range");
            data_need_bounds(tabs_host, tabs_len, f[8], f[9], f[10], nw, W, "ach_data_letterbox_batch: a horizontal table offset passes the table buffer");
            data_need_bounds(tabs_host, tabs_len, f[11], f[12], f[13], nh, H, "ach_data_letterbox_batch: a vertical table offset passes the table buffer");
            const ach::DataWindow w = ach::data_window(nw, nh, dx, dy, R);
            if (w.vx0 >= w.vx1 || w.vy0 >= w.vy1) continue;
            // the entries the kernels follow: inside the source axis, at most ks taps, both ends non-decreasing (the staged range is [first of the first, end of the last))
            auto walk = [&](int64_t boff, int64_t ks, long lo, long hi, int64_t n_in, long& first0, long& end1) {
                long pf = 0, pe = 0;
                for (long o = lo; o < hi; ++o) {
                    const long first = tabs_host[boff + 2 * o], count = tabs_host[boff + 2 * o + 1];
                    train_need(first >= 0 && count >= 0 && count <= ks && first + count <= n_in && (o == lo || (first >= pf && first + count >= pe)),
                               "ach_data_letterbox_batch: a bounds entry leaves its source axis");
                    pf = first; pe = first + count;
                    if (o == lo) first0 = first;
                }
                end1 = pe;
            };
            long sx0 = 0, sx1 = 0, r0 = 0, r1 = 0;
            walk(f[8], f[10], w.vx0 - dx, w.vx1 - dx, W, sx0, sx1);
            walk(f[11], f[13], w.vy0 - dy, w.vy1 - dy, H, r0, r1);
            train_need(f[14] >= 0 && f[14] % 4 == 0 && f[14] <= mid_bytes && (r1 - r0) * 3 * R4 <= mid_bytes - f[14],
                       "ach_data_letterbox_batch: a frame's intermediate passes the intermediate arena");
            max_span = std::max(max_span, (sx1 - sx0) * 3);
            max_rows = std::max(max_rows, r1 - r0);
        }
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (max_rows > 0 && max_span > 0) {
            const long lstride = (max_span + 15 + 15) / 16 * 16;
            if (lstride > ach::DATA_LDS_BYTES) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_data_letterbox_batch: a frame needs more than 16379 source columns of one row"};
            const int rows_pb = int(std::min<long>(ach::DATA_ROWS, ach::DATA_LDS_BYTES / lstride));
            ach::DataHParams hp{arena, reinterpret_cast<const long long*>(table_dev), tabs_dev, mid, R, R4, rows_pb, int(lstride)};
            ACH_LAUNCH(ach::data_hpass_kernel, dim3(unsigned(ach::cdivl(max_rows, rows_pb)), unsigned(B)), dim3(256), s, hp);
        }
        ach::DataVParams vp{reinterpret_cast<const long long*>(table_dev), tabs_dev, mid, lut, out, R, R4};
        const dim3 grid(unsigned(ach::cdivl(long(R) * (R4 / 4), 256)), unsigned(B));
        if (out_kind == ach::DATA_F32) ACH_LAUNCH(ach::data_vpass_kernel<float>, grid, dim3(256), s, vp);
        else if (out_kind == ach::DATA_BF16) ACH_LAUNCH(ach::data_vpass_kernel<ach::bf16_t>, grid, dim3(256), s, vp);
        else if (out_kind == ach::DATA_F16) ACH_LAUNCH(ach::data_vpass_kernel<ach::f16_t>, grid, dim3(256), s, vp);
        else ACH_LAUNCH(ach::data_vpass_kernel<uint8_t>, grid, dim3(256), s, vp);
    });
}
int ach_data_labels_batch(const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const int32_t* tabs_host,
                          const int32_t* tabs_dev, int64_t tabs_len, int32_t B, int32_t R, int32_t num_classes_seg, void* png, void* png_w, int32_t label_kind,
                          void* stream) {
    return train_guard([&] {
        train_need(arena && table_host && table_dev && tabs_host && tabs_dev && png && png_w && B > 0 && B <= 65535 && R > 0 && R <= 16384 && tabs_len >= 0 &&
                   arena_bytes >= 0, "ach_data_labels_batch");
        train_need(num_classes_seg >= 0 && num_classes_seg <= 255 && (label_kind == 0 || label_kind == 2), "ach_data_labels_batch: classes 0..255, label_kind 0 (int64) or 2 (uint8)");
        for (int b = 0; b < B; ++b) {
            const int64_t* f = table_host + long(b) * ach::DATA_TABLE_COLS;
            const int64_t nw = f[0], nh = f[1], dx = f[2], dy = f[3];
            train_need(nw >= 1 && nh >= 1 && nw < (1L << 30) && nh < (1L << 30) && dx > -(1L << 30) && dx < (1L << 30) && dy > -(1L << 30) && dy < (1L << 30),
                       "ach_data_labels_batch: placement out of range");
            const ach::DataWindow w = ach::data_window(nw, nh, dx, dy, R);
            for (int m = 0; m < 2; ++m) {
                const int64_t* g = f + 4 + 6 * m;
                if (g[0] < 0) continue;
                const int64_t off = g[0], H = g[1], W = g[2], pitch = g[3];
                train_need(H >= 1 && W >= 1 && H < (1L << 30) && W < (1L << 30) && pitch >= W && pitch < (1L << 32) && off <= arena_bytes &&
                           (H - 1) * pitch + W <= arena_bytes - off, "ach_data_labels_batch: a label map's extent passes the label arena");
                train_need(g[4] >= 0 && g[5] >= 0 && nw <= tabs_len - g[4] && nh <= tabs_len - g[5], "ach_data_labels_batch: an index table offset passes the table buffer");
                if (w.vx0 >= w.vx1 || w.vy0 >= w.vy1) continue;
                for (long o = w.vx0 - dx; o < w.vx1 - dx; ++o) train_need(tabs_host[g[4] + o] >= -1 && tabs_host[g[4] + o] < W, "ach_data_labels_batch: a column index leaves its map");
                for (long o = w.vy0 - dy; o < w.vy1 - dy; ++o) train_need(tabs_host[g[5] + o] >= -1 && tabs_host[g[5] + o] < H, "ach_data_labels_batch: a row index leaves its map");
            }
        }
        ach::DataLabelParams lp{arena, reinterpret_cast<const long long*>(table_dev), tabs_dev, {png, png_w}, R, num_classes_seg, label_kind == 0 ? 1 : 0};
        ACH_LAUNCH(ach::data_labels_kernel, dim3(unsigned(ach::cdivl(long(R) * R, 256)), 2u, unsigned(B)), dim3(256), static_cast<hipStream_t>(stream), lp);
    });
}

// ---- both radar inputs from raw point clouds (k_radarmap.h).  The host copy of the cloud table is checked against the arena — every extent, every column — and
// the sampled row indices against every frame's n BEFORE anything is launched; a bad table is ACH_ERR_INVALID and no launch.
static void radar_need_table(const int64_t* table_host, int32_t B, int64_t arena_elems, int64_t min_rows, const char* extent, const char* column) {
    for (int b = 0; b < B; ++b) {
        const int64_t* f = table_host + long(b) * ach::RADAR_TABLE_COLS;
        const int64_t off = f[0], n = f[1], F = f[2], stride = f[3];
        train_need(n >= min_rows && n < (1L << 40) && F >= 1 && F < (1L << 20) && stride >= F && stride < (1L << 20) && off >= 0 && off <= arena_elems &&
                   (n == 0 || (n - 1) * stride + F <= arena_elems - off), extent);
        for (int c = 4; c < 9; ++c) train_need(f[c] >= 0 && f[c] < F, column);
    }
}
int ach_data_radar_maps(const void* arena, int64_t arena_elems, int32_t in_kind, const int64_t* table_host, const int64_t* table_dev, int32_t B, int32_t R,
                        double cell_u, double cell_v, float* raw, float* partial, int64_t partial_floats, void* out, int32_t out_kind, void* stream) {
    return train_guard([&] {
        train_need(arena && table_host && table_dev && raw && B > 0 && B <= 65535 && R > 0 && arena_elems >= 0 &&
                   (in_kind == ach::RADAR_IN_F32 || in_kind == ach::RADAR_IN_F64), "ach_data_radar_maps");
        if (R > ach::RADAR_MAX_R) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_data_radar_maps: a map larger than 2048 x 2048"};
        train_need((reinterpret_cast<uintptr_t>(arena) & (in_kind == ach::RADAR_IN_F64 ? 7u : 3u)) == 0, "ach_data_radar_maps: the cloud arena is aligned to its element size");
        train_need(std::isfinite(cell_u) && std::isfinite(cell_v) && cell_u != 0.0 && cell_v != 0.0, "ach_data_radar_maps: the cell sizes are finite and not zero");
        const int rows = ach::radar_band_rows(R), bands = int(ach::cdivl(R, rows));
        train_need(!out || (out_kind >= ach::DATA_F32 && out_kind <= ach::DATA_F16 && partial && partial_floats >= 2L * B * bands),
                   "ach_data_radar_maps: the normalised map is fp32 / bf16 / fp16 (0..2) and needs 2 * B * ceil(R / band rows) floats of `partial`");
        radar_need_table(table_host, B, arena_elems, 0, "ach_data_radar_maps: a cloud's extent passes the cloud arena", "ach_data_radar_maps: a column index is not below F");
        hipStream_t s = static_cast<hipStream_t>(stream);
        ach::RadarMapParams p{arena, reinterpret_cast<const long long*>(table_dev), raw, out ? partial : nullptr, cell_u, cell_v, R, rows, bands, in_kind};
        ACH_LAUNCH(ach::radar_map_kernel, dim3(unsigned(bands), unsigned(B)), dim3(256), s, p);
        if (!out) return;
        const long per = 3L * R * R;
        ach::RadarScaleParams ps{raw, partial, out, per, bands, B};
        const dim3 grid(unsigned(ach::cdivl(per * B, 256)));
        if (out_kind == ach::DATA_F32) ACH_LAUNCH(ach::radar_scale_kernel<float>, grid, dim3(256), s, ps);
        else if (out_kind == ach::DATA_BF16) ACH_LAUNCH(ach::radar_scale_kernel<ach::bf16_t>, grid, dim3(256), s, ps);
        else ACH_LAUNCH(ach::radar_scale_kernel<ach::f16_t>, grid, dim3(256), s, ps);
    });
}
int ach_data_radar_points(const void* arena, int64_t arena_elems, int32_t in_kind, const int64_t* table_host, const int64_t* table_dev, const int64_t* indices_host,
                          const int64_t* indices_dev, const int32_t* columns, int32_t D, int32_t label_column, int32_t B, int32_t N, void* points,
                          int32_t out_kind, int64_t* labels, void* stream) {
    return train_guard([&] {
        train_need(arena && table_host && table_dev && indices_host && indices_dev && columns && points && B > 0 && N > 0 && arena_elems >= 0 &&
                   (in_kind == ach::RADAR_IN_F32 || in_kind == ach::RADAR_IN_F64) && out_kind >= ach::DATA_F32 && out_kind <= ach::DATA_F16, "ach_data_radar_points");
        train_need(D >= 1 && D <= ach::RADAR_MAX_D && long(B) * (D + 1) < (1L << 31), "ach_data_radar_points: 1..16 point columns");
        train_need((labels != nullptr) == (label_column >= 0), "ach_data_radar_points: a label column and a label output go together");
        train_need((reinterpret_cast<uintptr_t>(arena) & (in_kind == ach::RADAR_IN_F64 ? 7u : 3u)) == 0, "ach_data_radar_points: the cloud arena is aligned to its element size");
        radar_need_table(table_host, B, arena_elems, 1, "ach_data_radar_points: a cloud is empty or its extent passes the cloud arena",
                         "ach_data_radar_points: a column index is not below F");
        ach::RadarPointsParams p{arena, reinterpret_cast<const long long*>(table_dev), reinterpret_cast<const long long*>(indices_dev), points,
                                 reinterpret_cast<long long*>(labels), N, D, in_kind, label_column, {}};
        for (int b = 0; b < B; ++b) {
            const int64_t* f = table_host + long(b) * ach::RADAR_TABLE_COLS;
            for (int d = 0; d < D; ++d) train_need(columns[d] >= 0 && columns[d] < f[2], "ach_data_radar_points: a column index is not below F");
            train_need(label_column < f[2], "ach_data_radar_points: a column index is not below F");
            for (long i = 0; i < N; ++i) train_need(indices_host[long(b) * N + i] >= 0 && indices_host[long(b) * N + i] < f[1], "ach_data_radar_points: a row index is not below n");
        }
        for (int d = 0; d < D; ++d) p.cols[d] = columns[d];
        hipStream_t s = static_cast<hipStream_t>(stream);
        const dim3 grid(unsigned(B * (D + 1)));
        if (out_kind == ach::DATA_F32) ACH_LAUNCH(ach::radar_points_kernel<float>, grid, dim3(256), s, p);
        else if (out_kind == ach::DATA_BF16) ACH_LAUNCH(ach::radar_points_kernel<ach::bf16_t>, grid, dim3(256), s, p);
        else ACH_LAUNCH(ach::radar_points_kernel<ach::f16_t>, grid, dim3(256), s, p);
    });
}

// ---- serving a ragged batch (k_serve.h): both class maps at every frame's own size and the overlay image in ONE launch behind the two softmax launches, and the
// box correction with per-frame shapes.  The host copy of the frame table is checked against every arena before anything is launched.
int ach_seg_overlay_frames(ach_handle* h, int32_t batch, int32_t channels, const void* se_seg, const void* lane_seg, float* prob_se, float* prob_line,
                           const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const uint8_t* consts_host,
                           const uint8_t* consts_dev, int32_t palette_se_len, int32_t palette_line_len, float blend_se, float blend_line, int32_t use_lut,
                           uint8_t* out_semantic, int64_t semantic_bytes, uint8_t* out_waterline, int64_t waterline_bytes, uint8_t* out_overlay,
                           int64_t overlay_bytes, void* stream) {
    return guarded(h, [&] {
        const bool want_se = out_semantic || out_overlay, want_line = out_waterline || out_overlay;
        train_need(batch > 0 && batch <= 65535 && table_host && table_dev && (out_semantic || out_waterline || out_overlay), "ach_seg_overlay_frames: a batch, a frame table and an output");
        train_need((!want_se || (se_seg && prob_se && channels >= 1 && channels <= 255)) && (!want_line || (lane_seg && prob_line)),
                   "ach_seg_overlay_frames: every wanted output needs its head and probability workspace (1..255 classes)");
        const int R = h->eng->cfg.resolution, C0 = want_se ? channels : 0, C1 = want_line ? 2 : 0;
        if ((C0 + C1) * ach::SERVE_TW * 2 > ach::SERVE_LDS_FLOATS) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_seg_overlay_frames: more than 30 semantic classes"};
        auto aligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
        train_need(aligned(out_semantic) && aligned(out_waterline) && aligned(out_overlay) && semantic_bytes >= 0 && waterline_bytes >= 0 && overlay_bytes >= 0,
                   "ach_seg_overlay_frames: output arenas are 16-byte aligned");
        if (out_overlay) {
            train_need(arena && consts_host && consts_dev && aligned(arena) && arena_bytes > 0 && arena_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(consts_dev) & 3u) == 0,
                       "ach_seg_overlay_frames: the overlay needs the image arena (16-byte aligned, padded to 16 bytes) and the constants");
            train_need(blend_se >= 0.f && blend_se <= 1.f && blend_line >= 0.f && blend_line <= 1.f, "ach_seg_overlay_frames: blend factors lie in [0, 1]");
            train_need(palette_se_len >= 1 && palette_se_len <= 256 && palette_line_len >= 1 && palette_line_len <= 256, "ach_seg_overlay_frames: palettes hold 1..256 colours");
            for (int c = 0; c < channels; ++c)
                train_need(consts_host[ach::SERVE_REMAP_SE + c] < palette_se_len, "ach_seg_overlay_frames: the semantic palette is shorter than the remapped class range");
            for (int c = 0; c < 2; ++c)
                train_need(consts_host[ach::SERVE_REMAP_LINE + c] < palette_line_len, "ach_seg_overlay_frames: the water-line palette is shorter than the remapped class range");
        }
        const int rows = ach::serve_rows(C0 + C1);
        long blocks = 0;
        for (int b = 0; b < batch; ++b) {
            const int64_t* f = table_host + long(b) * ach::SERVE_TABLE_COLS;
            const int64_t H = f[1], W = f[2], y0 = f[4], x0 = f[5], nh = f[6], nw = f[7], mp = f[10];
            train_need(H >= 1 && W >= 1 && H < (1L << 30) && W < (1L << 30), "ach_seg_overlay_frames: a frame's H and W are at least 1");
            train_need(nh >= 1 && nw >= 1 && y0 >= 0 && x0 >= 0 && nh <= R - y0 && nw <= R - x0, "ach_seg_overlay_frames: a frame's window leaves the network map");
            if (out_semantic || out_waterline) train_need(mp >= W && mp % 16 == 0 && mp < (1L << 32), "ach_seg_overlay_frames: the class maps' pitch is a multiple of 16, at least W");
            if (out_semantic) train_need(f[8] >= 0 && f[8] % 16 == 0 && f[8] <= semantic_bytes && H * mp <= semantic_bytes - f[8], "ach_seg_overlay_frames: a frame's semantic map passes its arena");
            if (out_waterline) train_need(f[9] >= 0 && f[9] % 16 == 0 && f[9] <= waterline_bytes && H * mp <= waterline_bytes - f[9], "ach_seg_overlay_frames: a frame's water-line map passes its arena");
            if (out_overlay) {
                const int64_t off = f[0], pitch = f[3], op = f[12];
                train_need(pitch >= 3 * W && pitch < (1L << 32) && off >= 0 && off <= arena_bytes && (H - 1) * pitch + 3 * W <= arena_bytes - off,
                           "ach_seg_overlay_frames: a frame's extent passes the image arena");
                train_need(op >= 3 * W && op % 16 == 0 && op < (1L << 32) && f[11] >= 0 && f[11] % 16 == 0 && f[11] <= overlay_bytes && H * op <= overlay_bytes - f[11],
                           "ach_seg_overlay_frames: a frame's overlay passes its arena");
            }
            blocks = std::max(blocks, ach::cdivl(W, ach::SERVE_TW) * ach::cdivl(nh, rows - 1));
        }
        train_need(blocks < (1L << 31), "ach_seg_overlay_frames: a frame is too large");
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (want_se) h->eng->seg_softmax(batch, channels, se_seg, prob_se, s);
        if (want_line) h->eng->seg_softmax(batch, 2, lane_seg, prob_line, s);
        ach::ServeParams p{prob_se, prob_line, arena, reinterpret_cast<const long long*>(table_dev), consts_dev, out_semantic, out_waterline, out_overlay,
                           R, C0, C1, rows, blend_se, blend_line, use_lut != 0};
        ACH_LAUNCH(ach::seg_overlay_frames_kernel, dim3(unsigned(blocks), unsigned(batch)), dim3(256), s, p);
    });
}
int ach_correct_boxes_frames(ach_handle* h, int32_t batch, int32_t max_det, const float* rows, const int32_t* count, const int32_t* shapes_host,
                             const int32_t* shapes_dev, int32_t letterbox, float* out_rows, void* stream) {
    return guarded(h, [&] {
        train_need(batch > 0 && max_det > 0 && rows && count && shapes_host && shapes_dev && out_rows, "ach_correct_boxes_frames");
        for (int b = 0; b < batch; ++b) train_need(shapes_host[2 * b] >= 1 && shapes_host[2 * b + 1] >= 1, "ach_correct_boxes_frames: a frame's H and W are at least 1");
        h->eng->correct_boxes_frames(batch, max_det, rows, count, shapes_dev, letterbox, out_rows, static_cast<hipStream_t>(stream));
    });
}

// ---- drawing the kept detections on served frames (k_draw.h): box rings, label plates and label text of a ragged batch in two launches, in place.  Stateless.
// Every host table is checked before anything is launched; what comes from DEVICE data (count, class id, score, coordinates) is bounded by the kernels themselves.
int ach_draw_detections_frames(uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, int32_t batch, const float* boxes,
                               const int32_t* count, int32_t max_det, int32_t num_classes, const int32_t* labels_host, const int32_t* labels_dev, int64_t num_labels,
                               const uint8_t* blob_dev, int64_t blob_bytes, const uint8_t* style_dev, int32_t* records, int32_t* class_counts, void* stream) {
    return train_guard([&] {
        train_need(arena && table_host && table_dev && boxes && count && labels_host && labels_dev && blob_dev && style_dev && records && batch > 0 && batch <= 65535 &&
                   arena_bytes > 0 && num_labels > 0 && num_labels < (1L << 24) && blob_bytes >= 0, "ach_draw_detections_frames");
        train_need(max_det >= 1 && max_det <= ach::DRAW_MAX_DET, "ach_draw_detections_frames: max_det is 1..1024");
        train_need(num_classes >= 1 && num_classes <= ach::DRAW_MAX_CLASSES, "ach_draw_detections_frames: num_classes is 1..256");
        train_need((reinterpret_cast<uintptr_t>(arena) & 3u) == 0 && (reinterpret_cast<uintptr_t>(records) & 15u) == 0,
                   "ach_draw_detections_frames: the arena is 4-byte aligned and the record workspace 16-byte aligned");
        for (int64_t l = 0; l < num_labels; ++l) {
            const int32_t* L = labels_host + l * ach::DRAW_LABEL_COLS;
            train_need(L[0] >= 0 && L[1] >= 0 && L[2] >= 0 && L[1] <= 4096 && L[2] <= 4096 && int64_t(L[1]) * L[2] <= blob_bytes - L[0],
                       "ach_draw_detections_frames: a label's mask passes the atlas blob");
            train_need(L[3] >= -65536 && L[3] <= 65536 && L[4] >= -65536 && L[4] <= 65536 && L[5] >= 0 && L[5] <= 65536 && L[6] >= 0 && L[6] <= 65536,
                       "ach_draw_detections_frames: a label's offsets and size are out of range");
        }
        long blocks = 0;
        for (int b = 0; b < batch; ++b) {
            const int64_t* f = table_host + long(b) * ach::DRAW_TABLE_COLS;
            const int64_t off = f[0], H = f[1], W = f[2], pitch = f[3];
            train_need(H >= 1 && W >= 1 && H <= (1L << 20) && W <= (1L << 20), "ach_draw_detections_frames: a frame's H and W are 1..2^20");
            train_need(pitch >= 3 * W && pitch % 4 == 0 && pitch < (1L << 32) && off >= 0 && off % 4 == 0 && off <= arena_bytes && H * pitch <= arena_bytes - off,
                       "ach_draw_detections_frames: a frame's extent passes the arena (offset and pitch are multiples of 4, pitch >= 3 W)");
            train_need(f[4] >= 1 && f[4] <= ach::DRAW_MAX_THICKNESS, "ach_draw_detections_frames: thickness is 1..64");
            train_need(f[5] >= 0 && f[5] <= num_labels - int64_t(num_classes) * ach::DRAW_SCORES, "ach_draw_detections_frames: a frame's atlas base passes the label table");
            blocks = std::max(blocks, ach::cdivl(W, ach::DRAW_TW) * ach::cdivl(H, ach::DRAW_TH));
        }
        train_need(blocks < (1L << 31), "ach_draw_detections_frames: a frame is too large");
        hipStream_t s = static_cast<hipStream_t>(stream);
        ach::DrawParams p{boxes, count, records, arena, reinterpret_cast<const long long*>(table_dev), labels_dev, blob_dev, style_dev, class_counts, max_det, num_classes};
        ACH_LAUNCH(ach::draw_prepare_kernel, dim3(unsigned(batch)), dim3(256), s, p);
        ACH_LAUNCH(ach::draw_tiles_kernel, dim3(unsigned(blocks), unsigned(batch)), dim3(256), s, p);
    });
}

}  // extern "C"
