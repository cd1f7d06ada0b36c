// api.cpp — the extern "C" boundary of libachelous_hip.so (declared in include/achelous.h): the entries that take a handle.  api_train.cpp has the training,
// loss and metric kernels' entries, api_frames.cpp those of the ragged-batch data, serving and drawing kernels; api_util.h what the three share.
// No exception crosses the boundary: every failure becomes a negative code + a message retrievable with ach_last_error().
#include <cstring>

#include "api_util.h"

thread_local std::string g_stateless_error;

extern "C" {

int ach_create(const ach_config* cfg, ach_handle** out) {
    if (!cfg || !out) return ACH_ERR_INVALID;
    try {
        if (cfg->backbone != ACH_BACKBONE_EDGENEXT && cfg->backbone != ACH_BACKBONE_MOBILEVIT && cfg->backbone != ACH_BACKBONE_POOLFORMER && cfg->backbone != ACH_BACKBONE_REPVIT)
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
        g_stateless_error = e.msg;
        return e.code;
    } catch (...) {
        g_stateless_error = "allocation failure";
        return ACH_ERR_NOMEM;
    }
}

void ach_destroy(ach_handle* h) {
    if (!h) return;
    delete h->eng;
    delete h;
}

const char* ach_last_error(const ach_handle* h) { return h ? h->err.c_str() : g_stateless_error.c_str(); }

int ach_load_weights(ach_handle* h, const ach_tensor_desc* tensors, size_t n) { return guarded(h, [&] { h->eng->load(tensors, n); }); }

// options: lookups in the table of engine_options.h (engine.cpp).  ach_get_option reads the engine only; a failure still sets the handle's last error.
int ach_set_option(ach_handle* h, const char* key, int32_t value) { return guarded(h, [&] { h->eng->set_option(key, value); }); }
int ach_get_option(const ach_handle* h, const char* key, int32_t* value) {
    return guarded(const_cast<ach_handle*>(h), [&] { if (!value) throw ach::AchError{ACH_ERR_INVALID, "null option value"}; *value = h->eng->get_option(key); });
}
const char* ach_option_key(int32_t index) { return ach::EngineBase::option_key(index); }

int ach_plan(ach_handle* h, int32_t batch) { return guarded(h, [&] { h->eng->plan(batch); }); }

size_t ach_arena_bytes(const ach_handle* h) { return (h && h->eng) ? h->eng->aarena_used + h->eng->warena_used : 0; }

// the I/O pointers of a forward into the plan's IoPtrs; `more`: the entry's further pointers that go into the same null check
static void bind_io(ach::EngineBase* e, const char* unplanned, const char* null_pointer, bool more, const void* image, const void* radar, const void* points,
                    void* det3, void* det4, void* det5, void* se_seg, void* lane_seg, void* pc_seg) {
    if (e->ops.empty()) throw ach::AchError{ACH_ERR_INVALID, unplanned};
    if (!image || !radar || !det3 || !det4 || !det5 || !se_seg || !lane_seg || !more || (e->cfg.pc_seg != ACH_PCSEG_NONE && (!points || !pc_seg)))
        throw ach::AchError{ACH_ERR_INVALID, null_pointer};
    ach::IoPtrs& io = e->io;
    io.image = image; io.radar = radar; io.points = points;
    io.det[0] = det3; io.det[1] = det4; io.det[2] = det5; io.se = se_seg; io.lane = lane_seg; io.pc = pc_seg;
}
int ach_forward(ach_handle* h, const void* image, const void* radar, const void* points, void* det3, void* det4, void* det5,
                void* se_seg, void* lane_seg, void* pc_seg, void* stream) {
    return guarded(h, [&] {
        bind_io(h->eng, "ach_plan must precede ach_forward", "null input/output pointer", true, image, radar, points, det3, det4, det5, se_seg, lane_seg, pc_seg);
        h->eng->run(as_stream(stream));
        launch_check();
    });
}

int ach_forward_detect(ach_handle* h, const void* image, const void* radar, const void* points, void* det3, void* det4, void* det5,
                       void* se_seg, void* lane_seg, void* pc_seg, float* decoded, float conf_thres, float nms_thres, int32_t max_det,
                       float* out_rows, int32_t* out_idx, int32_t* out_count, void* workspace, void* stream) {
    return guarded(h, [&] {
        ach::EngineBase* e = h->eng;
        bind_io(e, "ach_plan must precede ach_forward_detect", "null input/output pointer", true, image, radar, points, det3, det4, det5, se_seg, lane_seg, pc_seg);
        if (max_det <= 0 || !decoded || !out_rows || !out_idx || !out_count || !workspace)
            throw ach::AchError{ACH_ERR_INVALID, "bad detect arguments"};
        const int B = e->batch;
        e->detect_tail = [=](hipStream_t st) {
            e->decode(B, det3, det4, det5, decoded, st);
            e->nms(B, decoded, conf_thres, nms_thres, max_det, out_rows, out_idx, out_count, workspace, st);
        };
        struct Clear { ach::EngineBase* e; ~Clear() { e->detect_tail = nullptr; } } clear{e};
        e->run_eager(as_stream(stream));          // the tail carries per-call arguments: never replayed from a graph
        launch_check();
    });
}

int ach_join(ach_handle* h, void* stream) { return guarded(h, [&] { h->eng->join(as_stream(stream)); }); }
int ach_forwards_in_flight(const ach_handle* h) { return (h && h->eng) ? int(h->eng->forwards_in_flight()) : 0; }

int ach_decode(ach_handle* h, int32_t batch, const void* det3, const void* det4, const void* det5, float* decoded, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || !det3 || !det4 || !det5 || !decoded) throw ach::AchError{ACH_ERR_INVALID, "bad decode arguments"};
        h->eng->decode(batch, det3, det4, det5, decoded, as_stream(stream));
    });
}

size_t ach_nms_workspace_bytes(const ach_handle* h, int32_t batch) { return (h && h->eng) ? h->eng->nms_workspace_bytes(batch) : 0; }

int ach_nms(ach_handle* h, int32_t batch, const float* decoded, float conf_thres, float nms_thres, int32_t max_det,
            float* out_rows, int32_t* out_idx, int32_t* out_count, void* workspace, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || max_det <= 0 || !decoded || !out_rows || !out_idx || !out_count || !workspace)
            throw ach::AchError{ACH_ERR_INVALID, "bad nms arguments"};
        h->eng->nms(batch, decoded, conf_thres, nms_thres, max_det, out_rows, out_idx, out_count, workspace, as_stream(stream));
    });
}

int ach_preprocess_radar(ach_handle* h, int32_t batch, int32_t channels, const float* in, void* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || channels <= 0 || !in || !out) throw ach::AchError{ACH_ERR_INVALID, "bad preprocess_radar arguments"};
        h->eng->preprocess_radar(batch, channels, in, out, as_stream(stream));
    });
}
int ach_normalize_points(ach_handle* h, int32_t batch, int32_t n, int32_t d, const float* in, void* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || n <= 0 || d <= 0 || !in || !out) throw ach::AchError{ACH_ERR_INVALID, "bad normalize_points arguments"};
        h->eng->normalize_points(batch, n, d, in, out, as_stream(stream));
    });
}
int ach_preprocess_image(ach_handle* h, int32_t batch, const uint8_t* in, void* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || !in || !out) throw ach::AchError{ACH_ERR_INVALID, "bad preprocess_image arguments"};
        h->eng->preprocess_image(batch, in, out, as_stream(stream));
    });
}
int ach_seg_argmax(ach_handle* h, int32_t batch, int32_t channels, const void* seg, uint8_t* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || channels <= 0 || channels > 255 || !seg || !out) throw ach::AchError{ACH_ERR_INVALID, "bad seg_argmax arguments"};
        h->eng->seg_argmax(batch, channels, seg, out, as_stream(stream));
    });
}

int ach_seg_resize_argmax(ach_handle* h, int32_t batch, int32_t channels, const void* seg, int32_t out_h, int32_t out_w, float* prob_workspace,
                          uint8_t* out, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || channels <= 0 || channels > 255 || out_h <= 0 || out_w <= 0 || !seg || !prob_workspace || !out)
            throw ach::AchError{ACH_ERR_INVALID, "bad seg_resize_argmax arguments"};
        h->eng->seg_resize_argmax(batch, channels, seg, out_h, out_w, prob_workspace, out, as_stream(stream));
    });
}
int ach_correct_boxes(ach_handle* h, int32_t batch, int32_t max_det, const float* rows, const int32_t* count, int32_t image_h, int32_t image_w,
                      int32_t letterbox, float* out_rows, void* stream) {
    return guarded(h, [&] {
        if (batch <= 0 || max_det <= 0 || image_h <= 0 || image_w <= 0 || !rows || !count || !out_rows) throw ach::AchError{ACH_ERR_INVALID, "bad correct_boxes arguments"};
        h->eng->correct_boxes(batch, max_det, rows, count, image_h, image_w, letterbox, out_rows, as_stream(stream));
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
        const int rc = fn(send_record, recv_records, ach_record_words(batch, max_det), /* ncclInt32 */ 2, comm, as_stream(stream));
        if (rc != 0) throw ach::AchError{ACH_ERR_DEVICE, "ncclAllGather failed with code " + std::to_string(rc)};
#endif
    });
}

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
        *count = uint64_t(h->eng->count_saturated(as_stream(stream)));
    });
}
int ach_plan_launches(const ach_handle* h) { return (h && h->eng) ? int(h->eng->ops.size()) : 0; }
static const ach::Op* op_at(const ach_handle* h, int i) { return (h && h->eng && i >= 0 && i < int(h->eng->ops.size())) ? &h->eng->ops[size_t(i)] : nullptr; }
const char* ach_op_name(const ach_handle* h, int i) { const ach::Op* op = op_at(h, i); return op ? op->name.c_str() : nullptr; }
double ach_op_bytes(const ach_handle* h, int i) { const ach::Op* op = op_at(h, i); return op ? op->bytes : 0; }
double ach_op_layout_bytes(const ach_handle* h, int i) { const ach::Op* op = op_at(h, i); return op ? op->layout_bytes : 0; }
int ach_op_stream(const ach_handle* h, int i) { const ach::Op* op = op_at(h, i); return op ? op->stream : -1; }
int ach_op_sync(const ach_handle* h, int i, int* wait, int* signal, int* xwait, int* xsignal) {
    const ach::Op* op = op_at(h, i);
    return (op && wait && signal && xwait && xsignal) ? (*wait = op->wait, *signal = op->signal, *xwait = op->xwait, *xsignal = op->xsignal, ACH_OK) : ACH_ERR_INVALID;
}
double ach_op_flops(const ach_handle* h, int i) { const ach::Op* op = op_at(h, i); return op ? op->flops : 0; }
int ach_forward_profiled(ach_handle* h, const void* image, const void* radar, const void* points, void* det3, void* det4,
                         void* det5, void* se_seg, void* lane_seg, void* pc_seg, void* stream, float* op_ms, size_t capacity) {
    return guarded(h, [&] {
        bind_io(h->eng, "ach_plan must precede ach_forward", "null pointer", op_ms != nullptr, image, radar, points, det3, det4, det5, se_seg, lane_seg, pc_seg);
        h->eng->run_profiled(as_stream(stream), op_ms, capacity);
    });
}
int ach_bench_gemm(ach_handle* h, int M, int K, int N, int act, int ln, int residual, int P, int iters, void* stream, float* ms) {
    return guarded(h, [&] {
        if (M <= 0 || K <= 0 || N <= 0 || iters <= 0 || !ms) throw ach::AchError{ACH_ERR_INVALID, "bad bench arguments"};
        *ms = h->eng->bench_gemm(M, K, N, act, ln, residual, P, iters, as_stream(stream));
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

}  // extern "C"
