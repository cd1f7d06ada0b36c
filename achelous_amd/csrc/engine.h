// engine.h — host side of the engine: state-dict ingestion, constant folding, weight packing, activation arena
// and the launch plan.  Compiled by hipcc into libachelous_hip.so (and by g++ against tests/hostemu for the CPU
// emulation used by the unit tests).  See include/achelous.h for the C ABI and DESIGN.md for the data layout.
#pragma once
#include <cstdlib>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/achelous.h"
#include "ach_platform.h"
#include "engine_schedule.h"

namespace ach {

struct AchError {
    int code;
    std::string msg;
};

struct HostTensor {
    std::vector<float> data;
    std::vector<long> shape;
    long numel() const { long n = 1; for (long s : shape) n *= s; return n; }
};

struct TapInfo {
    const void* ptr = nullptr;
    int kind = 0;                 // 0: NHWC activation [B,H,W,C] (ld) -> NCHW ; 1: NCHW dense ; 2: rows [R, C] (ld) ; 3: user output (not readable)
    int B = 0, H = 0, W = 0, C = 0;
    long ld = 0;
    int is_f32 = 0;               // buffer holds fp32 regardless of the engine dtype
    int is_i32 = 0;               // buffer holds int32 (index selections); read back as exact floats
    int add_eye = 0;              // rows kind: add identity of this size (PointNet transforms are stored without +I)
};

struct Op {
    std::string name;
    std::function<void(hipStream_t)> fn;
    double bytes = 0;             // algorithmic HBM bytes of one launch: inputs read once + outputs written once + weights, REAL channels
    double layout_bytes = 0;      // the same count over the pixel pitches actually stored (channel padding included): what the launch must move
    double flops = 0;             // 2 * MACs of one launch (dense contractions only)
    int stream = 0;               // 0: caller's stream (image path) ; 1, 2: engine-owned side streams (radar / point branches)
    // joins inside the forward: one bit per JoinEvent the launch waits for before it starts / records behind it.  Pipelined forwards: one bit per cross-forward
    // dependency (XDep).  `xwait`: the first launch of its stream to overwrite buffers that the PREVIOUS forward still reads through that dependency -> waits
    // for that forward's `xsignal` launch, the last one that reads them.  (engine_schedule.h places all four)
    unsigned char wait = 0, signal = 0, xwait = 0, xsignal = 0;
};

struct IoPtrs {
    const void* image = nullptr; const void* radar = nullptr; const void* points = nullptr;
    void* det[3] = {nullptr, nullptr, nullptr};
    void* se = nullptr; void* lane = nullptr; void* pc = nullptr;
};

class EngineBase {
public:
    explicit EngineBase(const ach_config& c) : cfg(c) {}
    virtual ~EngineBase();
    ach_config cfg;
    std::map<std::string, HostTensor> weights;
    std::string last_error;

    // device memory owned by the engine
    char* warena = nullptr; size_t warena_cap = 0, warena_used = 0;      // packed weights / constants
    char* aarena = nullptr; size_t aarena_cap = 0, aarena_used = 0;      // activations
    bool measuring = false;
    // the options (ach_set_option): key, member, default, normalisation rule and the measurement behind each default are stated once, in engine_options.h
#define ACH_OPTION(key, type, member, def, rule, lo, hi) type member = def;
#include "engine_options.h"
#undef ACH_OPTION
    int batch = 0;
    std::vector<Op> ops;
    std::map<std::string, TapInfo> taps;
    std::vector<std::string> tap_order;
    IoPtrs io;

    void load(const ach_tensor_desc* t, size_t n);
    static const char* option_key(int index);                 // nullptr past the end of the table
    void set_option(const char* key, int value);              // normalises by the option's rule, stores, and invalidates the plan
    int get_option(const char* key) const;                    // the stored (normalised) value
    // The plan was built from the weights and the options: whatever replaces either drops it (launches, taps, probes, graphs; batch = 0), and ach_forward
    // refuses to run until ach_plan.  The arenas stay, and so do `issued`, `joined` and the events: pipelined forwards in flight finish and can be joined.
    void invalidate_plan();
    virtual void plan(int B) = 0;
    void run(hipStream_t s);            // graph replay when possible, else eager launches
    void run_eager(hipStream_t s);
    void join(hipStream_t s);           // pipelined mode: `s` waits for the oldest forward that has not been joined yet (no-op when none)
    long forwards_in_flight() const { return issued - joined; }
    // transient: extra launches enqueued behind the last op of the detection branch (stream 1) by ach_forward_detect
    std::function<void(hipStream_t)> detect_tail;
    void run_profiled(hipStream_t s, float* op_ms, size_t cap);
    // live probes: HIP events around ONE op of the plan (slot 0: set_probe) or around a RUN of ops first..last that sit on one stream
    // (slot 1: set_probe_range — the neck + decoder sub-path of the caller's stream) on every run() (bench.py's roofline leg)
    void set_probe(int op_index) { set_probe_range(0, op_index, op_index); }
    void read_probe(float* avg_ms, int* samples) { read_probe_slot(0, avg_ms, samples); }
    void set_probe_range(int slot, int first, int last);
    void read_probe_slot(int slot, float* avg_ms, int* samples);
    virtual void decode(int B, const void* d3, const void* d4, const void* d5, float* out, hipStream_t s) = 0;
    // fp16 storage: how many elements of the plan's activation tensors are saturated (+-65504: every kernel of the fp16 engine runs with MODE.FP16_OVFL, so an
    // overflowing conversion clamps instead of becoming infinity) or non-finite after the forward(s) enqueued on `s` so far; synchronises `s`.  0 for the other engines.
    virtual unsigned long long count_saturated(hipStream_t s) = 0;
    std::vector<std::pair<const void*, size_t>> t_regions;       // activation tensors held in the storage type: (device pointer, bytes), filled by plan()
    void* sat_dev = nullptr; size_t sat_dev_regions = 0;         // device copy of t_regions + the counter (count_saturated)
    void note_region(const void* p, size_t bytes) { if (!measuring) t_regions.emplace_back(p, bytes); }
    void nms(int B, const float* decoded, float conf, float iou, int max_det, float* rows, int* idx, int* count,
             void* workspace, hipStream_t s);
    void nms_wide(int B, const float* decoded, float conf, float iou, int max_det, float* rows, int* idx, int* count,
                  void* workspace, hipStream_t s);            // more than NMS_MAXA anchors (k_nmswide.h); nms() dispatches
    size_t nms_workspace_bytes(int B) const;
    int num_anchors() const;
    void read_tap(const std::string& name, float* out, size_t cap);
    std::vector<long> tap_shape(const std::string& name) const;
    // pre / post-processing around the forward (k_prepost.h)
    virtual void preprocess_radar(int B, int C, const float* in, void* out, hipStream_t s) = 0;
    virtual void normalize_points(int B, int N, int D, const float* in, void* out, hipStream_t s) = 0;
    virtual void preprocess_image(int B, const unsigned char* in, void* out, hipStream_t s) = 0;
    virtual void seg_argmax(int B, int C, const void* seg, unsigned char* out, hipStream_t s) = 0;
    virtual void seg_resize_argmax(int B, int C, const void* seg, int out_h, int out_w, float* prob_ws, unsigned char* out, hipStream_t s) = 0;
    void correct_boxes(int B, int max_det, const float* rows, const int* count, int img_h, int img_w, int letterbox, float* out, hipStream_t s);
    // the ragged-batch forms (k_serve.h, k_prepost.h): the softmax of one head into an fp32 workspace [B, C, R, R] (what seg_resize_argmax runs first), and the box
    // correction with every frame's (H, W) read from an int32 [B, 2] table on the device
    virtual void seg_softmax(int B, int C, const void* seg, float* prob_ws, hipStream_t s) = 0;
    void correct_boxes_frames(int B, int max_det, const float* rows, const int* count, const int* shapes_dev, int letterbox, float* out, hipStream_t s);
    float* prepost_scratch = nullptr; size_t prepost_scratch_bytes = 0;
    // micro-benchmark hook: time the MFMA GEMM kernel alone on scratch buffers (ms per launch)
    virtual float bench_gemm(int M, int K, int N, int act, int ln, int residual, int P, int iters, hipStream_t s) = 0;

protected:
    const HostTensor& W(const std::string& key) const;
    bool hasW(const std::string& key) const { return weights.count(key) != 0; }
    void* walloc(size_t bytes);
    // The activation arena must stay a NON-REUSING bump allocator (no buffer handed out twice inside a plan) while options radar_bg / radar_pool_sparse
    // keep occupancy masks and maps in it from one forward to the next: a lifetime-based reuse of the arena would overwrite them between forwards.
    void* aalloc(size_t bytes);
    float* up_f32(const std::vector<float>& v);
    void* up_raw(const void* src, size_t bytes);        // opaque constants (pre-packed MFMA fragments)
    bool skip_warned = false;
    void add_op(const std::string& name, std::function<void(hipStream_t)> fn, double bytes = 0, double flops = 0, double layout_bytes = -1) {
        if (measuring) return;
        // timing experiments only (profiles/scripts/skip_ops.sh): ACH_DEBUG_SKIP="substr,substr" turns the matching launches into no-ops
        // (events and stream order stay) to read off what a kernel group costs END TO END; the outputs are garbage then.  Compiled ONLY into
        // the variant libraries that profiles/scripts/build_variant.sh builds with -DACH_TIMING_HOOKS: the shipped library never reads the variable.
#if defined(ACH_TIMING_HOOKS)
        if (const char* skip = std::getenv("ACH_DEBUG_SKIP")) {
            std::string all(skip);
            for (size_t a = 0; a < all.size();) {
                size_t b = all.find(',', a); if (b == std::string::npos) b = all.size();
                if (b > a && name.find(all.substr(a, b - a)) != std::string::npos) {
                    fn = [](hipStream_t) {};
                    if (!skip_warned) { skip_warned = true; std::fprintf(stderr, "achelous: ACH_DEBUG_SKIP is set: matching launches are no-ops, outputs are GARBAGE (timing experiments only)\n"); }
                    break;
                }
                a = b + 1;
            }
        }
        // ACH_DEBUG_ONLY="substr,substr": the complement — every launch that matches NONE of the substrings becomes a no-op.  tests/test_gpu_coresidency.py builds
        // its AGGRESSOR engines this way (a plan reduced to the row-walking heads, or the radar front kernels, or the band kernels, looping on its own stream
        // beside a victim forward of the SHIPPED library); an aggressor's outputs are never looked at.
        if (const char* only = std::getenv("ACH_DEBUG_ONLY")) {
            std::string all(only);
            bool keep = false;
            for (size_t a = 0; a < all.size() && !keep;) {
                size_t b = all.find(',', a); if (b == std::string::npos) b = all.size();
                if (b > a && name.find(all.substr(a, b - a)) != std::string::npos) keep = true;
                a = b + 1;
            }
            if (!keep && !all.empty()) fn = [](hipStream_t) {};
        }
#endif
        Op op{name, std::move(fn), bytes, layout_bytes < 0 ? bytes : layout_bytes, flops};
        op.stream = cur_stream;
        op.wait = pending.wait; op.xwait = pending.xwait;
        pending = {};
        ops.push_back(std::move(op));
    }
    // branch bookkeeping while the plan is built
    // the builder functions announce where they are; the schedule (engine_schedule.h, computed at the top of build()) says what that means: enter() — the launches
    // that follow run on the segment's stream, the first of them behind the segment's waits; reached() — the last launch so far records the point's events
    Schedule sched;
    int cur_stream = 0;
    Schedule::Marks pending;          // waits of the next launch
    void wait_next(const Schedule::Marks& m) { pending.wait |= m.wait; pending.xwait |= m.xwait; }
    void enter(Segment g) { cur_stream = sched.stream[g]; wait_next(sched.enter[g]); }
    void reached(Point p) { wait_next(sched.at[p]); if (!measuring && !ops.empty()) { ops.back().signal |= sched.at[p].signal; ops.back().xsignal |= sched.at[p].xsignal; } }
    static constexpr int kSideStreams = 3;
    hipStream_t side_stream[kSideStreams] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kJoinEvents] = {nullptr, nullptr, nullptr, nullptr}, ev_end[kSideStreams] = {nullptr, nullptr, nullptr};
    bool streams_ready = false;
    void ensure_streams();
    // pipelined mode: two alternating event sets (forward k uses set k & 1)
    struct XEvent { hipEvent_t ev[2] = {nullptr, nullptr}; bool recorded[2] = {false, false}; };
    XEvent xdep[kXDeps];
    hipEvent_t ev_done[kSideStreams][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    bool done_used[2][kSideStreams] = {{false, false, false}, {false, false, false}};
    long issued = 0, joined = 0;
#if !defined(ACH_HOSTEMU)
    struct GraphEntry { IoPtrs io; hipGraphExec_t exec; unsigned long stamp; };
    std::vector<GraphEntry> graphs;
    hipStream_t capture_stream = nullptr;
    unsigned long graph_clock = 0;
    bool graph_failed = false;
    void drop_graphs();
#endif
    static constexpr int kProbeEvents = 512, kProbeSlots = 3;
    struct Probe { int first = -1, last = -1; std::vector<hipEvent_t> ev0, ev1; long count = 0; };
    Probe probes[kProbeSlots];
    bool probing() const { for (const auto& pr : probes) if (pr.first >= 0) return true; return false; }
    void add_tap(const std::string& name, const TapInfo& t) { if (!measuring) { if (!taps.count(name)) tap_order.push_back(name); taps[name] = t; } }
    void reset_plan(int B);          // the start of a build() for batch B: no plan, no pending marks, empty arenas
};

EngineBase* make_engine(const ach_config& cfg);

}  // namespace ach
