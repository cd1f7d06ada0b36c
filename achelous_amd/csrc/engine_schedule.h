// engine_schedule.h — the launch schedule of a plan, stated once (host only): the stream of each segment of the forward, the join events its first launch waits for, the events
// each point of the build records, and the cross-forward marks of the pipelined plan.  make_schedule() is the only reader of the options behind it; build() computes it first, and the builder
// functions of engine_impl.h only announce where they are: enter(segment), reached(point).  tests/golden/plan_schedules.json pins the result: a change of schedule is a diff of that listing.
#pragma once
#include "../../include/achelous.h"
namespace ach {
// The joins inside one forward: a launch carries one bit per event it waits for (`wait`) / records (`signal`); run_eager takes the lower event first.
enum JoinEvent {
    kEvRadarRelease = 0,  // the backbone stage after which the radar branch may start (option "radar_start")
    kEvFpnOutputs = 1,    // the residual adds have written the FPN outputs: fusion + head may start (and, dec_fork = 1, the attention stage on stream 2)
    kEvDecoderFork = 2,   // the decoder side of the neck may leave its stream: at the backbone's end (dec_fork = 3), at p3 (2), behind the attention stage (0, split_decoders)
    kEvRadarPyramid = 3,  // the radar branch's last launch (waited for only with head_stream = 1: otherwise fusion follows it in stream order)
    kJoinEvents = 4
};
// The cross-forward dependencies of the pipelined plan (option "pipeline"; run_eager in engine.cpp): buffers are not double-buffered, so forward k+1 may overwrite something
// only after forward k has read it for the last time.  Each has a pair of alternating events; a launch carries one bit per dependency it waits for / signals.
enum XDep {
    kXFusion = 0,     // fusion's reads of the FPN outputs / attention maps and the radar pyramid: the first neck launch and the first radar launch of the next forward wait for this forward's fusion launch
    kXDecoders = 1,   // the same for the DECODERS' reads of the attention maps: since fusion + head moved to the radar stream (head_stream = 0) the fusion launch no longer follows the decoders in stream order, so kXFusion alone would let the next forward's neck overwrite what this forward's decoders still read
    kXNeck = 2,       // option dec_fork = 3 (the NECK on stream 2): the backbone launch that first writes a feature map the previous forward's neck reads (stage 1's output, a slice of the neck's concat buffer) waits for that neck's last reader of the backbone's maps
    kXDeps = 3
};
enum Segment { kSegPoints, kSegRadar, kSegBackbone, kSegNeck /* SPP .. p3 */, kSegResidual, kSegAttention, kSegLaneDecoder, kSegSeDecoder, kSegDetect /* fusion + head */, kSegments };
// (kPtStage0 + k: backbone stage k done; kPtConcatSlice: the next launch writes a stage output that is a slice of the neck's concat buffers; kPtFusion: fusion's last launch)
enum Point { kPtStage0, kPtStage1, kPtStage2, kPtStage3, kPtConcatSlice, kPtBackboneEnd, kPtP3, kPtFpnOutputs, kPtAttention, kPtDecodersEnd, kPtRadarPyramid, kPtFusion, kPoints };
struct Schedule {
    struct Marks { unsigned char wait = 0, signal = 0, xwait = 0, xsignal = 0; };
    int stream[kSegments] = {};      // 0: the caller's stream, 1..3: side streams
    Marks enter[kSegments], at[kPoints];     // enter: `wait` / `xwait` of a segment's first launch; at: `signal` / `xsignal` of the last launch before the point, `xwait` of the first one after it
    bool points_first = false;       // the point branch (small launches) is planned ahead of the radar branch: it fills the window before the radar branch is released
    bool neck_on_side = false;       // dec_fork = 3 took effect: the neck runs on stream 2
    int radar_release = -1, detect_stream = 1;   // the effective "radar_start"; the stream the detection head ends on (decode + NMS of ach_forward_detect follow it there)
};
template <class Engine> Schedule make_schedule(const Engine& e) {
    Schedule s;
    constexpr auto bit = [](int event) { return static_cast<unsigned char>(1u << event); };
    // (PoolFormer is one in-order segment on the caller's stream like the other two and takes the MobileViT side of both decisions below: its stage outputs are fork-norm
    //  launches, not the preset block outputs the neck-on-stream-2 plan orders against; its direct write into the neck's concat buffers is the engine's business, not the schedule's.
    //  RepViT likewise: one in-order segment, the MobileViT side, maps 2 .. 4 announced as stages 0 .. 2)
    const bool edgenext = e.cfg.backbone == ACH_BACKBONE_EDGENEXT, pn2 = e.cfg.pc_seg == ACH_PCSEG_PN2 || e.cfg.pc_seg == ACH_PCSEG_PN2_MSG;
    const bool piped = e.pipeline && e.multi_stream && e.split_decoders == 0;      // the pipelined plan proper: the decoders leave the caller's stream together
    // radar release.  -2 (default) = stage 2 in the pipelined plan, else 1.  EdgeNeXt records it at stage `radar_start` exactly, so 4 and above record nothing and the plan fails in
    // interleave_streams ("unsatisfiable event order"; with streams = 0 too); MobileViT treats every value >= 2 as stage 2.  Recorded even when streams = 0 and nothing waits.
    const int rs = s.radar_release = e.radar_start == -2 ? ((e.pipeline && e.multi_stream) ? 2 : 1) : e.radar_start, stage = (!edgenext && rs >= 2) ? 2 : rs;
    if (stage >= 0 && stage <= 3) s.at[kPtStage0 + stage].signal = bit(kEvRadarRelease);
    s.points_first = rs >= 0 && e.multi_stream;
    // points: "point_stream2" = 3 a stream of their own; -1 (auto) = stream 2 for PointNet++ and for `pipeline && !head_stream`, where they share it with the decoders, else stream 1
    const bool point2 = e.point_on_head_stream < 0 ? (pn2 || (!e.head_stream && e.pipeline)) : e.point_on_head_stream != 0;
    s.stream[kSegPoints] = e.point_on_head_stream == 3 ? 3 : (point2 ? 2 : 1);
    s.stream[kSegRadar] = 1;
    if (s.points_first) s.enter[kSegRadar].wait = bit(kEvRadarRelease);
    s.enter[kSegRadar].xwait = bit(kXFusion);                      // the radar branch rewrites the radar pyramid the previous forward's fusion reads
    s.at[kPtRadarPyramid].signal = bit(kEvRadarPyramid);
    // the neck on stream 2 needs the stage outputs' launches to be identifiable (the preset concat slices of the EdgeNeXt plans) and the radar branch released before stage 3
    s.neck_on_side = piped && e.dec_fork == 3 && edgenext && rs < 3;
    // "dec_fork" (engine_options.h): the pipelined plan's decoders leave the caller's stream 0: behind the shared attention stage, 1: in front of it, 2: as soon as p3 exists (the residual
    // adds stay and run beside the attention stage), 3: with the whole neck, behind the backbone's last launch (which then records nothing else: the radar release came before stage 3)
    const int fork = s.neck_on_side ? 3 : (piped ? (e.dec_fork < 2 ? e.dec_fork : 2) : 0), neck = fork == 3 ? 2 : 0;
    s.stream[kSegNeck] = s.stream[kSegResidual] = neck;
    s.enter[kSegNeck].xwait = bit(kXFusion) | bit(kXDecoders);     // the neck rewrites what the previous forward's fusion and decoders read
    if (fork == 3) { s.at[kPtBackboneEnd].signal = s.enter[kSegNeck].wait = bit(kEvDecoderFork); s.at[kPtConcatSlice].xwait = s.at[kPtFpnOutputs].xsignal = bit(kXNeck); }   // (the residual adds are the neck's last reader of the backbone's maps)
    if (fork == 2) s.at[kPtP3].signal = s.enter[kSegAttention].wait = bit(kEvDecoderFork);
    s.at[kPtFpnOutputs].signal = bit(kEvFpnOutputs);
    if (fork == 1) s.enter[kSegAttention].wait = bit(kEvFpnOutputs);   // (the residual adds: the caller's last launch of this forward)
    s.stream[kSegAttention] = (fork == 1 || fork == 2) ? 2 : neck;
    // past the shared attention stage the two decoders are independent.  fork = 0 of the pipelined plan: both leave for stream 2 here.  "split_decoders" = 1: the semantic decoder on
    // stream 3; 2: the (shorter) water-line decoder joins side stream 1 behind the radar branch instead — no extra stream — and the semantic decoder keeps the caller's
    const bool fork0 = piped && fork == 0;
    if (fork0 || e.split_decoders != 0) s.at[kPtAttention].signal = bit(kEvDecoderFork);
    s.stream[kSegLaneDecoder] = e.split_decoders == 2 ? 1 : (fork0 ? 2 : s.stream[kSegAttention]);
    s.stream[kSegSeDecoder] = e.split_decoders == 1 ? 3 : (e.split_decoders == 2 ? 0 : s.stream[kSegLaneDecoder]);
    if (fork0 || e.split_decoders == 2) s.enter[kSegLaneDecoder].wait = bit(kEvDecoderFork);
    if (e.split_decoders == 1) s.enter[kSegSeDecoder].wait = bit(kEvDecoderFork);
    // cross-forward marks: the waits and fusion's signal are placed in plans that are not pipelined too (run_eager ignores them there), the decoders' signal only in the pipelined plan proper
    if (piped) s.at[kPtDecodersEnd].xsignal = bit(kXDecoders);     // the next forward's neck may rewrite the attention maps after the decoders' last launch
    s.at[kPtFusion].xsignal = bit(kXFusion);                       // last reader of the FPN outputs / radar pyramid (and, in stream order, after the decoders' reads)
    // fusion + head continue on the RADAR stream, gated only on the FPN outputs: they overlap with the decoders; "head_stream": on stream 2, gated on the FPN outputs and the radar pyramid
    s.stream[kSegDetect] = s.detect_stream = e.head_stream ? 2 : 1;
    s.enter[kSegDetect].wait = bit(kEvFpnOutputs) | (e.head_stream ? bit(kEvRadarPyramid) : 0);
    return s;
}
}  // namespace ach
