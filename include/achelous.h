/* achelous.h — C ABI of the MI355X-native Achelous forward engine (libachelous_hip.so).
 *
 * The reference (GuanRunwei/Achelous @ 2024-08-07) is 100 % Python: there is no FFI, plugin registry or native
 * operator table in it.  Its "operator API" for the hot path is one nn.Module and two free functions, and each
 * entry point below replaces exactly one of them (file:line relative to the reference tree):
 *
 *   ach_create / ach_destroy      <- nets/Achelous.py:26-47      Achelous.__init__ (ctor arguments -> ach_config)
 *   ach_load_weights              <- achelous.py:171             net.load_state_dict(torch.load(path))  (reference key names)
 *   ach_plan                      <- (implicit in eager PyTorch)  shape specialisation for one batch size
 *   ach_forward                   <- nets/Achelous.py:49-53      Achelous.forward(x, x_radar, x_point_clouds)
 *   ach_decode                    <- utils/utils_bbox.py:33-85   decode_outputs(outputs, input_shape)
 *   ach_nms                       <- utils/utils_bbox.py:87-132  non_max_suppression(...) up to the host-side un-letterbox
 *   ach_forward_detect            <- achelous.py:196-262         the three calls above as the reference's detect_image chains them
 *   ach_all_gather_records        <- achelous.py:176             nn.DataParallel's gather of the replicas' outputs (here: RCCL all-gather of detection records)
 *   ach_read_tap / ach_tap_*      <- (test hook) intermediate tensors at the SURVEY.md §8(a) boundaries
 *
 * Conventions: plain pointers and sizes only (no torch / HIP C++ types in the signatures; `stream` is a
 * hipStream_t passed as void*).  Every function returns 0 on success and a negative code on failure and never
 * throws; ach_last_error() returns a message for the most recent failure on that handle (or a global one when the
 * handle itself could not be created).  The caller owns inputs and outputs (device pointers, dtype = config dtype,
 * layouts exactly those of the reference: NCHW images / maps, [B, C, N] point clouds, [B, N, classes] point
 * log-probabilities).  The engine owns its packed weights and activation arena (allocated in ach_load_weights /
 * ach_plan; nothing is allocated inside ach_forward, which is asynchronous on `stream` and performs no host sync).
 * One handle per (device, stream); calls on one handle must not overlap.
 */
#ifndef ACHELOUS_H_
#define ACHELOUS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ach_handle ach_handle;

enum { ACH_DTYPE_F32 = 0, ACH_DTYPE_BF16 = 1,
       ACH_DTYPE_F16 = 2    /* fp16 activations and MFMA operands, fp32 accumulation: the type the reference's mixed-precision mode computes in
                             * (utils/utils_fit.py:120-121, train.py:37 --fp16).  Inputs / outputs are fp16, or bf16 with option "io_bf16" */ };
enum { ACH_BACKBONE_EDGENEXT = 0, ACH_BACKBONE_MOBILEVIT = 1, ACH_BACKBONE_POOLFORMER = 2,
       ACH_BACKBONE_REPVIT = 4 /* 3 is reserved (the reference's default 'ef') and refused */ };
enum { ACH_PHI_S0 = 0, ACH_PHI_S1 = 1, ACH_PHI_S2 = 2 };

enum {
    ACH_OK = 0,
    ACH_ERR_INVALID = -1,       /* bad argument / shape / state */
    ACH_ERR_UNSUPPORTED = -2,   /* configuration outside the built scope (mirrors NotImplementedError) */
    ACH_ERR_MISSING_KEY = -3,   /* state-dict key absent or of the wrong shape */
    ACH_ERR_DEVICE = -4,        /* HIP runtime error */
    ACH_ERR_NOMEM = -5
};

enum { ACH_NECK_GDF = 0, ACH_NECK_CDF = 1 };     /* Ghost-Dual-FPN (neck/ghostdualfpn.py) / CSP-Dual-FPN (neck/cspdualfpn.py) */
/* point-cloud branch: PointNet (nets/pointcloudseg/pointnet2/pointnet_sem_seg.py) / PointNet++.  The reference snapshot has no
 * PointNet++ code (nets/Achelous.py:31-32 builds only 'pn'): ACH_PCSEG_PN2 runs OUR OWN specification of that branch
 * (state-dict keys pc_seg_model.sa{1-4} / fp{4-1} / conv1 / bn1 / conv2); num_points must be a multiple
 * of 128 and at most 1024. */
enum { ACH_PCSEG_PN = 0, ACH_PCSEG_PN2 = 1,
       ACH_PCSEG_NONE = 2,  /* nets/Achelous.py:56-76 (Achelous3T): no point-cloud stream; `points` / `pc_seg` arguments are ignored (may be NULL) */
       ACH_PCSEG_PN2_MSG = 3 /* round 6: the MULTI-scale-grouping PointNet++ (spec.py::PN2_MSG: two radii and two shared-MLP stacks per level, keys sa{k}.conv_blocks.<scale>.<layer>):
                                the variant the reference's only PointNet++ datum (README.md:81,83: ~2.0 M parameters) points at; own specification, parity unpinned */ };

typedef struct ach_config {
    int32_t num_det;        /* detection classes           (Achelous.__init__ num_det)      */
    int32_t num_seg;        /* semantic classes            (num_seg)                        */
    int32_t phi;            /* ACH_PHI_*                   (phi)                            */
    int32_t backbone;       /* ACH_BACKBONE_*              (backbone in {'en','mv','pf','rv'}) */
    int32_t resolution;     /* square input size           (resolution)                     */
    int32_t pc_channels;    /* point features              (pc_channels)                    */
    int32_t pc_classes;     /* point classes               (pc_classes)                     */
    int32_t num_points;     /* points per cloud N                                           */
    int32_t nano_head;      /* 1: 64-channel head          (nano_head)                      */
    int32_t spp;            /* 1: SPP, 0: SPPF             (spp)                            */
    int32_t dtype;          /* ACH_DTYPE_*: storage type of activations, inputs and outputs */
    int32_t neck;           /* ACH_NECK_*                  (neck in {'gdf','cdf'})           */
    int32_t pc_seg;         /* ACH_PCSEG_*                 (pc_seg in {'pn','pn2'}; NONE = Achelous3T) */
} ach_config;

/* one entry of a reference-keyed state_dict; `data` is HOST memory, fp32, contiguous, reference shape */
typedef struct ach_tensor_desc {
    const char* name;
    const float* data;
    int32_t ndim;
    int64_t shape[4];
} ach_tensor_desc;

int ach_create(const ach_config* cfg, ach_handle** out);
void ach_destroy(ach_handle* h);
const char* ach_last_error(const ach_handle* h);

/* Copies the weights to the host side of the handle.  Folding (eval-mode BatchNorm, LayerNorm affine, layer scale, constant positional
 * encoding) and repacking into kernel-native layouts on the device happen in ach_plan, which must follow: loading drops the handle's plan,
 * and ach_forward returns ACH_ERR_INVALID until ach_plan has run again.  Integer buffers (num_batches_tracked) may be omitted. */
int ach_load_weights(ach_handle* h, const ach_tensor_desc* tensors, size_t n);

/* Options, set before ach_plan: a successful ach_set_option drops the handle's plan (ach_forward returns ACH_ERR_INVALID until ach_plan has run again; ach_join and
 * ach_forwards_in_flight keep working).  The value is normalised as stated per key and stored; ach_get_option returns the stored value (reads the handle only; a failure still
 * sets its ach_last_error), ach_option_key(i) enumerates the keys in the order below (NULL past the end).  An unknown key is ACH_ERR_INVALID.  One line per key: values, default,
 * what it selects.  The table itself, with the measurement behind every default, is achelous_amd/csrc/engine_options.h; DESIGN.md §4 and profiles/NOTES_r0*.md have the rest.
 * "16-bit engines" = ACH_DTYPE_BF16 / ACH_DTYPE_F16.
 * The plan and its schedule
 *   "full_taps"         0 / 1, default 0: also write to HBM the SURVEY §8(a) boundaries that production plans keep on-chip (the 32-channel full-resolution decoder tensors), so that parity tests can read them back
 *   "streams"           0 / 1, default 1: the independent radar and point branches run on two engine-owned side streams, forked from / joined into the caller's stream with events; 0: everything on the caller's stream
 *   "graph"             0 / 1, default 0: capture the plan into a hipGraph per distinct set of I/O pointers and replay it (measured no faster than the interleaved eager launches on the side streams)
 *   "io_bf16"           0 / 1, default 0 (round 4): ACH_DTYPE_F16 only, else ACH_ERR_INVALID — the caller's input / output tensors are bf16, converted in the first / last kernels
 *   "pipeline"          0 / 1, default 0: consecutive forwards overlap (see ach_join)
 *   "dec_fork"          0..3 (clamped), default 1 (round 5): pipelined plan, where the segmentation decoders leave the caller's stream — 1: in front of the shared ShuffleAttention stage (+0.9 %), 0: behind it (round 3), 2: as soon as the neck's p3 exists, 3: the whole neck on stream 2, ordered against the next forward's backbone by a third cross-forward event (EdgeNeXt plans; level with 1); bit-identical
 *   "radar_start"       integer, default -2: the radar branch is released after backbone stage k = 0..3, -1 = at once; -2 = stage 2 in the pipelined plan, stage 1 in the plain plan
 *   "head_stream"       0 / 1, default 0: 1 = radar + point branches share low-priority stream 1, fusion + head + NMS run on stream 2 at the caller's priority; 0: they queue behind the radar branch on stream 1
 *   "side_priority"     bit mask, default 3: with head_stream = 0, the side streams created at the lowest stream priority
 *   "point_stream2"     -1 / 0 / 1 / 3, default -1: the point branch opens stream 2 ahead of fusion + head (-1 auto = PointNet++ only); 3 (round 5) = a stream of its own — the process's fourth: measured -1 %, and it leaves no stream for a collective
 *   "split_decoders"    integer, default 0: semantic decoder on its own stream (measured slower)
 * Kernel selection, kept so that each fused kernel can be A/B-measured against the layer-wise path it replaced (results agree to rounding, or bit for bit where stated)
 *   "fused_mlp"         0 / 1, default 1: EdgeNeXt blocks and decoder conv pairs through k_mlp.h
 *   "mlp_split"         -1 / 0 / 1, default -1 (auto): four waves per pixel tile in k_mlp.h
 *   "mlp_split_hw"      integer, default 1024: maps of at most this many pixels run the fused blocks with four waves per 16-pixel tile
 *   "mlp_band"          0 / 1 / 2, default 1 (round 3, 16-bit engines): EdgeNeXt blocks of the instantiated shapes — d = 96 / 144 on maps up to 20 wide, d = 176 up to 10 wide — as the band kernel, 2: also stages 0 / 1, 0: never
 *   "band_rows_s3"      integer, default 0 (= 5): rows per band of the stage-3 band kernel
 *   "dw_even"           0 / 1, default 1: even deal of depthwise tap rows over the four SPLIT waves, d = 144
 *   "dw_tile"           0 / 1, default 1: LDS-tiled depthwise kernel on 10x10 maps
 *   "ds_fuse"           0 / 1, default 1 (round 4): the channels-first LayerNorm of a downsample layer inside its 2x2 / stride-2 conv
 *   "sdta_fuse"         0 / 1 / 2, default 1 (round 3, 16-bit engines): an SDTA encoder's conv cascade + tail copy + positional encoding as one launch on maps up to 20 x 20, 2: every map, 0: never; bit-identical
 *   "xca_mfma"          0 / 1, default 1: XCA Gram matrices on the matrix cores; 0: VALU kernel
 *   "xca_fold_mfma"     0 / 1, default 1 (round 6, 16-bit engines): the XCA finalize launch folds softmax(attn) into the projection weights on the matrix cores, one workgroup per (frame, head); 0: round 5's fp32 VALU fold
 *   "stem_mfma"         0 / 1, default 1: the 4x4/s4 stem conv as an MFMA GEMM gathered from the NCHW image; 0: scalar-FMA kernel
 *   "mv_stem"           0 / 1, default 1 (round 4, 16-bit engines): MobileViT's conv1 gathered straight from the NCHW image instead of an NHWC copy + implicit GEMM
 *   "fused_mv2"         0 / 1, default 1: MobileViT's MV2 blocks (1x1 -> dw3x3 -> 1x1) as one launch (k_mv2.h)
 *   "attn_mfma"         0 / 1, default 1: MobileViT attention scores / P.V on MFMA (k_mvit.h) instead of one query per thread
 *   "ffn_rows2"         0 / 1, default 1 (round 5, 16-bit engines): MobileViT's feed-forward layers on the large maps with two 16-row tiles per wave; bit-identical
 *   "gemm_blocks"       integer, default 0 (= 1024): workgroups a GEMM launch aims for when its rows alone cannot fill the chip
 *   "row_conv"          0 / 1, default 1: offset/modulator convs through k_conv3.h
 *   "fused_rc"          0 / 1, default 1: RCBlock conv + deformable sampling + contraction as one kernel
 *   "pool_strip"        integer, default 2: which RCBlock average pools use the 4-pixel strip kernel
 *   "radar_skip"        0 / 1, default 1: closed-form shortcut for empty 16-pixel segments of the first RCBlock, bit-identical
 *   "radar_rows4"       0 / 1 / 2, default 2: a workgroup owns four rows in the first / in all fused RCBlocks and the row-walking conv
 *   "radar_compact"     0 / 1, default 1 (round 3, 16-bit engines): first RCBlock — per-pixel activity, active pixels compacted into dense tiles; bit-identical
 *   "radar_direct"      0 / 1, default 1 (round 4, 16-bit engines): the first RCBlock pools and adds its residual straight from the NCHW radar map; bit-identical
 *   "radar_bg"          0 / 1, default 1 (round 6, 16-bit engines): the first RCBlock's output map keeps relu(bias) at every unoccupied pixel; rc_front neither reads nor writes such pixels; bit-identical, carries masks from one forward to the next inside the plan's arena
 *   "radar_pool_sparse" 0 / 1, default 1 (round 6, 16-bit engines): the first RCBlock's pool stores a pixel only where the pooled map is, or was after the previous forward, non-zero; bit-identical, carries masks from one forward to the next inside the plan's arena
 *   "ghost_fuse"        0 / 1, default 1 (round 4): the neck's Ghost bottlenecks, shortcuts, Upsample modules and the SPP block as band kernels — k_ghost.h; bit-identical
 *   "ghost_rb"          positive (else the default), default 5: rows per band of those kernels
 *   "spp_split"         integer, default 0 (auto: 2): workgroups per frame of the fused SPP launch
 *   "level_chain"       0 / 1, default 1 (round 3, 16-bit engines): a decoder level's kernel also applies the next level's low-resolution conv pair; bit-identical
 *   "head_rows"         0 / 1 / 2, default 2 (round 3, 16-bit engines): last decoder level + segmentation head as the row-walking two-columns-per-lane kernel, 1: one column, 0: the LDS tile kernel
 *   "head_band"         positive (else the default), default 40: rows per workgroup band of that kernel
 *   "csp_fuse"          0..2 (clamped), default 2 (round 5, 16-bit engines): CSP-Dual-FPN decoders — 2: the two 32-channel levels (160 x 160 and full resolution) as row-walking launches (k_csphead.h), the last one with the segmentation head in it; 1: the last level + head only; 0: layer-wise
 *   "csp_band"          positive (else the default), default 40: rows per band of those launches
 *   "head_batch"        0 / 1, default 1: detection-head layers batched over the levels
 *   "head_fuse"         0 / 1, default 1 (round 3, 16-bit engines): a detection-head layer's depthwise + pointwise convs of both towers and all levels as one launch
 *   "pc_chain"          0 / 1, default 1 (round 4): PointNet's conv3 + conv4 as one two-layer chain launch
 *   "pn2_fps_all"       0 / 1, default 1 (round 4): PointNet++'s four farthest-point samplings as one launch
 *   "group_wpc"         >= 0 (negative = 0 = never), default 4096 (round 5): PointNet++ grouping with a workgroup per centroid on levels with at most this many centroids; bit-identical
 *   "group_max"         >= 0 (negative = 0 = never), default 1024 (round 5): PointNet++'s shared-MLP + max-over-the-ball layers with a wave per ball for layers of at least this many balls; bit-identical
 * Measured slower or level, kept
 *   "gemm_rows"         1 / 2 / 4 (anything else = 1), default 1: 16-row sub-tiles per wave for GEMMs with K >= 1024 — 2 / 4 measured slower
 *   "xca_frame"         0 / 1 / 2, default 0 (round 6, 16-bit engines): four launches per attention; 2: two launches — qkv + Gram partials per token slice, softmax + fold + projection per 64 tokens; 1: one launch with a workgroup per frame; both measured slower, DESIGN.md 4.5
 *   "xca_slice"         integer, default 0 (64, 128 on maps of 1024 tokens or more): with xca_frame, tokens per workgroup of the front kernel
 *   "xca_front_waves"   4 / 8 / 16, default 0 (by the number of work units): with xca_frame, waves per workgroup of the front kernel
 *   "xca_back_waves"    4 / 8 / 16, default 0 (by the number of work units): with xca_frame, waves per workgroup of the back kernel
 * Debugging only
 *   "xwait2_op"         launch index, default -1 (none): pipelined mode, the launch that waits for the previous forward's decoders instead of the planned one */
int ach_set_option(ach_handle* h, const char* key, int32_t value);
int ach_get_option(const ach_handle* h, const char* key, int32_t* value);
const char* ach_option_key(int32_t index);

/* Builds the launch plan and the activation arena for batch size B (re-plan to change B). */
int ach_plan(ach_handle* h, int32_t batch);
size_t ach_arena_bytes(const ach_handle* h);

/* image [B,3,R,R], radar [B,3,R,R], points [B,pc_channels,N]  ->
 * det3 [B,5+num_det,R/8,R/8], det4 [..,R/16,R/16], det5 [..,R/32,R/32], se_seg [B,num_seg,R,R],
 * lane_seg [B,2,R,R], pc_seg [B,N,pc_classes] (log-probabilities).  All device pointers of the config dtype. */
int ach_forward(ach_handle* h, const void* image, const void* radar, const void* points,
                void* det3, void* det4, void* det5, void* se_seg, void* lane_seg, void* pc_seg, void* stream);

/* ach_forward + ach_decode + ach_nms in one call (achelous.py:246-262 runs net -> decode_outputs -> non_max_suppression back to
 * back).  Same outputs as the three separate calls, bit for bit; the difference is scheduling: decode and NMS are enqueued on the
 * engine's detection-branch stream right behind the detection head, so they overlap with the segmentation decoders instead of
 * running alone at the end of the step.  `decoded` [B,A,5+num_det] fp32 and `workspace` (>= ach_nms_workspace_bytes) are scratch
 * owned by the caller. */
int ach_forward_detect(ach_handle* h, const void* image, const void* radar, const void* points,
                       void* det3, void* det4, void* det5, void* se_seg, void* lane_seg, void* pc_seg,
                       float* decoded, float conf_thres, float nms_thres, int32_t max_det,
                       float* out_rows, int32_t* out_idx, int32_t* out_count, void* workspace, void* stream);

/* Pipelined serving (ach_set_option(h, "pipeline", 1) before ach_plan): ach_forward / ach_forward_detect return with the work of
 * the engine's side streams NOT yet joined into `stream`, so that the caller can enqueue the next forward first; ach_join makes
 * `stream` wait for the oldest un-joined forward (its outputs are complete in stream order after that).  At most two forwards may
 * be un-joined (a third call joins the oldest itself); inputs, outputs and the detect workspace of a forward must stay allocated
 * and untouched until it has been joined.  Results are bit-identical to the plain mode.  The reference's counterpart is the
 * python loop around `net(...)` in achelous.py:246-262 / utils/callbacks.py:184, which serialises frames. */
int ach_join(ach_handle* h, void* stream);
int ach_forwards_in_flight(const ach_handle* h);

/* det maps (config dtype) -> decoded [B, A, 5+num_det] fp32, A = (R/8)^2 + (R/16)^2 + (R/32)^2 */
int ach_decode(ach_handle* h, int32_t batch, const void* det3, const void* det4, const void* det5,
               float* decoded, void* stream);

/* decoded [B,A,5+num_det] fp32 -> per image: rows [max_det,7] = x1,y1,x2,y2,obj,cls_conf,cls_id (normalised
 * corners), kept anchor indices [max_det] (descending score), count.  Every slot of the outputs is written: slots past `count`
 * get zero rows and index -1 (the caller need not clear them).  `workspace` >= ach_nms_workspace_bytes().
 * Any planned resolution works: up to 4096 anchors per image (416 x 416) one launch, above it two (up to 15309 anchors, 864 x 864), which also follow
 * torchvision's switch to per-class suppression when more than 5000 candidates pass the filter.  A handle whose resolution gives more than 15309 anchors
 * gets ACH_ERR_UNSUPPORTED before any launch.  The same holds for ach_forward_detect. */
size_t ach_nms_workspace_bytes(const ach_handle* h, int32_t batch);
int ach_nms(ach_handle* h, int32_t batch, const float* decoded, float conf_thres, float nms_thres, int32_t max_det,
            float* out_rows, int32_t* out_idx, int32_t* out_count, void* workspace, void* stream);

/* Multi-GPU (the reference's nn.DataParallel gather, achelous.py:176): frames shard by contiguous batch slices with NO data-path
 * collective; the one exchange step is an all-gather of the shards' fixed-size detection records.  A shard's record is ONE flat int32 buffer of
 * ach_record_words(batch, max_det) words, planar: rows [batch, max_det, 7] (fp32 bits) | kept anchor indices [batch, max_det] | counts [batch] — pass
 * pointers into it as out_rows / out_idx / out_count of ach_nms / ach_forward_detect (the kernel fills every slot).  ach_all_gather_records enqueues
 * ncclAllGather(send, recv, words, ncclInt32, comm, stream): `comm` is an ncclComm_t the caller created with RCCL (one rank per GPU), recv_records holds
 * world x words.  RCCL is dlopen'ed at first use (librccl.so, or $ACH_RCCL_LIBRARY); the library does not link against it. */
size_t ach_record_words(int32_t batch, int32_t max_det);
int ach_all_gather_records(ach_handle* h, void* nccl_comm, const int32_t* send_record, int32_t* recv_records, int32_t batch, int32_t max_det, void* stream);

/* Pre / post-processing either side of the forward (the reference does these per frame on the host):
 *   ach_preprocess_radar  <- utils/utils.py:51-54   preprocess_input_radar: (x - min) / (max - min) + 1e-13, min/max per frame;
 *                                                   in fp32 [B,C,R,R] -> out [B,C,R,R] (config dtype)
 *   ach_normalize_points  <- achelous.py:240-243    sklearn normalize(X[N,D], axis=0) + permute; in fp32 [B,N,D] -> out [B,D,N]
 *   ach_preprocess_image  <- utils/utils.py:44-48   preprocess_input + HWC->CHW (achelous.py:205); in uint8 [B,R,R,3] (already
 *                                                   letterboxed) -> out [B,3,R,R]
 *   ach_seg_argmax        <- achelous.py:283-318    per-pixel class at network resolution; in [B,C,R,R] -> out uint8 [B,R,R] */
int ach_preprocess_radar(ach_handle* h, int32_t batch, int32_t channels, const float* in, void* out, void* stream);
int ach_normalize_points(ach_handle* h, int32_t batch, int32_t n, int32_t d, const float* in, void* out, void* stream);
int ach_preprocess_image(ach_handle* h, int32_t batch, const uint8_t* in, void* out, void* stream);
int ach_seg_argmax(ach_handle* h, int32_t batch, int32_t channels, const void* seg, uint8_t* out, void* stream);
/*   ach_seg_resize_argmax <- achelous.py:283-318    the class map at the ORIGINAL image size as detect_image produces it: softmax ->
 *                                                   crop the letterbox bars (utils_seg/utils.py:19-31) -> cv2.resize INTER_LINEAR ->
 *                                                   argmax; seg [B,C,R,R] (config dtype) -> out uint8 [B,out_h,out_w];
 *                                                   prob_workspace: batch * channels * R * R floats
 *   ach_correct_boxes     <- utils_bbox.py:5-30,177-180  kept rows (normalised x1,y1,x2,y2 in the network input) -> (y1,x1,y2,x2) in pixels
 *                                                   of the original image (letterbox undone), rows past count[b] zeroed; fp64 as numpy */
int ach_seg_resize_argmax(ach_handle* h, int32_t batch, int32_t channels, const void* seg, int32_t out_h, int32_t out_w,
                          float* prob_workspace, uint8_t* out, void* stream);
int ach_correct_boxes(ach_handle* h, int32_t batch, int32_t max_det, const float* rows, const int32_t* count, int32_t image_h, int32_t image_w,
                      int32_t letterbox, float* out_rows, void* stream);

/* The same two steps for a RAGGED batch — frames of different sizes in one call, a fixed number of launches whatever the batch (achelous_amd/csrc/k_serve.h):
 *   ach_seg_overlay_frames  <- achelous.py:283-345  both heads' class maps at every frame's own size (the arithmetic of ach_seg_resize_argmax, operation for
 *                       operation) and the overlay image detect_image draws: palette lookup, Image.blend twice, ImageEnhance.Brightness.  Two softmax launches
 *                       and ONE launch for all frames, both heads and all outputs.  se_seg [B, channels, R, R], lane_seg [B, 2, R, R] (config dtype);
 *                       prob_se / prob_line: batch * channels * R * R and batch * 2 * R * R floats.  Each output is optional (null: skipped, and a head no
 *                       wanted output needs is not read): out_semantic / out_waterline uint8 class maps (the arg-max itself, not remapped), out_overlay uint8
 *                       HWC.  The original images sit in `arena`, a packed uint8 buffer (HWC, 16-byte aligned, `arena_bytes` a multiple of 16; needed for the
 *                       overlay only).  Every output is a packed arena of its own: 16-byte aligned, frame starts and row pitches multiples of 16.
 *                       Frame table int64 [batch][16], host copy and device copy: 0 byte offset of the image in `arena`, 1 H, 2 W, 3 image pitch (>= 3 W),
 *                       4 y0, 5 x0, 6 nh, 7 nw (the window of the R x R network map that is stretched over the frame: the letterbox's, utils_seg/utils.py:19-31,
 *                       or any other inside the map), 8 byte offset of the semantic map in out_semantic, 9 of the water-line map in out_waterline, 10 pitch of
 *                       both maps (>= W), 11 byte offset of the overlay in out_overlay, 12 overlay pitch (>= 3 W), 13-15 unused.
 *                       Constants, 2304 bytes, host copy and device copy (overlay only): semantic palette [256][3], water-line palette [256][3], semantic class
 *                       remap [256], water-line class remap [256], brightness table [256] (read when use_lut != 0):
 *                       overlay = table[blend(blend(image, palette_se[remap_se[class]], blend_se), palette_line[remap_line[line class]], blend_line)],
 *                       blend(a, b, t) = (uint8)(a + t * (b - a)) in float32 as PIL's Image.blend, 0 <= t <= 1.  palette_*_len: colours the caller filled.
 *                       The host copies are checked before anything is launched: an extent past an arena, a bad pitch or alignment, H or W < 1, a window
 *                       outside the map, a remapped class past its palette -> ACH_ERR_INVALID, no launch.  More than 30 semantic classes: ACH_ERR_UNSUPPORTED.
 *   ach_correct_boxes_frames  ach_correct_boxes with every frame's (image_h, image_w) read from an int32 [batch][2] table (host copy checked, device copy read). */
int ach_seg_overlay_frames(ach_handle* h, int32_t batch, int32_t channels, const void* se_seg, const void* lane_seg, float* prob_se, float* prob_line,
                           const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const uint8_t* consts_host,
                           const uint8_t* consts_dev, int32_t palette_se_len, int32_t palette_line_len, float blend_se, float blend_line, int32_t use_lut,
                           uint8_t* out_semantic, int64_t semantic_bytes, uint8_t* out_waterline, int64_t waterline_bytes, uint8_t* out_overlay,
                           int64_t overlay_bytes, void* stream);
int ach_correct_boxes_frames(ach_handle* h, int32_t batch, int32_t max_det, const float* rows, const int32_t* count, const int32_t* shapes_host,
                             const int32_t* shapes_dev, int32_t letterbox, float* out_rows, void* stream);

/* The drawing detect_image ends with (achelous.py:363-433) for a ragged batch, IN PLACE, in two launches whatever the batch (achelous_amd/csrc/k_draw.h): per
 * kept detection, in the order of boxes[b, :count[b]], `thickness` one-pixel rings of the box in the class colour, the filled label plate and the label text
 * '{name} {obj * cls:.2f}' — byte for byte what PIL's ImageDraw.rectangle / ImageDraw.text leave.  Stateless (no handle).
 *   arena        packed HWC uint8 frames (4-byte aligned), e.g. the overlay arena of ach_seg_overlay_frames.
 *   frame table  int64 [batch][8], host copy and device copy: 0 byte offset of the frame (a multiple of 4), 1 H, 2 W, 3 pitch (>= 3 W, a multiple of 4),
 *                4 ring thickness (1..64), 5 first entry of the frame's font size in the label table, 6-7 unused.
 *   boxes, count device [batch, max_det, 7] = (y1, x1, y2, x2 in the frame's pixels, obj, class conf, class id) and int32 [batch], as ach_correct_boxes_frames
 *                leaves them.  A row is skipped if its class is flagged in `style`, its id is outside [0, num_classes) or one of its six floats is not finite;
 *                count is clamped to max_det (1..1024) and coordinates are clamped on the device.
 *   label table  int32 [num_labels][7], host and device copy; entry base + class * 101 + hundredths: 0 byte offset of the glyph mask (8-bit coverage, w * h
 *                bytes) in `blob_dev`, 1 mask w, 2 mask h, 3 ox, 4 oy (mask position relative to the text origin), 5 label w, 6 label h.
 *   style_dev    uint8 [1028]: class colours [256][3], skip flag per class [256], ink [3], pad.
 *   records      workspace, int32 [batch * max_det * 16], 16-byte aligned.  class_counts: optional int32 [batch, num_classes], the kept rows per class id.
 * The host copies are checked before anything is launched: a frame past the arena, a bad pitch or alignment, thickness outside 1..64, num_classes outside
 * 1..256, a label mask past the blob, an atlas base past the label table -> ACH_ERR_INVALID, no launch. */
int ach_draw_detections_frames(uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, int32_t batch, const float* boxes,
                               const int32_t* count, int32_t max_det, int32_t num_classes, const int32_t* labels_host, const int32_t* labels_dev, int64_t num_labels,
                               const uint8_t* blob_dev, int64_t blob_bytes, const uint8_t* style_dev, int32_t* records, int32_t* class_counts, void* stream);

/* Range guard of the fp16-storage engine (ACH_DTYPE_F16).  The reference runs fp32 or, under autocast, fp16 WITH torch's GradScaler / inf checks
 * (utils/utils_fit.py:120-166); bf16 callers (BASELINE configs[1]) are served by fp16 storage inside, which overflows at 65504 where bf16 does not.
 * Every kernel of that engine therefore runs with MODE.FP16_OVFL (overflowing conversions clamp to +-65504, never infinity), and this entry counts the
 * elements of the plan's activation tensors that are saturated or non-finite after the forward(s) enqueued on `stream` so far (it synchronises the
 * stream; ~1 ms at batch 64).  0 = the forward stayed inside the fp16 range.  Always 0 for the fp32 / bf16 engines.  The Python module checks a
 * model's first forward with it and falls back to bf16 storage when it is not 0 (achelous_amd/nets.py, `f16_guard`). */
int ach_count_saturated(ach_handle* h, void* stream, uint64_t* count);

/* test hooks: intermediate tensors of the last ach_forward, converted to fp32 NCHW (or [rows, C]) on the host */
int ach_tap_count(const ach_handle* h);
const char* ach_tap_name(const ach_handle* h, int i);
int ach_tap_shape(const ach_handle* h, const char* name, int64_t shape[4], int32_t* ndim);
int ach_read_tap(ach_handle* h, const char* name, float* host_out, size_t capacity_elems);

/* measurement hooks (bench.py): the plan's launch list with the ALGORITHMIC bytes / flops of each launch, a pass
 * that brackets every launch with HIP events, and a live probe that brackets ONE launch on every ach_forward. */
int ach_plan_launches(const ach_handle* h);
const char* ach_op_name(const ach_handle* h, int i);
double ach_op_bytes(const ach_handle* h, int i);          /* inputs read once + outputs written once + weights, REAL channel counts */
double ach_op_layout_bytes(const ach_handle* h, int i);   /* the same over the stored pixel pitches (channel padding included) */
double ach_op_flops(const ach_handle* h, int i);          /* 2 x MACs of the dense contractions of the launch */
int ach_op_stream(const ach_handle* h, int i);            /* 0: caller's stream, 1..: engine side streams */
/* read-only look at the plan's schedule: the events launch `i` waits for before it starts and records once it is enqueued, as bit masks.  `wait` / `signal`: the
 * joins inside one forward (bit 0 radar release, 1 FPN outputs, 2 decoder fork, 3 radar pyramid); `xwait` / `xsignal`: the cross-forward marks of the pipelined plan
 * (bit 0 fusion's reads, 1 the decoders' reads, 2 the neck's reads; placed in every plan, honoured only under option "pipeline").  A launch outside the plan:
 * ACH_ERR_INVALID.  tests/golden/plan_schedules.json pins these for a set of plans. */
int ach_op_sync(const ach_handle* h, int i, int* wait, int* signal, int* xwait, int* xsignal);
int ach_forward_profiled(ach_handle* h, const void* image, const void* radar, const void* points,
                         void* det3, void* det4, void* det5, void* se_seg, void* lane_seg, void* pc_seg, void* stream,
                         float* op_ms, size_t capacity);
int ach_set_probe(ach_handle* h, int op_index);          /* -1 disables */
/* micro-benchmark of the MFMA GEMM kernel alone on scratch buffers: ms per launch of Y[M,N] = epi(X[M,K] W^T) */
int ach_bench_gemm(ach_handle* h, int M, int K, int N, int act, int ln, int residual, int P, int iters, void* stream, float* ms);
int ach_read_probe(ach_handle* h, float* avg_ms, int* samples);
/* second probe form: events before launch `first` and after launch `last` of the plan (both on the same stream: a run of the
 * caller's stream such as the neck + decoder sub-path), slot 0, 1 or 2 (ach_set_probe uses slot 0); first = -1 disables */
int ach_set_probe_range(ach_handle* h, int slot, int first, int last);
int ach_read_probe_slot(ach_handle* h, int slot, float* avg_ms, int* samples);

/* ---- training mode, first block (utils/utils_fit.py:37-166 trains through ATen autograd).
 * Stateless fp32 kernels (no handle; errors through ach_last_error(NULL)) for the PointNet shared-MLP layer
 * relu(BatchNorm1d(Conv1d_k1(x))) on [B, C, N] tensors in TRAINING mode — batch statistics — forward and backward:
 *   ach_train_gemm         C[b] (+)= op(A[b]) op(B[b]) [+ bias per row]: row-major, leading dimensions and batch strides in elements,
 *                          trans_x = the stored matrix is the transpose; reduce_batch sums the products over the batch into ONE C
 *   ach_train_bn_stats     mean / biased variance per channel over (B, N)
 *   ach_train_bn_relu_fwd  y = [relu](gamma * (z - mean) / sqrt(var + eps) + beta)
 *   ach_train_bn_relu_bwd  dgamma, dbeta and dz from dy (z, y, mean, var of the forward) */
int ach_train_gemm(const float* A, const float* B, float* C, const float* bias, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                   int64_t stride_a, int64_t stride_b, int64_t stride_c, int32_t trans_a, int32_t trans_b, int32_t batch, int32_t reduce_batch,
                   int32_t accumulate, void* stream);
/*   ach_train_set_gemm_precision   element type of ach_train_gemm's matrix-instruction operands, process-wide: 0 = fp32 (default; the arithmetic the
 *                          float64 reference-step test holds to 5e-3), 1 = the fp32 operands are rounded to bf16 while they are staged into LDS, products
 *                          accumulated in fp32, fp32 output (the reference's default loop runs under torch.cuda.amp.autocast, utils/utils_fit.py:120-166,
 *                          train.py:37 `fp16 = True`; achelous_amd.Achelous.train_precision = 'bf16' selects it).  Every other training kernel stays fp32.
 *                          Measured no faster on this network (its training GEMMs are HBM-bound streams of fp32 activations): opt-in.
 *                          Returns ACH_ERR_INVALID for another value; ach_train_get_gemm_precision returns the current one. */
int ach_train_set_gemm_precision(int32_t precision);
int ach_train_get_gemm_precision(void);
/*   ach_train_gemm_p       ach_train_gemm with the operand type of THIS call (0 / 1 as above; -1 = the process-wide setting): an autograd node records the type its
 *                          forward ran with and passes it to its backward launches, so two modules (or threads) with different `train_precision` never run a backward
 *                          with the other's choice */
int ach_train_gemm_p(const float* A, const float* B, float* C, const float* bias, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                     int64_t stride_a, int64_t stride_b, int64_t stride_c, int32_t trans_a, int32_t trans_b, int32_t batch, int32_t reduce_batch,
                     int32_t accumulate, int32_t precision, void* stream);
int ach_train_bn_stats(const float* z, float* mean, float* var, int32_t B, int32_t C, int32_t N, void* stream);
/*   ach_train_bn_running    nn.BatchNorm's running estimates after a training forward: running <- (1 - momentum) running + momentum batch; `unbias` = M / (M - 1) on the variance */
int ach_train_bn_running(const float* mean, const float* var, float* running_mean, float* running_var, int32_t C, float momentum, float unbias, void* stream);
int ach_train_bn_relu_fwd(const float* z, const float* mean, const float* var, const float* gamma, const float* beta, float* y, int32_t B, int32_t C,
                          int32_t N, float eps, int32_t relu, void* stream);
int ach_train_bn_relu_bwd(const float* z, const float* y, const float* dy, const float* mean, const float* var, const float* gamma, float* dgamma,
                          float* dbeta, float* dz, int32_t B, int32_t C, int32_t N, float eps, int32_t relu, void* stream);
/*   ach_train_max_points   max over the N points of rows = B*C rows with the arg-max (dy == NULL: forward x -> y, idx; else backward dy, idx -> dx)
 *   ach_train_log_softmax  log-softmax over the classes of z [B,K,N] written as [B,N,K] (dy == NULL: forward; else y, dy -> dz [B,K,N])
 *                          (pointnet_utils.py:32,127; pointnet_sem_seg.py:34-37) */
int ach_train_max_points(const float* x, float* y, int32_t* idx, const float* dy, float* dx, int64_t rows, int32_t N, void* stream);
int ach_train_log_softmax(const float* z, float* y, const float* dy, float* dz, int32_t B, int32_t K, int32_t N, void* stream);

/* One pass of Pillow's 8-bit ImagingResample (the reference letterboxes its input with PIL BICUBIC, utils/utils.py:20-33): integer dot products
 * with 22-bit fixed-point coefficients computed on the host exactly as Resample.c does (achelous_amd/prepost.py).  HWC uint8 images; a resize
 * is a horizontal pass into an 8-bit intermediate and a vertical pass (dst_pitch lets it write into the letterbox canvas).  Stateless. */
int ach_resample_pass_u8(const uint8_t* src, uint8_t* dst, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, int32_t h_in, int32_t w_in,
                         int32_t h_out, int32_t w_out, int32_t channels, int32_t vertical, int64_t src_pitch, int64_t dst_pitch, void* stream);

/* Training-mode primitives, second set (achelous_amd/csrc/k_train2.h): with the functions above, every arithmetic operation of
 * Achelous.forward in .train() — forward and backward (utils/utils_fit.py:37-166 runs them through ATen autograd).  fp32, NCHW-contiguous.
 * A function with a `dy` argument runs FORWARD when dy == NULL and BACKWARD otherwise.
 *   ach_train_act            kind 0 ReLU, 1 SiLU, 2 GELU (erf), 3 sigmoid: out = f(x) | dy * f'(x)
 *   ach_train_layernorm      over C of elements (r, c, i) at (r*C + c)*inner + i (channels-last rows: inner 1; channels_first maps: inner H*W)
 *   ach_train_dwconv         depthwise k x k, stride 1, pad k/2, w [C,k*k]; flip = 1: the input gradient;  _wgrad: dw [C,k*k]
 *                            (the ONE depthwise family: the Ghost blocks' 3x3, ghost_conv.py:19-23, 47-56, runs through it in the model and stand-alone)
 *   ach_train_im2col         col [B][C*kh*kw][Ho*Wo] <- x (backward = 1: dx <- dcol), dense convolutions run through ach_train_gemm
 *   ach_train_softmax        over the last dimension d of [rows, d]
 *   ach_train_upsample2x     bilinear x2, align_corners=True: [planes,h,w] -> [planes,2h,2w] (backward = 1: the adjoint)
 *   ach_train_maxpool        k x k, stride 1, pad k/2 with arg-max;  ach_train_avgpool3: 3x3 / 9 (self-adjoint)
 *   ach_train_row_reduce     out[r] = scale * sum_i a[r,i] * (b ? b[r,i] : 1);     ach_train_row_scale  out[r,i] = (x ? x[r,i] : 1) * s[r % period]
 *   ach_train_col_reduce     out[c] = scale * sum_r a[r,c] * (b ? b[r,c] : 1);     ach_train_col_scale  out[r,c] = x[r,c] * g[c]
 *   ach_train_instnorm       per-row statistics (GroupNorm with one channel per group), gamma / beta index r % C; backward also returns per-row dgamma / dbeta
 *   ach_train_l2norm         y = x / max(||x||, eps) per row (F.normalize)
 *   ach_train_deform_im2col  modulated deformable 3x3 sampling (torchvision 0.12 deform_conv2d semantics): col [B][C*9][Ho*Wo]
 *   ach_train_deform_bwd     from dcol: doffset, dmask, and dx (scattered with fp32 atomics into a buffer the caller zeroed; dx_zeroed = NULL skips it: an input without a gradient) */
int ach_train_act(const float* x, const float* dy, float* out, int64_t n, int32_t kind, void* stream);
int ach_train_mul(const float* a, const float* b, float* out, int64_t n, void* stream);      /* out = a * b element-wise */
int ach_train_layernorm(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows, int32_t C, int64_t inner,
                        float eps, void* stream);
int ach_train_layernorm_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                            int64_t rows, int32_t C, int64_t inner, void* stream);
int ach_train_dwconv(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, int32_t flip, void* stream);
int ach_train_dwconv_wgrad(const float* x, const float* dz, float* dw, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, void* stream);
int ach_train_im2col(const float* src, float* dst, int32_t B, int32_t C, int32_t H, int32_t W, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                     int32_t Ho, int32_t Wo, int32_t backward, void* stream);
int ach_train_softmax(const float* x, float* y, const float* dy, float* dx, int64_t rows, int32_t d, void* stream);
int ach_train_upsample2x(const float* src, float* dst, int64_t planes, int32_t h, int32_t w, int32_t backward, void* stream);
int ach_train_maxpool(const float* x, float* y, int32_t* idx, const float* dy, float* dx, int64_t planes, int32_t H, int32_t W, int32_t k, void* stream);
int ach_train_avgpool3(const float* x, float* y, int64_t planes, int32_t H, int32_t W, void* stream);
int ach_train_row_reduce(const float* a, const float* b, float* out, int64_t rows, int64_t n, float scale, void* stream);
int ach_train_row_scale(const float* x, const float* s, float* out, int64_t rows, int64_t n, int64_t period, void* stream);
int ach_train_col_reduce(const float* a, const float* b, float* out, int64_t rows, int64_t cols, float scale, void* stream);
int ach_train_col_scale(const float* x, const float* g, float* out, int64_t rows, int64_t cols, void* stream);
int ach_train_instnorm(const float* x, const float* dy, const float* gamma, const float* beta, float* y, float* mean, float* rstd, float* dx, float* dgamma_rows,
                       float* dbeta_rows, int64_t rows, int64_t n, int32_t C, float eps, void* stream);
int ach_train_l2norm(const float* x, float* y, float* norm, const float* dy, float* dx, int64_t rows, int64_t n, float eps, void* stream);
int ach_train_deform_im2col(const float* x, const float* offset, const float* mask, float* col, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                            int32_t stride, int32_t pad, void* stream);
int ach_train_deform_bwd(const float* x, const float* offset, const float* mask, const float* dcol, float* dx_zeroed, float* doffset, float* dmask, int32_t B,
                         int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t stride, int32_t pad, void* stream);

/* PointNet++ in training mode (achelous_amd/csrc/k_train3.h; OUR OWN specification of `pc_seg='pn2'`, DESIGN.md 5b — the reference snapshot builds only 'pn',
 * nets/Achelous.py:31-32, and trains whatever it builds through ATen autograd, utils/utils_fit.py:37-166).  Point tensors are ROWS: xyz [B, n, 3], features [B, n, C].
 *   ach_train_pn2_fps        farthest-point sampling (start at point 0, ties to the lowest index): idx [B, npoint], new_xyz [B, npoint, 3]
 *   ach_train_pn2_group      ball query + grouping: grouped [B*S*nsample, 3 + C] = [xyz - centroid | features], group_idx [B, S, nsample] (first nsample in-ball
 *                            points in index order, padded with the first)
 *   ach_train_pn2_group_bwd  dfeats[b, group_idx, c] += dgrouped[.., 3 + c] into a buffer the caller zeroed (fp32 atomics; the xyz columns carry no gradient)
 *   ach_train_pn2_interp     dout == NULL: out [B*n, C1 + C2] = [skip | sum_j w_j sparse[nn_j]] (3-NN, w = 1 / (d + 1e-8) normalised);
 *                            else the adjoint: dskip [B*n, C1] and dsparse [B, s, C2] (zeroed by the caller, fp32 atomics) from dout */
int ach_train_pn2_fps(const float* xyz, int32_t B, int32_t n, int32_t npoint, int32_t* idx, float* new_xyz, void* stream);
int ach_train_pn2_group(const float* xyz, const float* new_xyz, const float* feats, int32_t C, int32_t B, int32_t n, int32_t S, int32_t nsample, float radius2,
                        float* grouped, int32_t* group_idx, void* stream);
int ach_train_pn2_group_bwd(const int32_t* group_idx, const float* dgrouped, float* dfeats_zeroed, int32_t C, int32_t B, int32_t n, int32_t S, int32_t nsample, void* stream);
int ach_train_pn2_interp(const float* xyz1, const float* xyz2, const float* skip, int32_t C1, const float* sparse, int32_t C2, float* out, float* dskip, float* dsparse_zeroed,
                         const float* dout, int32_t B, int32_t n, int32_t s, void* stream);

/* Training losses (achelous_amd/csrc/k_loss.h; achelous_amd/losses.py): forward and gradient of the reference's losses without a host read, so that a training
 * step with its loss can be captured into a graph.  fp32, contiguous; every workspace belongs to the caller; the same inputs give the same bits.
 *   ach_train_yolo_loss   YOLOX loss with SimOTA assignment (loss/detection_loss.py:60-411) on the three RAW head maps raw_k [B, 5 + C, H_k, W_k] (not modified) and
 *                         packed labels boxes [B, G, 5] = (cx, cy, w, h in input pixels, class), counts [B] (G <= 128; H0*W0 + H1*W1 + H2*W2 <= 5376).
 *                         Four launches: assign (claims [B, G, 10]: anchor or -1, cost, IoU), resolve (matched [B, A] box or -1, pred_iou [B, A], num_fg [B]),
 *                         loss-and-gradient (grad: d loss / d raw_0 | raw_1 | raw_2, flat, each laid out as its map; partial [B * ceil(A / 256)]), reducer (loss [1]).
 *                         Equal costs go to the lowest anchor index, then the lowest box index.
 *   ach_train_loss_scale  out[i] = g[i] * scale[0], the scale read on the device (a stored gradient times the incoming cotangent)
 *   ach_train_seg_loss    loss/segmentation_loss.py:9-59 on logits [B, C, HW] (C <= 16) and INTEGER labels [B, HW] (label_kind 0 int64, 1 int32, 2 uint8; C and anything
 *                         outside 0..C-1 = ignored): mode 0 weighted CE, 1 focal, 2 none; dice != 0 adds the Dice loss with the one-hot target taken from the label.
 *                         cot == NULL: forward, two launches -> stats[0] = loss, stats[1 .. 2 + 2 C) = what the backward needs; partial holds 1024 * (2 + 3 C) floats.
 *                         cot != NULL: backward, one launch: dlogits = cot[0] * d loss / d logits from logits, labels and the forward's stats. */
int ach_train_yolo_loss(const float* raw0, const float* raw1, const float* raw2, const float* boxes, const int32_t* counts, int32_t B, int32_t C, int32_t G,
                        int32_t H0, int32_t W0, int32_t H1, int32_t W1, int32_t H2, int32_t W2, float s0, float s1, float s2, int32_t* claim_anchor, float* claim_cost,
                        float* claim_iou, int32_t* matched, float* pred_iou, int32_t* num_fg, float* grad, float* partial, float* loss, void* stream);
int ach_train_loss_scale(const float* g, const float* scale, float* out, int64_t n, void* stream);
int ach_train_seg_loss(const float* logits, const void* labels, int32_t label_kind, const float* weights, int32_t B, int32_t C, int64_t HW, int32_t mode, int32_t dice,
                       float alpha, float gamma, float beta, float smooth, float* partial, float* stats, const float* cot, float* dlogits, void* stream);

/* Validation metrics (achelous_amd/csrc/k_metrics.h; achelous_amd/metrics.py): the per-batch half of the reference's per-epoch evaluation, one launch each, with
 * no host read and no synchronisation inside.  Every buffer belongs to the caller; both ADD to their accumulators and never clear them.
 *   ach_eval_confusion  utils_seg/utils_metrics.py:31-33 `fast_hist` (and the counts of utils_seg_pc/utils_metrics.py `mean_iou`) with the arg-max fused in:
 *                       hist[n * label + pred] += 1 into a uint64 [n, n] (n <= 16).  pred_kind 0 / 1 / 2: fp32 / bf16 / fp16 logits, layout 0 [B, n, HW] or
 *                       1 [B, HW, n], equal values go to the LOWEST class (numpy / torch.argmax; NaN logits: unspecified); pred_kind 3: a uint8 class map
 *                       [B, HW] (what ach_seg_resize_argmax writes; layout ignored; a value >= n is dropped).  labels [B, HW], label_kind as
 *                       ach_train_seg_loss (0 int64, 1 int32, 2 uint8); a pixel counts only if 0 <= label < n.  Integer adds: the same bits on every run.
 *   ach_eval_match      utils/utils_map.py:462-498 in parallel form, one workgroup per image.  rows [B, max_det, 7] with counts [B]: columns
 *                       (x1, y1, x2, y2, obj, cls_conf, class) as ach_nms writes them, or (y1, x1, y2, x2, ...) as ach_correct_boxes does (yx_order = 1);
 *                       truncate = 1 applies the int() of utils/callbacks.py:216-217 to the four coordinates.  gt [B, G, 5] = (x1, y1, x2, y2, class),
 *                       G <= 128, difficult [B, G] or NULL, gt_counts [B]; max_det <= 1024; thresholds: T <= 10 doubles in HOST memory, read before the launch.
 *                       Per detection: score = obj * cls_conf (fp32), the best same-class box of its image by float64 IoU with the +1 pixel convention
 *                       (the first box reaching the maximum wins) -> match [B, max_det] (-1: none), iou [B, max_det] (-1: no overlap), score [B, max_det],
 *                       and per threshold flags [T, B, max_det]: 0 empty slot, 1 tp, 2 fp, 3 ignored (matched a difficult box).  Rank inside an image is
 *                       score descending, then slot ascending.  gt_per_class [C] uint64 += the non-difficult boxes of each class. */
int ach_eval_confusion(const void* pred, int32_t pred_kind, int32_t layout, const void* labels, int32_t label_kind, int32_t B, int32_t n, int64_t HW, uint64_t* hist,
                       void* stream);
int ach_eval_match(const float* rows, const int32_t* counts, int32_t yx_order, int32_t truncate, const float* gt, const uint8_t* difficult, const int32_t* gt_counts,
                   int32_t B, int32_t max_det, int32_t G, int32_t C, const double* thresholds, int32_t T, uint8_t* flags, int32_t* match, double* iou, float* score,
                   uint64_t* gt_per_class, void* stream);

/* Training batches assembled on the device from ragged frames (achelous_amd/csrc/k_data.h; achelous_amd/data.py): the reference's dataset step
 * (utils/dataloader.py:87-148, 153-233) for a whole batch, with a launch count that does not depend on the batch and no device-to-host copy.
 * All images sit in one packed uint8 arena (HWC rows), all label maps in another; frames are described by a host-built int64 table of 16 columns per frame
 * whose copy on the device the kernels read.  `tabs` is one int32 buffer holding every bounds / coefficient / index table; table offsets count its elements.
 * Both entries read the HOST copies (`table_host`, `tabs_host`) first and check every extent against its arena, every table offset against `tabs_len` and every
 * table entry the kernels will follow against its source axis: a bad table returns ACH_ERR_INVALID with a message and launches nothing.
 *   ach_data_letterbox_batch  PIL Image.BICUBIC resize to (nw, nh) pasted at (dx, dy) on a (128, 128, 128) R x R canvas, then ((v / 255) - mean) / std through
 *                       `lut`, 768 floats [channel][value] on the device.  Image table: 0 byte offset, 1 H, 2 W, 3 pitch, 4 nw, 5 nh, 6 dx, 7 dy, 8 horizontal
 *                       bounds [nw][2], 9 horizontal coefficients [nw][ks], 10 ks, 11-13 the same for the vertical axis, 14 byte offset (a multiple of 4) into
 *                       `mid`, 15 unused.  Bounds and coefficients as for ach_resample_pass_u8, over the whole axis.  dx, dy of either sign; the window may be
 *                       larger than the canvas or outside it: the paste clips and only visible pixels are computed.  `arena`: 16-byte aligned, `arena_bytes` a
 *                       multiple of 16.  `mid`: the 8-bit intermediate, per frame 3 * round_up(R, 4) bytes for every source row the visible rows need.
 *                       out_kind 0 / 1 / 2: [B, 3, R, R] fp32 / bf16 / fp16 (one RNE rounding of the fp32 table value); 3: the bytes, [B, R, R, 3] (lut unused).
 *                       Two launches; a row wider than 16379 needed source columns is ACH_ERR_UNSUPPORTED.
 *   ach_data_labels_batch   PIL Image.NEAREST resize + paste on zeros + min(v, n) for both label maps of every frame in one launch: n = num_classes_seg for `png`,
 *                       2 for `png_w`.  Label table: 0 nw, 1 nh, 2 dx, 3 dy, then per map (png at 4, png_w at 10): byte offset (negative: the frame has no such
 *                       map, zeros are written), H, W, pitch, column index table [nw], row index table [nh] (source index per resized sample, -1: none).
 *                       label_kind as ach_train_seg_loss: 0 int64, 2 uint8 outputs [B, R, R]. */
int ach_data_letterbox_batch(const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const int32_t* tabs_host,
                             const int32_t* tabs_dev, int64_t tabs_len, const float* lut, int32_t B, int32_t R, uint8_t* mid, int64_t mid_bytes, void* out,
                             int32_t out_kind, void* stream);
int ach_data_labels_batch(const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const int32_t* tabs_host,
                          const int32_t* tabs_dev, int64_t tabs_len, int32_t B, int32_t R, int32_t num_classes_seg, void* png, void* png_w, int32_t label_kind,
                          void* stream);

/* Both radar inputs of the network from raw radar point clouds (achelous_amd/csrc/k_radarmap.h; achelous_amd/data.py): the reference's offline map generation
 * (radar_feature_map_generate.ipynb) and its per-frame point sampling (utils/dataloader.py:137-141) for a whole batch of ragged clouds, with a launch count that
 * does not depend on the batch and no device-to-host copy.  All clouds sit in one packed arena of fp32 (in_kind 0) or fp64 (in_kind 1) rows, aligned to its
 * element size, `arena_elems` elements long; frames are described by a host-built int64 table of 16 columns per frame whose copy on the device the kernels read.
 * Cloud table: 0 element offset of the first row, 1 n (rows), 2 F (columns per row), 3 row stride in elements (>= F), 4 / 5 / 6 the columns of range, doppler
 * and RCS (the map's three channels), 7 / 8 the columns of u and v, 9-15 unused.  Both entries read the HOST copy first and check every extent against the
 * arena and every column against F (ach_data_radar_points also every row index against n): a bad table returns ACH_ERR_INVALID with a message and launches
 * nothing.  The kernels test every cell index computed from the data on the device.
 *   ach_data_radar_maps   `raw` [B, 3, R, R] fp32: per channel and point in row order, x = int(u / cell_u), y = int(v / cell_v) in float64 (truncation toward
 *                       zero; an index in [-R, -1] wraps, anything else outside, NaN and infinities skip the point); if raw[ch][y][x] != 0 and the un-wrapped
 *                       x >= 1 then x -= 1; raw[ch][y][x] = the channel's value rounded once to fp32.  n = 0 gives a zero map; n is not limited.  One launch.
 *                       `out` not NULL: also (raw - min) / (max - min) + 1e-13 with min / max per frame over all channels, as ach_preprocess_radar computes it
 *                       from `raw` (the same bits), [B, 3, R, R] of out_kind 0 / 1 / 2 = fp32 / bf16 / fp16; the extrema come out of the first launch through
 *                       `partial` (at least 2 * B * R floats are always enough), so this is one more launch.  R <= 2048, else ACH_ERR_UNSUPPORTED.
 *   ach_data_radar_points N rows per frame by `indices` [B, N] int64 (host and device copies), the D <= 16 columns `columns` (host int32) each divided by its L2
 *                       norm over the sampled rows in fp32 (sklearn normalize(axis=0); a zero column stays zero) -> `points` [B, D, N] of out_kind 0 / 1 / 2;
 *                       label_column >= 0: that column of the sampled rows -> `labels` [B, N] int64 (label_column < 0 and labels NULL: none).  Every cloud
 *                       holds at least one row.  One launch. */
int ach_data_radar_maps(const void* arena, int64_t arena_elems, int32_t in_kind, const int64_t* table_host, const int64_t* table_dev, int32_t B, int32_t R,
                        double cell_u, double cell_v, float* raw, float* partial, int64_t partial_floats, void* out, int32_t out_kind, void* stream);
int ach_data_radar_points(const void* arena, int64_t arena_elems, int32_t in_kind, const int64_t* table_host, const int64_t* table_dev, const int64_t* indices_host,
                          const int64_t* indices_dev, const int32_t* columns, int32_t D, int32_t label_column, int32_t B, int32_t N, void* points,
                          int32_t out_kind, int64_t* labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACHELOUS_H_ */
