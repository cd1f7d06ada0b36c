/* achelous_heatmap.h — extension of the C ABI of libachelous_hip.so (include/achelous.h, which this header includes and whose conventions, error codes and
 * ach_last_error(NULL) it shares): the heat-map mode on served frames.  A header of its own, so that the set of entries include/achelous.h declares stays what it is;
 * the Python binding reads this header exactly as it reads that one (achelous_amd/engine.py EXTENSION_HEADERS). */
#ifndef ACHELOUS_HEATMAP_H_
#define ACHELOUS_HEATMAP_H_

#include "achelous.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's heat-map mode (achelous.detect_heatmap, achelous.py:451-555) for a ragged batch from the detection maps of a forward, in three launches whatever
 * the batch (achelous_amd/csrc/k_heatmap.h): per cell max_c sigmoid(cls) * sigmoid(obj); every level stretched to the frame's own size (cv2 INTER_LINEAR, float32, not
 * contracted), truncated to uint8, the maximum over the levels = the mask; the mask's range; the mask through a colour map, blended over a base image.  Stateless.
 *   det_kind     element type of det3 / det4 / det5: 0 fp32, 1 bf16, 2 fp16 (the in_kind / pred_kind codes); device [batch, 5 + num_det, R/s, R/s], s = 8, 16, 32.
 *                R is a multiple of 32; more than 4096 cells per frame (R above 416): ACH_ERR_UNSUPPORTED.
 *   scores       workspace and output, float32 [batch, A], level-major, A = (R/8)^2 + (R/16)^2 + (R/32)^2.  A cell with a NaN logit scores 0.
 *   frame table  int64 [batch][16], host copy and device copy: 0 byte offset of the frame in `base`, 1 H, 2 W, 3 base pitch (>= 3 W), 4 y0, 5 x0, 6 nh, 7 nw (the
 *                window of the R x R network input the frame covers; (0, 0, R, R) is the reference, which stretches the whole map over the frame), 8 byte offset
 *                of the mask in `mask`, 9 mask pitch, 10 byte offset of the coloured frame in `out`, 11 its pitch, 12-15 unused.  Offsets and pitches of `mask`
 *                and `out` are multiples of 16 (a thread stores the dwords of 4 neighbouring pixels; bytes of a row's last dword past W are written as zero).
 *   mask         uint8 arena (16-byte aligned): m = max_l uint8(trunc(resize_l * 255)).  stats: int32 [batch][2] = (max m, max 255 - m): hi = stats[0],
 *                lo = 255 - stats[1]; zeroed by the first launch.
 *   cmap_dev, alpha, base, out   colour, all optional together (out == NULL: mask and statistics only, two launches): colour map uint8 [256][3] on the device;
 *                out = blend(base, cmap[idx(m)], alpha), idx(m) = min(int((m - lo) / (hi - lo) * 256.0), 255) in double, 0 when hi == lo (matplotlib's
 *                Normalize(lo, hi) and a 256-entry colour map), blend(a, b, t) = (uint8)(a + t * (b - a)) in float32 as PIL's Image.blend, 0 <= alpha <= 1.
 *                `base`: packed HWC uint8 frames, 4-byte aligned and padded to 4 bytes; `out`: an arena of its own (16-byte aligned, not overlapping `base`) or
 *                `base` itself (in place: out offsets and pitches equal the base's).
 * The host copy of the table is checked before anything is launched: an extent past an arena, a bad pitch or alignment, H or W < 1, a window outside R x R or
 * empty, alpha outside [0, 1], R not a multiple of 32 -> ACH_ERR_INVALID, no launch. */
int ach_heatmap_frames(int32_t det_kind, int32_t R, int32_t num_det, int32_t batch, const void* det3, const void* det4, const void* det5, float* scores,
                       const uint8_t* base, int64_t base_bytes, const int64_t* table_host, const int64_t* table_dev, const uint8_t* cmap_dev, float alpha,
                       uint8_t* mask, int64_t mask_bytes, int32_t* stats, uint8_t* out, int64_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACHELOUS_HEATMAP_H_ */
