/* achelous_points.h — extension of the C ABI of libachelous_hip.so (include/achelous.h, which this header includes and whose conventions, error codes and
 * ach_last_error(NULL) it shares): the picture of the radar point classes on served frames.  A header of its own, so that the set of entries include/achelous.h
 * declares stays what it is; the Python binding reads this header exactly as it reads that one (achelous_amd/engine.py POINT_ENTRIES). */
#ifndef ACHELOUS_POINTS_H_
#define ACHELOUS_POINTS_H_

#include "achelous.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's scatter of the radar point classes (achelous.py:261-271) for a ragged batch, in two launches whatever the batch (achelous_amd/csrc/k_scatter.h):
 * per frame the table np.unique(concat[u, v, rcs, class], axis=0) of the sampled points, and every row of it painted as a disc in its class colour, in sorted order,
 * later rows over earlier ones, in place into a packed HWC uint8 arena.  Stateless.
 *   arena        packed HWC uint8 frames, 4-byte aligned.  A byte no disc covers is not written.
 *   frame table  int64 [batch][16], host copy and device copy: 0 byte offset of the frame in `arena`, 1 H, 2 W (1..2^20), 3 pitch (>= 3 W; offset and pitch are
 *                multiples of 4), 4 element offset of the frame's cloud in `clouds`, 5 n (its rows, 0 allowed), 6 F (columns per row), 7 row stride in elements
 *                (>= F), 8 / 9 / 10 the columns of u, v and the marker size s (the reference's rcs), each < F, 11-15 unused.
 *   clouds       device float32 (cloud_kind 0) or float64 (1), cloud_elems elements, aligned to its element size.
 *   indices_dev  device int64 [batch][num_points]: sample j of frame b is row indices[b][j] of its cloud; NULL: row j.  Tested against n ON THE DEVICE: a sample
 *                whose index is outside [0, n) is dropped and nothing is read for it.
 *   point_class  device int64 [batch][num_points]: the class of every sample; a sample whose class is outside [0, num_classes) is dropped, as is one whose u, v or s
 *                is not finite.  num_points is 1..4096 (above: ACH_ERR_UNSUPPORTED, nothing launched), num_classes 1..256.
 *   rows         out, float64 [batch][num_points][4]: the kept samples as (u, v, s, class), ascending by (u, v, s, class) by value, equal rows once; rows past the
 *                count are zero.  count: out, int32 [batch].  class_range: out, int32 [batch][2] = the smallest and largest class among the rows, (0, 0) without one.
 *   colours_dev  device uint8 [256][3].  colour_mode 0: a colour map, entry 0 when hi == lo, else min(((c - lo) * 256) / (hi - lo), 255) over the frame's own
 *                class_range (matplotlib's Normalize and a 256-entry map); 1: the same over the fixed (range_lo, range_hi), 0 <= range_lo <= range_hi <= 255, ids
 *                clamped to it; 2: a palette, entry c.
 *   k, max_radius  pixel (x, y), centre at integer coordinates, is covered by a row iff s > 0 and dx * dx + dy * dy <= min(k * s, max_radius^2), dx = x - u,
 *                dy = y - v, every operation one rounded float64 operation.  k > 0 and finite, max_radius 1..256.
 *   alpha        a covered pixel becomes (uint8)(p + alpha * (colour - p)) per channel in float32 (PIL's Image.blend), once per covering row, in the rows' order.
 *   discs, boxes workspaces, 16-byte aligned: at least batch * num_points * 32 and batch * num_points * 16 bytes.
 * The host copy of the table is checked before anything is launched: a frame's extent past the arena, a pitch below 3 W, an offset or pitch that is no multiple of 4,
 * H or W outside 1..2^20, a cloud's extent past `clouds`, a column index >= F, num_points < 1, num_classes, alpha, k or max_radius out of range, a workspace too small
 * or misaligned -> ACH_ERR_INVALID, no launch. */
int ach_scatter_points_frames(uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, int32_t batch, const void* clouds,
                              int64_t cloud_elems, int32_t cloud_kind, const int64_t* indices_dev, const int64_t* point_class, int32_t num_points,
                              int32_t num_classes, const uint8_t* colours_dev, int32_t colour_mode, int32_t range_lo, int32_t range_hi, float alpha, double k,
                              int32_t max_radius, double* rows, int32_t* count, int32_t* class_range, double* discs, int64_t discs_bytes, int32_t* boxes,
                              int64_t boxes_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACHELOUS_POINTS_H_ */
