// api_frames.cpp — the entries that work on ragged batches of frames: the resample pass, training batches and radar inputs assembled on the device (k_data.h,
// k_radarmap.h), serving at every frame's own size (k_serve.h), drawing (k_draw.h), the heat-map mode (k_heatmap.h) and the point-class scatter (k_scatter.h).  What they share is the host-side check of a frame table against its arenas
// BEFORE anything is launched: a bad table must never become an out-of-bounds access on the device.  See api.cpp / api_util.h.
#include <algorithm>
#include <cmath>

#include "api_util.h"
#include "k_detect.h"      // (k_prepost.h takes its host-side round-to-nearest helpers from here)
#include "k_prepost.h"
#include "k_data.h"
#include "k_radarmap.h"
#include "k_serve.h"
#include "k_draw.h"
#include "k_heatmap.h"
#include "k_scatter.h"
#include "../../include/achelous_heatmap.h"
#include "../../include/achelous_points.h"

static const int64_t SIZE_TOP = (1L << 30) - 1;      // a frame's H and W (the drawing entry has a limit of its own)
static_assert(int(ach::DATA_F32) == KIND_F32 && int(ach::DATA_BF16) == KIND_BF16 && int(ach::DATA_F16) == KIND_F16 && int(ach::DATA_U8_HWC) == KIND_U8, "the data entries' kinds are ElemKind");

extern "C" {

// ---- one pass of the 8-bit PIL resample (k_prepost.h): stateless
int ach_resample_pass_u8(const uint8_t* src, uint8_t* dst, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, int32_t h_in, int32_t w_in,
                         int32_t h_out, int32_t w_out, int32_t channels, int32_t vertical, int64_t src_pitch, int64_t dst_pitch, void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        if (!src || !dst || !bounds || !coeffs || ksize <= 0 || h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0 || channels <= 0 ||
            (vertical ? w_out != w_in : h_out != h_in))
            throw ach::AchError{ACH_ERR_INVALID, "bad resample_pass arguments"};
        ach::ResamplePassParams p{src, dst, bounds, coeffs, ksize, h_in, w_in, h_out, w_out, channels, vertical, long(src_pitch), long(dst_pitch)};
        ACH_LAUNCH(ach::resample_pass_kernel, dim3(unsigned(ach::cdivl(long(h_out) * w_out * channels, 256))), dim3(256), s, p);
    });
}

// ---- training batches from ragged frames (k_data.h).  Both entries check the host copy of the frame table — every extent against its arena, every table
// offset against `tabs`, every bounds / index entry the kernels will follow — BEFORE anything is launched; a bad table is ACH_ERR_INVALID and no launch.
static void data_need_bounds(const int32_t* tabs, int64_t tabs_len, int64_t boff, int64_t koff, int64_t ks, int64_t n_out, int64_t n_in, const char* what) {
    need(ks >= 1 && boff >= 0 && koff >= 0 && n_out <= (tabs_len - boff) / 2 && boff + 2 * n_out <= tabs_len && n_out <= (tabs_len - koff) / ks && koff + n_out * ks <= tabs_len, what);
}
int ach_data_letterbox_batch(const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const int32_t* tabs_host,
                             const int32_t* tabs_dev, int64_t tabs_len, const float* lut, int32_t B, int32_t R, uint8_t* mid, int64_t mid_bytes, void* out,
                             int32_t out_kind, void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        need(arena && table_host && table_dev && tabs_host && tabs_dev && mid && out && B > 0 && R > 0 && R <= 16384 && tabs_len >= 0 && mid_bytes >= 0, "ach_data_letterbox_batch");
        need(out_kind >= ach::DATA_F32 && out_kind <= ach::DATA_U8_HWC && (lut || out_kind == ach::DATA_U8_HWC), "ach_data_letterbox_batch: out_kind 0..3, a value table unless 3");
        need(arena_bytes > 0 && arena_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(arena) & 15u) == 0 && (reinterpret_cast<uintptr_t>(mid) & 3u) == 0,
             "ach_data_letterbox_batch: the image arena is 16-byte aligned and padded to 16 bytes");
        const int R4 = (R + 3) / 4 * 4;
        long max_span = 0, max_rows = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t* f = table_host + long(b) * ach::DATA_TABLE_COLS;
            const int64_t off = f[0], H = f[1], W = f[2], pitch = f[3], nw = f[4], nh = f[5], dx = f[6], dy = f[7];
            need(dims_ok(H, W, SIZE_TOP) && frame_fits(off, H, 3 * W, pitch, 3 * W, arena_bytes), "ach_data_letterbox_batch: a frame's extent passes the image arena");
            need(placement_ok(nw, nh, dx, dy), "ach_data_letterbox_batch: placement out of range");
            data_need_bounds(tabs_host, tabs_len, f[8], f[9], f[10], nw, W, "ach_data_letterbox_batch: a horizontal table offset passes the table buffer");
            data_need_bounds(tabs_host, tabs_len, f[11], f[12], f[13], nh, H, "ach_data_letterbox_batch: a vertical table offset passes the table buffer");
            const ach::DataWindow w = ach::data_window(nw, nh, dx, dy, R);
            if (w.vx0 >= w.vx1 || w.vy0 >= w.vy1) continue;
            // the entries the kernels follow: inside the source axis, at most ks taps, both ends non-decreasing (the staged range is [first of the first, end of the last))
            auto walk = [&](int64_t boff, int64_t ks, long lo, long hi, int64_t n_in, long& first0, long& end1) {
                long pf = 0, pe = 0;
                for (long o = lo; o < hi; ++o) {
                    const long first = tabs_host[boff + 2 * o], count = tabs_host[boff + 2 * o + 1];
                    need(first >= 0 && count >= 0 && count <= ks && first + count <= n_in && (o == lo || (first >= pf && first + count >= pe)),
                         "ach_data_letterbox_batch: a bounds entry leaves its source axis");
                    pf = first; pe = first + count;
                    if (o == lo) first0 = first;
                }
                end1 = pe;
            };
            long sx0 = 0, sx1 = 0, r0 = 0, r1 = 0;
            walk(f[8], f[10], w.vx0 - dx, w.vx1 - dx, W, sx0, sx1);
            walk(f[11], f[13], w.vy0 - dy, w.vy1 - dy, H, r0, r1);
            need(f[14] >= 0 && f[14] % 4 == 0 && f[14] <= mid_bytes && (r1 - r0) * 3 * R4 <= mid_bytes - f[14], "ach_data_letterbox_batch: a frame's intermediate passes the intermediate arena");
            max_span = std::max(max_span, (sx1 - sx0) * 3);
            max_rows = std::max(max_rows, r1 - r0);
        }
        if (max_rows > 0 && max_span > 0) {
            const long lstride = (max_span + 15 + 15) / 16 * 16;
            if (lstride > ach::DATA_LDS_BYTES) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_data_letterbox_batch: a frame needs more than 16379 source columns of one row"};
            const int rows_pb = int(std::min<long>(ach::DATA_ROWS, ach::DATA_LDS_BYTES / lstride));
            ach::DataHParams hp{arena, reinterpret_cast<const long long*>(table_dev), tabs_dev, mid, R, R4, rows_pb, int(lstride)};
            ACH_LAUNCH(ach::data_hpass_kernel, dim3(unsigned(ach::cdivl(max_rows, rows_pb)), unsigned(B)), dim3(256), s, hp);
        }
        ach::DataVParams vp{reinterpret_cast<const long long*>(table_dev), tabs_dev, mid, lut, out, R, R4};
        const dim3 grid(unsigned(ach::cdivl(long(R) * (R4 / 4), 256)), unsigned(B));
        by_kind<uint8_t>(out_kind, [&](auto e) { ACH_LAUNCH(ach::data_vpass_kernel<typename decltype(e)::type>, grid, dim3(256), s, vp); });
    });
}
int ach_data_labels_batch(const uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, const int32_t* tabs_host,
                          const int32_t* tabs_dev, int64_t tabs_len, int32_t B, int32_t R, int32_t num_classes_seg, void* png, void* png_w, int32_t label_kind,
                          void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        need(arena && table_host && table_dev && tabs_host && tabs_dev && png && png_w && B > 0 && B <= 65535 && R > 0 && R <= 16384 && tabs_len >= 0 && arena_bytes >= 0, "ach_data_labels_batch");
        need(num_classes_seg >= 0 && num_classes_seg <= 255 && (label_kind == 0 || label_kind == 2), "ach_data_labels_batch: classes 0..255, label_kind 0 (int64) or 2 (uint8)");
        for (int b = 0; b < B; ++b) {
            const int64_t* f = table_host + long(b) * ach::DATA_TABLE_COLS;
            const int64_t nw = f[0], nh = f[1], dx = f[2], dy = f[3];
            need(placement_ok(nw, nh, dx, dy), "ach_data_labels_batch: placement out of range");
            const ach::DataWindow w = ach::data_window(nw, nh, dx, dy, R);
            for (int m = 0; m < 2; ++m) {
                const int64_t* g = f + 4 + 6 * m;
                if (g[0] < 0) continue;
                const int64_t off = g[0], H = g[1], W = g[2], pitch = g[3];
                need(dims_ok(H, W, SIZE_TOP) && frame_fits(off, H, W, pitch, W, arena_bytes), "ach_data_labels_batch: a label map's extent passes the label arena");
                need(g[4] >= 0 && g[5] >= 0 && nw <= tabs_len - g[4] && nh <= tabs_len - g[5], "ach_data_labels_batch: an index table offset passes the table buffer");
                if (w.vx0 >= w.vx1 || w.vy0 >= w.vy1) continue;
                for (long o = w.vx0 - dx; o < w.vx1 - dx; ++o) need(tabs_host[g[4] + o] >= -1 && tabs_host[g[4] + o] < W, "ach_data_labels_batch: a column index leaves its map");
                for (long o = w.vy0 - dy; o < w.vy1 - dy; ++o) need(tabs_host[g[5] + o] >= -1 && tabs_host[g[5] + o] < H, "ach_data_labels_batch: a row index leaves its map");
            }
        }
        ach::DataLabelParams lp{arena, reinterpret_cast<const long long*>(table_dev), tabs_dev, {png, png_w}, R, num_classes_seg, label_kind == 0 ? 1 : 0};
        ACH_LAUNCH(ach::data_labels_kernel, dim3(unsigned(ach::cdivl(long(R) * R, 256)), 2u, unsigned(B)), dim3(256), s, lp);
    });
}

// ---- both radar inputs from raw point clouds (k_radarmap.h).  The host copy of the cloud table is checked against the arena — every extent, every column — and
// the sampled row indices against every frame's n BEFORE anything is launched; a bad table is ACH_ERR_INVALID and no launch.
static void radar_need_table(const int64_t* table_host, int32_t B, int64_t arena_elems, int64_t min_rows, const char* extent, const char* column) {
    for (int b = 0; b < B; ++b) {
        const int64_t* f = table_host + long(b) * ach::RADAR_TABLE_COLS;
        const int64_t off = f[0], n = f[1], F = f[2], stride = f[3];
        need(n >= min_rows && n < (1L << 40) && F >= 1 && F < (1L << 20) && frame_fits(off, n, F, stride, F, arena_elems, 1, 1L << 20), extent);      // (no row: F - stride fits)
        for (int c = 4; c < 9; ++c) need(f[c] >= 0 && f[c] < F, column);
    }
}
int ach_data_radar_maps(const void* arena, int64_t arena_elems, int32_t in_kind, const int64_t* table_host, const int64_t* table_dev, int32_t B, int32_t R,
                        double cell_u, double cell_v, float* raw, float* partial, int64_t partial_floats, void* out, int32_t out_kind, void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        need(arena && table_host && table_dev && raw && B > 0 && B <= 65535 && R > 0 && arena_elems >= 0 && (in_kind == ach::RADAR_IN_F32 || in_kind == ach::RADAR_IN_F64), "ach_data_radar_maps");
        if (R > ach::RADAR_MAX_R) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_data_radar_maps: a map larger than 2048 x 2048"};
        need((reinterpret_cast<uintptr_t>(arena) & (in_kind == ach::RADAR_IN_F64 ? 7u : 3u)) == 0, "ach_data_radar_maps: the cloud arena is aligned to its element size");
        need(std::isfinite(cell_u) && std::isfinite(cell_v) && cell_u != 0.0 && cell_v != 0.0, "ach_data_radar_maps: the cell sizes are finite and not zero");
        const int rows = ach::radar_band_rows(R), bands = int(ach::cdivl(R, rows));
        need(!out || (out_kind >= ach::DATA_F32 && out_kind <= ach::DATA_F16 && partial && partial_floats >= 2L * B * bands),
             "ach_data_radar_maps: the normalised map is fp32 / bf16 / fp16 (0..2) and needs 2 * B * ceil(R / band rows) floats of `partial`");
        radar_need_table(table_host, B, arena_elems, 0, "ach_data_radar_maps: a cloud's extent passes the cloud arena", "ach_data_radar_maps: a column index is not below F");
        ach::RadarMapParams p{arena, reinterpret_cast<const long long*>(table_dev), raw, out ? partial : nullptr, cell_u, cell_v, R, rows, bands, in_kind};
        ACH_LAUNCH(ach::radar_map_kernel, dim3(unsigned(bands), unsigned(B)), dim3(256), s, p);
        if (!out) return;
        const long per = 3L * R * R;
        ach::RadarScaleParams ps{raw, partial, out, per, bands, B};
        const dim3 grid(unsigned(ach::cdivl(per * B, 256)));
        by_kind(out_kind, [&](auto e) { ACH_LAUNCH(ach::radar_scale_kernel<typename decltype(e)::type>, grid, dim3(256), s, ps); });
    });
}
int ach_data_radar_points(const void* arena, int64_t arena_elems, int32_t in_kind, const int64_t* table_host, const int64_t* table_dev, const int64_t* indices_host,
                          const int64_t* indices_dev, const int32_t* columns, int32_t D, int32_t label_column, int32_t B, int32_t N, void* points,
                          int32_t out_kind, int64_t* labels, void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        need(arena && table_host && table_dev && indices_host && indices_dev && columns && points && B > 0 && N > 0 && arena_elems >= 0 &&
             (in_kind == ach::RADAR_IN_F32 || in_kind == ach::RADAR_IN_F64) && out_kind >= ach::DATA_F32 && out_kind <= ach::DATA_F16, "ach_data_radar_points");
        need(D >= 1 && D <= ach::RADAR_MAX_D && long(B) * (D + 1) < (1L << 31), "ach_data_radar_points: 1..16 point columns");
        need((labels != nullptr) == (label_column >= 0), "ach_data_radar_points: a label column and a label output go together");
        need((reinterpret_cast<uintptr_t>(arena) & (in_kind == ach::RADAR_IN_F64 ? 7u : 3u)) == 0, "ach_data_radar_points: the cloud arena is aligned to its element size");
        radar_need_table(table_host, B, arena_elems, 1, "ach_data_radar_points: a cloud is empty or its extent passes the cloud arena",
                         "ach_data_radar_points: a column index is not below F");
        ach::RadarPointsParams p{arena, reinterpret_cast<const long long*>(table_dev), reinterpret_cast<const long long*>(indices_dev), points,
                                 reinterpret_cast<long long*>(labels), N, D, in_kind, label_column, {}};
        for (int b = 0; b < B; ++b) {
            const int64_t* f = table_host + long(b) * ach::RADAR_TABLE_COLS;
            for (int d = 0; d < D; ++d) need(columns[d] >= 0 && columns[d] < f[2], "ach_data_radar_points: a column index is not below F");
            need(label_column < f[2], "ach_data_radar_points: a column index is not below F");
            for (long i = 0; i < N; ++i) need(indices_host[long(b) * N + i] >= 0 && indices_host[long(b) * N + i] < f[1], "ach_data_radar_points: a row index is not below n");
        }
        for (int d = 0; d < D; ++d) p.cols[d] = columns[d];
        const dim3 grid(unsigned(B * (D + 1)));
        by_kind(out_kind, [&](auto e) { ACH_LAUNCH(ach::radar_points_kernel<typename decltype(e)::type>, grid, dim3(256), s, p); });
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
        need(batch > 0 && batch <= 65535 && table_host && table_dev && (out_semantic || out_waterline || out_overlay), "ach_seg_overlay_frames: a batch, a frame table and an output");
        need((!want_se || (se_seg && prob_se && channels >= 1 && channels <= 255)) && (!want_line || (lane_seg && prob_line)),
             "ach_seg_overlay_frames: every wanted output needs its head and probability workspace (1..255 classes)");
        const int R = h->eng->cfg.resolution, C0 = want_se ? channels : 0, C1 = want_line ? 2 : 0;
        if ((C0 + C1) * ach::SERVE_TW * 2 > ach::SERVE_LDS_FLOATS) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_seg_overlay_frames: more than 30 semantic classes"};
        need(aligned16(out_semantic, out_waterline, out_overlay) && semantic_bytes >= 0 && waterline_bytes >= 0 && overlay_bytes >= 0, "ach_seg_overlay_frames: output arenas are 16-byte aligned");
        if (out_overlay) {
            need(arena && consts_host && consts_dev && aligned16(arena) && arena_bytes > 0 && arena_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(consts_dev) & 3u) == 0,
                 "ach_seg_overlay_frames: the overlay needs the image arena (16-byte aligned, padded to 16 bytes) and the constants");
            need(blend_se >= 0.f && blend_se <= 1.f && blend_line >= 0.f && blend_line <= 1.f, "ach_seg_overlay_frames: blend factors lie in [0, 1]");
            need(palette_se_len >= 1 && palette_se_len <= 256 && palette_line_len >= 1 && palette_line_len <= 256, "ach_seg_overlay_frames: palettes hold 1..256 colours");
            for (int c = 0; c < channels; ++c)
                need(consts_host[ach::SERVE_REMAP_SE + c] < palette_se_len, "ach_seg_overlay_frames: the semantic palette is shorter than the remapped class range");
            for (int c = 0; c < 2; ++c)
                need(consts_host[ach::SERVE_REMAP_LINE + c] < palette_line_len, "ach_seg_overlay_frames: the water-line palette is shorter than the remapped class range");
        }
        const int rows = ach::serve_rows(C0 + C1);
        long blocks = 0;
        for (int b = 0; b < batch; ++b) {
            const int64_t* f = table_host + long(b) * ach::SERVE_TABLE_COLS;
            const int64_t H = f[1], W = f[2], y0 = f[4], x0 = f[5], nh = f[6], nw = f[7], mp = f[10];
            need(dims_ok(H, W, SIZE_TOP), "ach_seg_overlay_frames: a frame's H and W are at least 1");
            need(nh >= 1 && nw >= 1 && y0 >= 0 && x0 >= 0 && nh <= R - y0 && nw <= R - x0, "ach_seg_overlay_frames: a frame's window leaves the network map");
            if (out_semantic || out_waterline) need(mp >= W && mp % 16 == 0 && mp < (1L << 32), "ach_seg_overlay_frames: the class maps' pitch is a multiple of 16, at least W");
            if (out_semantic) need(frame_fits(f[8], H, W, mp, mp, semantic_bytes, 16), "ach_seg_overlay_frames: a frame's semantic map passes its arena");
            if (out_waterline) need(frame_fits(f[9], H, W, mp, mp, waterline_bytes, 16), "ach_seg_overlay_frames: a frame's water-line map passes its arena");
            if (out_overlay) {
                need(frame_fits(f[0], H, 3 * W, f[3], 3 * W, arena_bytes), "ach_seg_overlay_frames: a frame's extent passes the image arena");
                need(frame_fits(f[11], H, 3 * W, f[12], f[12], overlay_bytes, 16), "ach_seg_overlay_frames: a frame's overlay passes its arena");
            }
            blocks = std::max(blocks, ach::cdivl(W, ach::SERVE_TW) * ach::cdivl(nh, rows - 1));
        }
        need(blocks < (1L << 31), "ach_seg_overlay_frames: a frame is too large");
        const hipStream_t s = as_stream(stream);
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
        need(batch > 0 && max_det > 0 && rows && count && shapes_host && shapes_dev && out_rows, "ach_correct_boxes_frames");
        for (int b = 0; b < batch; ++b) need(shapes_host[2 * b] >= 1 && shapes_host[2 * b + 1] >= 1, "ach_correct_boxes_frames: a frame's H and W are at least 1");
        h->eng->correct_boxes_frames(batch, max_det, rows, count, shapes_dev, letterbox, out_rows, as_stream(stream));
    });
}

// ---- drawing the kept detections on served frames (k_draw.h): box rings, label plates and label text of a ragged batch in two launches, in place.  Stateless.
// Every host table is checked before anything is launched; what comes from DEVICE data (count, class id, score, coordinates) is bounded by the kernels themselves.
int ach_draw_detections_frames(uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, int32_t batch, const float* boxes,
                               const int32_t* count, int32_t max_det, int32_t num_classes, const int32_t* labels_host, const int32_t* labels_dev, int64_t num_labels,
                               const uint8_t* blob_dev, int64_t blob_bytes, const uint8_t* style_dev, int32_t* records, int32_t* class_counts, void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        need(arena && table_host && table_dev && boxes && count && labels_host && labels_dev && blob_dev && style_dev && records && batch > 0 && batch <= 65535 &&
             arena_bytes > 0 && num_labels > 0 && num_labels < (1L << 24) && blob_bytes >= 0, "ach_draw_detections_frames");
        need(max_det >= 1 && max_det <= ach::DRAW_MAX_DET, "ach_draw_detections_frames: max_det is 1..1024");
        need(num_classes >= 1 && num_classes <= ach::DRAW_MAX_CLASSES, "ach_draw_detections_frames: num_classes is 1..256");
        need((reinterpret_cast<uintptr_t>(arena) & 3u) == 0 && (reinterpret_cast<uintptr_t>(records) & 15u) == 0,
             "ach_draw_detections_frames: the arena is 4-byte aligned and the record workspace 16-byte aligned");
        for (int64_t l = 0; l < num_labels; ++l) {
            const int32_t* L = labels_host + l * ach::DRAW_LABEL_COLS;
            need(L[0] >= 0 && L[1] >= 0 && L[2] >= 0 && L[1] <= 4096 && L[2] <= 4096 && int64_t(L[1]) * L[2] <= blob_bytes - L[0], "ach_draw_detections_frames: a label's mask passes the atlas blob");
            need(L[3] >= -65536 && L[3] <= 65536 && L[4] >= -65536 && L[4] <= 65536 && L[5] >= 0 && L[5] <= 65536 && L[6] >= 0 && L[6] <= 65536,
                 "ach_draw_detections_frames: a label's offsets and size are out of range");
        }
        long blocks = 0;
        for (int b = 0; b < batch; ++b) {
            const int64_t* f = table_host + long(b) * ach::DRAW_TABLE_COLS;
            const int64_t off = f[0], H = f[1], W = f[2], pitch = f[3];
            need(dims_ok(H, W, 1L << 20), "ach_draw_detections_frames: a frame's H and W are 1..2^20");
            need(frame_fits(off, H, 3 * W, pitch, pitch, arena_bytes, 4), "ach_draw_detections_frames: a frame's extent passes the arena (offset and pitch are multiples of 4, pitch >= 3 W)");
            need(f[4] >= 1 && f[4] <= ach::DRAW_MAX_THICKNESS, "ach_draw_detections_frames: thickness is 1..64");
            need(f[5] >= 0 && f[5] <= num_labels - int64_t(num_classes) * ach::DRAW_SCORES, "ach_draw_detections_frames: a frame's atlas base passes the label table");
            blocks = std::max(blocks, ach::cdivl(W, ach::DRAW_TW) * ach::cdivl(H, ach::DRAW_TH));
        }
        need(blocks < (1L << 31), "ach_draw_detections_frames: a frame is too large");
        ach::DrawParams p{boxes, count, records, arena, reinterpret_cast<const long long*>(table_dev), labels_dev, blob_dev, style_dev, class_counts, max_det, num_classes};
        ACH_LAUNCH(ach::draw_prepare_kernel, dim3(unsigned(batch)), dim3(256), s, p);
        ACH_LAUNCH(ach::draw_tiles_kernel, dim3(unsigned(blocks), unsigned(batch)), dim3(256), s, p);
    });
}

// ---- the heat-map mode on served frames (k_heatmap.h): cell scores, the uint8 mask at every frame's own size with its range, and the colour-mapped blend over a base
// arena, in three launches (two without colour).  Stateless.  The host copy of the frame table is checked against every arena before anything is launched.
int ach_heatmap_frames(int32_t det_kind, int32_t R, int32_t num_det, int32_t batch, const void* det3, const void* det4, const void* det5, float* scores,
                       const uint8_t* base, int64_t base_bytes, const int64_t* table_host, const int64_t* table_dev, const uint8_t* cmap_dev, float alpha,
                       uint8_t* mask, int64_t mask_bytes, int32_t* stats, uint8_t* out, int64_t out_bytes, void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        need(det3 && det4 && det5 && scores && table_host && table_dev && mask && stats && batch > 0 && batch <= 65535 && mask_bytes >= 0, "ach_heatmap_frames");
        need(det_kind >= KIND_F32 && det_kind <= KIND_F16, "ach_heatmap_frames: det_kind is 0 (fp32), 1 (bf16) or 2 (fp16)");
        need(R >= 32 && R <= 16384 && R % 32 == 0, "ach_heatmap_frames: R is a multiple of 32");
        need(num_det >= 1 && num_det <= 4096, "ach_heatmap_frames: num_det is 1..4096");
        const int A = ach::heat_cells(R);
        if (A > ach::HEAT_MAX_CELLS) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_heatmap_frames: more than 4096 cells per frame (R above 416)"};
        need(aligned16(mask, out) && (reinterpret_cast<uintptr_t>(scores) & 3u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3u) == 0, "ach_heatmap_frames: the mask and out arenas are 16-byte aligned");
        const bool colour = out != nullptr;
        if (colour) {
            need(base && cmap_dev && base_bytes > 0 && base_bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 3u) == 0 && out_bytes >= 0,
                 "ach_heatmap_frames: colour needs the base arena (4-byte aligned, padded to 4 bytes), the colour map and the out arena");
            need(alpha >= 0.f && alpha <= 1.f, "ach_heatmap_frames: alpha lies in [0, 1]");
        }
        long blocks = 0;
        for (int b = 0; b < batch; ++b) {
            const int64_t* f = table_host + long(b) * ach::HEAT_TABLE_COLS;
            const int64_t H = f[1], W = f[2], y0 = f[4], x0 = f[5], nh = f[6], nw = f[7];
            need(dims_ok(H, W, SIZE_TOP), "ach_heatmap_frames: a frame's H and W are at least 1");
            need(nh >= 1 && nw >= 1 && y0 >= 0 && x0 >= 0 && nh <= R - y0 && nw <= R - x0, "ach_heatmap_frames: a frame's window leaves the network input");
            need(frame_fits(f[8], H, W, f[9], f[9], mask_bytes, 16), "ach_heatmap_frames: a frame's mask passes its arena (offset and pitch are multiples of 16, pitch >= W)");
            if (colour) {
                need(frame_fits(f[0], H, 3 * W, f[3], 3 * W, base_bytes), "ach_heatmap_frames: a frame's extent passes the base arena");
                need(frame_fits(f[10], H, 3 * W, f[11], f[11], out_bytes, 16), "ach_heatmap_frames: a coloured frame passes the out arena (offset and pitch are multiples of 16, pitch >= 3 W)");
                // in place: the frame is written where it is read, so it lies in `out` exactly as in `base`
                if (out == base) need(f[10] == f[0] && f[11] == f[3], "ach_heatmap_frames: in place, a frame's out offset and pitch are its base offset and pitch");
            }
            blocks = std::max(blocks, ach::cdivl(W, ach::HEAT_TW) * ach::cdivl(H, ach::HEAT_TH));
        }
        need(blocks < (1L << 31), "ach_heatmap_frames: a frame is too large");
        ach::HeatScoreParams sp{{det3, det4, det5}, scores, stats, R, num_det, A};
        by_kind(det_kind, [&](auto e) { ACH_LAUNCH(ach::heat_scores_kernel<typename decltype(e)::type>, dim3(unsigned(ach::cdivl(A, 256)), unsigned(batch)), dim3(256), s, sp); });
        ach::HeatParams p{scores, stats, base, reinterpret_cast<const long long*>(table_dev), cmap_dev, mask, out, R, A, alpha};
        ACH_LAUNCH(ach::heat_mask_kernel, dim3(unsigned(blocks), unsigned(batch)), dim3(256), s, p);
        if (colour) ACH_LAUNCH(ach::heat_colour_kernel, dim3(unsigned(blocks), unsigned(batch)), dim3(256), s, p);
    });
}

// ---- the picture of the radar point classes on served frames (k_scatter.h): the unique sorted (u, v, s, class) rows of every frame and their discs painted in place, in
// two launches.  Stateless.  The host copy of the frame table is checked against the arena and the cloud buffer before anything is launched; what comes from DEVICE
// data (indices, class ids, u, v, s) is bounded by the kernels themselves.
int ach_scatter_points_frames(uint8_t* arena, int64_t arena_bytes, const int64_t* table_host, const int64_t* table_dev, int32_t batch, const void* clouds,
                              int64_t cloud_elems, int32_t cloud_kind, const int64_t* indices_dev, const int64_t* point_class, int32_t num_points,
                              int32_t num_classes, const uint8_t* colours_dev, int32_t colour_mode, int32_t range_lo, int32_t range_hi, float alpha, double k,
                              int32_t max_radius, double* rows, int32_t* count, int32_t* class_range, double* discs, int64_t discs_bytes, int32_t* boxes,
                              int64_t boxes_bytes, void* stream) {
    return stateless(stream, [&](hipStream_t s) {
        need(arena && table_host && table_dev && clouds && point_class && colours_dev && rows && count && class_range && discs && boxes && batch > 0 && batch <= 65535 &&
             arena_bytes > 0 && cloud_elems >= 0 && (cloud_kind == ach::SCATTER_IN_F32 || cloud_kind == ach::SCATTER_IN_F64), "ach_scatter_points_frames");
        need(num_points >= 1, "ach_scatter_points_frames: num_points is 1..4096");
        if (num_points > ach::SCATTER_MAX_POINTS) throw ach::AchError{ACH_ERR_UNSUPPORTED, "ach_scatter_points_frames: more than 4096 points per frame"};
        need(num_classes >= 1 && num_classes <= ach::SCATTER_MAX_CLASSES, "ach_scatter_points_frames: num_classes is 1..256");
        need(colour_mode >= ach::SCATTER_CMAP_AUTO && colour_mode <= ach::SCATTER_PALETTE, "ach_scatter_points_frames: colour_mode is 0 (colour map), 1 (fixed range) or 2 (palette)");
        if (colour_mode == ach::SCATTER_CMAP_FIXED) need(range_lo >= 0 && range_lo <= range_hi && range_hi <= 255, "ach_scatter_points_frames: a fixed class range has 0 <= lo <= hi <= 255");
        need(alpha >= 0.f && alpha <= 1.f, "ach_scatter_points_frames: alpha lies in [0, 1]");
        need(max_radius >= 1 && max_radius <= ach::SCATTER_MAX_RADIUS, "ach_scatter_points_frames: max_radius is 1..256");
        need(std::isfinite(k) && k > 0.0, "ach_scatter_points_frames: k = size_scale^2 / 4 is finite and above 0");
        need((reinterpret_cast<uintptr_t>(arena) & 3u) == 0 && (reinterpret_cast<uintptr_t>(clouds) & (cloud_kind == ach::SCATTER_IN_F64 ? 7u : 3u)) == 0 &&
             ((reinterpret_cast<uintptr_t>(indices_dev) | reinterpret_cast<uintptr_t>(point_class) | reinterpret_cast<uintptr_t>(rows)) & 7u) == 0 &&
             ((reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(class_range)) & 3u) == 0,
             "ach_scatter_points_frames: the arena is 4-byte aligned, clouds, indices, classes and rows to their element size");
        const int64_t samples = int64_t(batch) * num_points;
        need(aligned16(discs, boxes) && discs_bytes >= samples * 32 && boxes_bytes >= samples * 16,
             "ach_scatter_points_frames: the workspaces are 16-byte aligned and hold 32 and 16 bytes per sample");
        long blocks = 0;
        for (int b = 0; b < batch; ++b) {
            const int64_t* f = table_host + long(b) * ach::SCATTER_TABLE_COLS;
            const int64_t off = f[0], H = f[1], W = f[2], pitch = f[3], coff = f[4], n = f[5], F = f[6], stride = f[7];
            need(dims_ok(H, W, 1L << 20), "ach_scatter_points_frames: a frame's H and W are 1..2^20");
            need(frame_fits(off, H, 3 * W, pitch, pitch, arena_bytes, 4), "ach_scatter_points_frames: a frame's extent passes the arena (offset and pitch are multiples of 4, pitch >= 3 W)");
            need(n >= 0 && n < (1L << 40) && F >= 1 && F < (1L << 20) && frame_fits(coff, n, F, stride, F, cloud_elems, 1, 1L << 20),
                 "ach_scatter_points_frames: a cloud's extent passes the cloud buffer");
            for (int c = 8; c < 11; ++c) need(f[c] >= 0 && f[c] < F, "ach_scatter_points_frames: a column index is not below F");
            blocks = std::max(blocks, ach::cdivl(W, ach::SCATTER_TW) * ach::cdivl(H, ach::SCATTER_TH));
        }
        need(blocks < (1L << 31), "ach_scatter_points_frames: a frame is too large");
        ach::ScatterParams p{clouds, reinterpret_cast<const long long*>(table_dev), reinterpret_cast<const long long*>(indices_dev), reinterpret_cast<const long long*>(point_class),
                             colours_dev, arena, rows, count, class_range, discs, boxes, k, double(max_radius) * double(max_radius), num_points,
                             ach::scatter_pow2(num_points), num_classes, cloud_kind, colour_mode, range_lo, range_hi, alpha};
        ACH_LAUNCH(ach::scatter_rows_kernel, dim3(unsigned(batch)), dim3(256), s, p);
        ACH_LAUNCH(ach::scatter_tiles_kernel, dim3(unsigned(blocks), unsigned(batch)), dim3(256), s, p);
    });
}

}  // extern "C"
