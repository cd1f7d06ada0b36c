// k_draw.h — the last step of the reference's detect_image (achelous.py:363-433) for a whole ragged batch: every kept detection's box outline, its filled label
// plate and the anti-aliased label text, drawn IN PLACE into the packed HWC uint8 overlay arena of k_serve.h, byte for byte what PIL's ImageDraw draws.
//
// Drawing is order-dependent (a later detection overwrites an earlier one, and the text is a blend of what lies under it), so a scatter per detection would race.
// Two launches instead, whatever the batch:
//   draw_prepare_kernel  one workgroup per frame: boxes / count -> one fixed-size integer record per detection (everything that depends on DEVICE data is bounded
//                        here: count is clamped to max_det, the class id is range-checked BEFORE it indexes anything, the label's hundredths are clamped to 0..100,
//                        coordinates are clamped before the float -> int conversion), and the per-class tally of the kept rows (the reference's count=True).
//   draw_tiles_kernel    one workgroup per DRAW_TW x DRAW_TH tile of a frame (grid = (largest frame's tiles, B); a smaller frame's surplus workgroups return at
//                        once, as in seg_overlay_frames_kernel).  It tests the frame's records against the tile (16 bytes per record: the clipped bounding box of
//                        everything the detection paints), keeps the survivors in LDS IN THEIR ORIGINAL ORDER and returns without touching memory if there are
//                        none.  Otherwise a thread owns four neighbouring pixels of a row, applies the surviving detections in order in registers — ring test,
//                        plate test, mask blend — and stores only its own bytes, and only if something painted them.
//
// Tables (host-built; the C entry ach_draw_detections_frames checks the host copies before anything is launched, the kernels trust them):
//   frame table int64 [B][8]: 0 byte offset of the frame in the arena (a multiple of 4), 1 H, 2 W, 3 pitch (>= 3 W, a multiple of 4), 4 ring thickness (1..64),
//                5 the frame's first entry in the label table (its font size's atlas), 6-7 unused.
//   label table int32 [L][7], entry base + class * 101 + hundredths: 0 byte offset of the glyph mask in the blob, 1 mask w, 2 mask h, 3 ox, 4 oy (where
//                font.getmask2 puts the mask relative to the text origin), 5 label w, 6 label h (textbbox(...)[2:4]).
//   style uint8 [1028]: class colours [256][3], skip flag per class [256], ink [3], pad.
//   record int32 [16] per (frame, detection): 0-3 x0, y0, x1, y1 of everything it paints, inclusive and clipped to the image (x1 < x0: nothing), 4-7 left, top,
//                right, bottom, 8-11 plate x0, y0, x1, y1 inclusive, 12-13 where the mask's first pixel goes, 14 label table entry, 15 colour r | g << 8 | b << 16.
//
// The rules (PIL 12, restated): ring i < thickness is the one-pixel border of [left + i, right - i] x [top + i, bottom - i], not drawn when it is empty — so a pixel is
// ring-coloured iff 0 <= min(x - left, right - x, y - top, bottom - y) < thickness.  ImageDraw's outline of a rectangle of height 0 (y0 == y1) also paints the row
// below at its two end columns (its vertical strokes run from y0 + 1 back to y1); that is reproduced.  The plate is filled with both corners inclusive.  The text is
// out = MULDIV255(dst, 255 - a) + MULDIV255(ink, a) per channel, MULDIV255(p, q) = ((t >> 8) + t) >> 8 with t = p * q + 128: integers only.
#pragma once
#include "ach_platform.h"

// tile of one workgroup: DRAW_TX threads of four pixels across, DRAW_TY rows; DRAW_TX * DRAW_TY = 256.  8 = 32 x 32 pixels, the fastest of 32 x 32, 64 x 16, 128 x 8 and
// 256 x 4 at 100 detections per full-HD frame and level with 64 x 16 at 5 (profiles/draw_timing.txt; the timing script takes libraries built with the other shapes)
#ifndef ACH_DRAW_TX
#define ACH_DRAW_TX 8
#endif

namespace ach {

constexpr int DRAW_TABLE_COLS = 8, DRAW_LABEL_COLS = 7, DRAW_REC = 16, DRAW_SCORES = 101;
constexpr int DRAW_MAX_DET = 1024, DRAW_MAX_CLASSES = 256, DRAW_MAX_THICKNESS = 64;
constexpr int DRAW_STYLE_BYTES = 1028, DRAW_STYLE_SKIP = 768, DRAW_STYLE_INK = 1024;
constexpr int DRAW_TX = ACH_DRAW_TX, DRAW_TY = 256 / DRAW_TX, DRAW_TW = 4 * DRAW_TX, DRAW_TH = DRAW_TY;
constexpr int DRAW_COORD_MAX = 1 << 24;          // |coordinate| bound before the float -> int conversion (frames are at most 2^20 pixels a side)
static_assert(DRAW_TX * DRAW_TY == 256 && DRAW_TX >= 1, "a draw tile is 256 threads");

struct DrawParams {
    const float* boxes; const int* count;      // [B, max_det, 7] = (y1, x1, y2, x2, obj, class conf, class id), [B]
    int* recs;                                  // [B, max_det, DRAW_REC]
    uint8_t* arena; const long long* table; const int* labels; const uint8_t* blob; const uint8_t* style;
    int* class_counts;                          // [B, num_classes] or null
    int max_det, num_classes;
};

__host__ __device__ __forceinline__ int draw_muldiv255(int p, int q) {
    const int t = p * q + 128;
    return ((t >> 8) + t) >> 8;
}
__host__ __device__ __forceinline__ int draw_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int draw_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ bool draw_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ int draw_floor(float v) {            // floor of a FINITE float, clamped to +-DRAW_COORD_MAX
    const float f = floorf(v);
    return f <= float(-DRAW_COORD_MAX) ? -DRAW_COORD_MAX : f >= float(DRAW_COORD_MAX) ? DRAW_COORD_MAX : int(f);
}
__device__ __forceinline__ int draw_count(const int* count, int b, int max_det) {
    const int n = count[b];
    return n < 0 ? 0 : n > max_det ? max_det : n;
}

static __global__ __launch_bounds__(256) void draw_prepare_kernel(const DrawParams p) {
    __shared__ int hist[DRAW_MAX_CLASSES];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    for (int c = tid; c < p.num_classes; c += 256) hist[c] = 0;
    __syncthreads();
    const long long* f = p.table + b * DRAW_TABLE_COLS;
    const int H = int(f[1]), W = int(f[2]), base = int(f[5]);
    const int n = draw_count(p.count, int(b), p.max_det);
    for (int j = tid; j < p.max_det; j += 256) {
        int r[DRAW_REC] = {0, 0, -1, -1, 0, 0, -1, -1, 0, 0, -1, -1, 0, 0, 0, 0};
        if (j < n) {
            const float* q = p.boxes + (b * p.max_det + j) * 7;
            const float id = q[6];
            if (id > -1.f && id < float(p.num_classes)) {                   // false for NaN: nothing below is indexed with an id outside [0, num_classes)
                const int c = int(id);
                atomicAdd(&hist[c], 1);
                bool ok = p.style[DRAW_STYLE_SKIP + c] == 0;
                ACH_UNROLL
                for (int k = 0; k < 6; ++k) ok = ok && draw_finite(q[k]);
                if (ok) {
                    const float score = q[4] * q[5];
                    double kd = rint(double(score) * 100.0);                // exact product, round half even: '{:.2f}'.format
                    kd = kd < 0.0 ? 0.0 : kd > 100.0 ? 100.0 : kd;
                    const int entry = base + c * DRAW_SCORES + int(kd);
                    const int* L = p.labels + long(entry) * DRAW_LABEL_COLS;
                    const int top = draw_max(0, draw_floor(q[0])), left = draw_max(0, draw_floor(q[1]));
                    const int bottom = draw_min(H, draw_floor(q[2])), right = draw_min(W, draw_floor(q[3]));
                    const int ox = left, oy = top - L[6] >= 0 ? top - L[6] : top + 1;
                    r[4] = left; r[5] = top; r[6] = right; r[7] = bottom;
                    r[8] = ox; r[9] = oy; r[10] = ox + L[5]; r[11] = oy + L[6];
                    r[12] = ox + L[3]; r[13] = oy + L[4]; r[14] = entry;
                    r[15] = int(p.style[3 * c]) | int(p.style[3 * c + 1]) << 8 | int(p.style[3 * c + 2]) << 16;
                    int x0 = r[8], y0 = r[9], x1 = r[10], y1 = r[11];        // the plate is never empty
                    if (L[1] > 0 && L[2] > 0) {
                        x0 = draw_min(x0, r[12]); y0 = draw_min(y0, r[13]); x1 = draw_max(x1, r[12] + L[1] - 1); y1 = draw_max(y1, r[13] + L[2] - 1);
                    }
                    if (right >= left && bottom >= top) {                   // + 1: the row below a ring of height 0
                        x0 = draw_min(x0, left); y0 = draw_min(y0, top); x1 = draw_max(x1, right); y1 = draw_max(y1, bottom + 1);
                    }
                    r[0] = draw_max(x0, 0); r[1] = draw_max(y0, 0); r[2] = draw_min(x1, W - 1); r[3] = draw_min(y1, H - 1);
                    if (r[3] < r[1]) { r[2] = -1; r[0] = 0; }
                }
            }
        }
        uint4* o = reinterpret_cast<uint4*>(p.recs + (b * p.max_det + j) * DRAW_REC);
        ACH_UNROLL
        for (int k = 0; k < 4; ++k) o[k] = make_uint4(uint32_t(r[4 * k]), uint32_t(r[4 * k + 1]), uint32_t(r[4 * k + 2]), uint32_t(r[4 * k + 3]));
    }
    if (p.class_counts) {
        __syncthreads();
        for (int c = tid; c < p.num_classes; c += 256) p.class_counts[b * p.num_classes + c] = hist[c];
    }
}

static __global__ __launch_bounds__(256) void draw_tiles_kernel(const DrawParams p) {
    __shared__ uint32_t hitw[DRAW_MAX_DET / 4];                               // one flag byte per record, summed four at a time
    unsigned char* hit = reinterpret_cast<unsigned char*>(hitw);
    __shared__ unsigned short list[DRAW_MAX_DET];
    __shared__ int nhit;
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const long long* f = p.table + b * DRAW_TABLE_COLS;
    const int H = int(f[1]), W = int(f[2]), thick = int(f[4]);
    const int ntx = (W + DRAW_TW - 1) / DRAW_TW, nty = (H + DRAW_TH - 1) / DRAW_TH;
    if (long(blockIdx.x) >= long(ntx) * nty) return;
    const int trow = int(blockIdx.x) / ntx, tx0 = (int(blockIdx.x) - trow * ntx) * DRAW_TW, ty0 = trow * DRAW_TH;
    const int tx1 = draw_min(tx0 + DRAW_TW, W) - 1, ty1 = draw_min(ty0 + DRAW_TH, H) - 1;
    const int n = draw_count(p.count, int(b), p.max_det);
    const int* recs = p.recs + b * p.max_det * DRAW_REC;
    if (tid == 0) nhit = 0;
    __syncthreads();
    for (int j = tid; j < n; j += 256) {
        const uint4 bb = *reinterpret_cast<const uint4*>(recs + j * DRAW_REC);
        const bool h = int(bb.x) <= tx1 && int(bb.z) >= tx0 && int(bb.y) <= ty1 && int(bb.w) >= ty0;
        hit[j] = h ? 1 : 0;
        if (h) atomicAdd(&nhit, 1);
    }
    __syncthreads();
    const int ns = nhit;
    if (ns == 0) return;                                                     // most tiles of most frames: nothing read but the records' boxes, nothing written
    for (int j = tid; j < n; j += 256) {                                     // order-preserving compaction without wave votes: a survivor's slot = survivors before it
        if (!hit[j]) continue;
        auto flags = [](uint32_t w) { return (w * 0x01010101u) >> 24; };       // flags are 0 / 1: the sum of a word's four
        uint32_t pos = flags(hitw[j >> 2] & ((1u << (8 * (j & 3))) - 1u));
        for (int i = 0; i < (j >> 2); ++i) pos += flags(hitw[i]);
        list[pos] = (unsigned short)j;
    }
    __syncthreads();
    const int x4 = tx0 + 4 * (tid % DRAW_TX), y = ty0 + tid / DRAW_TX;
    if (x4 >= W || y >= H) return;
    const int npx = W - x4 < 4 ? W - x4 : 4, nbytes = 3 * npx;
    uint8_t* row = p.arena + f[0] + long(y) * f[3] + 3L * x4;                // a multiple of 4: offset and pitch are, and 3 * x4 = 12 * (x4 / 4)
    uint32_t w[3] = {0u, 0u, 0u};
    ACH_UNROLL
    for (int k = 0; k < 3; ++k)
        if (4 * k < nbytes) w[k] = reinterpret_cast<const uint32_t*>(row)[k];  // inside the row's pitch (pitch >= 3 W, a multiple of 4)
    int px[12];
    ACH_UNROLL
    for (int k = 0; k < 12; ++k) px[k] = int((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    const int ink[3] = {p.style[DRAW_STYLE_INK], p.style[DRAW_STYLE_INK + 1], p.style[DRAW_STYLE_INK + 2]};
    bool touched = false;
    for (int s = 0; s < ns; ++s) {
        const int* r = recs + wave_uniform(int(list[s])) * DRAW_REC;
        if (y < r[1] || y > r[3] || x4 > r[2] || x4 + 3 < r[0]) continue;
        const int left = r[4], top = r[5], right = r[6], bottom = r[7];
        const int* L = p.labels + long(r[14]) * DRAW_LABEL_COLS;
        const int mw = L[1], mh = L[2], my = y - r[13];
        const int col[3] = {r[15] & 0xff, (r[15] >> 8) & 0xff, (r[15] >> 16) & 0xff};
        const int dy = draw_min(y - top, bottom - y), hh = bottom - top;
        const bool in_plate_y = y >= r[9] && y <= r[11];
        // the row below a ring of height 0 (ring i = hh / 2, if it is one of the `thick` rings and not empty across): its two end columns
        const int qi = hh >> 1;
        const bool quirk = hh >= 0 && !(hh & 1) && qi < thick && right - qi >= left + qi && y == top + qi + 1;
        ACH_UNROLL
        for (int i = 0; i < 4; ++i) {
            if (i >= npx) break;
            const int x = x4 + i;
            const int d = draw_min(draw_min(x - left, right - x), dy);
            if ((d >= 0 && d < thick) || (quirk && (x == left + qi || x == right - qi)) || (in_plate_y && x >= r[8] && x <= r[10])) {
                px[3 * i] = col[0]; px[3 * i + 1] = col[1]; px[3 * i + 2] = col[2];
                touched = true;
            }
            const int mx = x - r[12];
            if (my >= 0 && my < mh && mx >= 0 && mx < mw) {
                const int a = p.blob[L[0] + long(my) * mw + mx];
                ACH_UNROLL
                for (int ch = 0; ch < 3; ++ch) px[3 * i + ch] = draw_muldiv255(px[3 * i + ch], 255 - a) + draw_muldiv255(ink[ch], a);
                touched = true;
            }
        }
    }
    if (!touched) return;
    if (npx == 4) {
        ACH_UNROLL
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<uint32_t*>(row)[k] = uint32_t(px[4 * k]) | uint32_t(px[4 * k + 1]) << 8 | uint32_t(px[4 * k + 2]) << 16 | uint32_t(px[4 * k + 3]) << 24;
    } else {                                                                 // the row's last, partial group: its own bytes only
        ACH_UNROLL
        for (int k = 0; k < 9; ++k)
            if (k < nbytes) row[k] = uint8_t(px[k]);
    }
}

}  // namespace ach
