// k_nmswide.h — class-aware NMS on the device for more anchors than nms_kernel (k_detect.h) holds in one workgroup's registers and
// LDS: NMS_MAXA < A <= NMSW_MAXA (448 x 448 .. 864 x 864).  Same contract: for identical decoded inputs the kept-anchor sequence,
// the rows and the count equal oracle/nms.py (torchvision 0.12.0 `batched_nms`, CUDA rule) bit for bit.
//
// Two launches:
//   nms_wide_filter_kernel  grid (tiles of 1024 anchors, B), a thread per anchor: step 1 of nms_kernel (xywh->xyxy, class max with
//                           torch.max's NaN rule, obj * cls >= conf), a block scan that compacts the tile's candidates in anchor order
//                           into the tile's own 1024 slots of the workspace, the tile's candidate count and coordinate maximum.
//                           No atomics: every word has one writer, so a frame's result does not depend on the batch it sits in.
//   nms_wide_kernel         one workgroup per image: scans the <= 15 tile counts, builds the 64-bit keys (score | slot), sorts them
//                           in LDS (bitonic, up to 16384 keys = 128 KiB), chooses torchvision's rule from the candidate count, writes
//                           the sorted boxes (and class ids) and runs the greedy suppression of nms_kernel's step 5, 64 candidates a round.
// A slot is tile * 1024 + position in the tile: slots rise with the anchor index, so "ties to the lower slot" is "ties to the lower
// anchor", and the second compaction (tiles -> one dense list) happens only in the keys' positions, never in memory.
#pragma once
#include "k_detect.h"

namespace ach {

constexpr int NMSW_TILE = 1024;             // anchors per tile of the first launch; threads per workgroup of both launches
constexpr int NMSW_MAXTILES = 15;
constexpr int NMSW_MAXA = 15309;            // 864 x 864: 108^2 + 54^2 + 27^2 anchors
constexpr int NMSW_IDX_BITS = 14;           // index field of a sort key: a slot is < NMSW_MAXTILES * NMSW_TILE = 15360 < 2^14
constexpr int NMSW_KEYS = 1 << NMSW_IDX_BITS;   // keys the LDS sort holds (the candidate count rounded up to a power of two)
constexpr int NMSW_LDS_BOXES = 4096;        // up to this many candidates the sorted boxes live in LDS behind the keys, above it in global scratch
constexpr int NMSW_TRICK_MAX = 5000;        // torchvision: boxes.numel() > 20000 (more than 5000 boxes) -> per-class NMS
static_assert(NMSW_MAXTILES * NMSW_TILE <= NMSW_KEYS && NMSW_MAXA <= NMSW_MAXTILES * NMSW_TILE, "slot index must fit the key's index field");
static_assert(NMSW_LDS_BOXES * 8 + NMSW_LDS_BOXES * 16 <= NMSW_KEYS * 8, "keys + boxes of the small case must fit the key buffer");

struct NmsWideParams {
    const float* dec;           // [B, A, NC5] decoded predictions (cx, cy, w, h, obj, cls...)
    float* rec;                 // [B, tiles * 1024, 8] candidate records by slot: x1, y1, x2, y2 (un-offset), score, cls_conf, obj, cls_id
    int* rec_anchor;            // [B, tiles * 1024] slot -> anchor index
    int* tile_cnt;              // [B, 16] candidates per tile
    float* tile_max;            // [B, 16] largest candidate coordinate per tile
    float* sbox;                // [B, A, 4] sorted candidate boxes when more than NMSW_LDS_BOXES pass the filter
    int* scls;                  // [B, A] sorted class ids (per-class rule only)
    float* rows; int* kept; int* count;   // [B, max_det, 7], [B, max_det], [B]
    int B, A, NC5, num_classes, max_det, tiles; float conf, iou;
};

static __global__ __launch_bounds__(NMSW_TILE) void nms_wide_filter_kernel(const NmsWideParams p) {
    __shared__ int scan[NMSW_TILE];
    __shared__ float redf[NMSW_TILE];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int a = tile * NMSW_TILE + tid;
    // ---- per-anchor box / score / filter: the arithmetic of nms_kernel's step 1, operation for operation
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, score = 0.f, conf = 0.f, obj = 0.f;
    int cls = 0, flag = 0;
    float mymax = -3.0e38f;
    if (a < p.A) {
        const float* r = p.dec + (long(b) * p.A + a) * p.NC5;
        const float hw = __fdiv_rn(r[2], 2.0f), hh = __fdiv_rn(r[3], 2.0f);
        x1 = __fsub_rn(r[0], hw); y1 = __fsub_rn(r[1], hh);
        x2 = __fadd_rn(r[0], hw); y2 = __fadd_rn(r[1], hh);
        float best = r[5]; int bi = 0;
        // torch.max over the classes propagates NaN: the first NaN wins and stays, the score becomes NaN and the filter drops the anchor
        for (int c = 1; c < p.num_classes; ++c) if (best == best && !(r[5 + c] <= best)) { best = r[5 + c]; bi = c; }
        conf = best; cls = bi; obj = r[4];
        score = __fmul_rn(r[4], best);
        flag = score >= p.conf ? 1 : 0;
        if (flag) mymax = fmaxf(fmaxf(x1, y1), fmaxf(x2, y2));
    }
    // ---- inclusive scan of the flags (stable compaction inside the tile) + the tile's coordinate maximum
    scan[tid] = flag;
    redf[tid] = mymax;
    __syncthreads();
    for (int off = 1; off < NMSW_TILE; off <<= 1) {
        const int v = tid >= off ? scan[tid - off] : 0;
        const float m = tid >= off ? redf[tid - off] : -3.0e38f;
        __syncthreads();
        scan[tid] += v;
        redf[tid] = fmaxf(redf[tid], m);
        __syncthreads();
    }
    if (flag) {
        const long slot = (long(b) * p.tiles + tile) * NMSW_TILE + (scan[tid] - 1);
        float* q = p.rec + slot * 8;
        q[0] = x1; q[1] = y1; q[2] = x2; q[3] = y2;
        q[4] = score; q[5] = conf; q[6] = obj; q[7] = float(cls);
        p.rec_anchor[slot] = a;
    }
    if (tid == NMSW_TILE - 1) {
        p.tile_cnt[b * 16 + tile] = scan[tid];
        p.tile_max[b * 16 + tile] = redf[tid];
    }
}

static __global__ __launch_bounds__(NMSW_TILE) void nms_wide_kernel(const NmsWideParams p) {
    alignas(16) __shared__ unsigned long long keybuf[NMSW_KEYS];    // sort keys; the upper part holds the sorted boxes of up to NMSW_LDS_BOXES candidates
    __shared__ unsigned char supp[NMSW_KEYS];
    __shared__ float4 cbox[64];                                     // the round's 64 candidates: box, area, class
    __shared__ float carea[64];
    __shared__ int ccls[64];
    __shared__ unsigned char pm[64][16];                            // 4 pair bits per entry
    __shared__ unsigned long long s_keep;
    __shared__ unsigned long long s_keepc[64];                      // the round's kept candidates by class (num_det <= 59); under the trick rule all in [0]
    __shared__ int s_base[NMSW_MAXTILES + 1];
    __shared__ float s_max;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const long slots = long(p.tiles) * NMSW_TILE;
    const float* dec = p.dec + long(b) * p.A * p.NC5;
    const float* rec = p.rec + long(b) * slots * 8;
    const int* ranchor = p.rec_anchor + long(b) * slots;
    // ---- 2. the tiles' counts -> each tile's base in the dense candidate list; the image's coordinate maximum (max is exact in any order)
    if (tid == 0) {
        int acc = 0;
        float m = -3.0e38f;
        for (int t = 0; t < p.tiles; ++t) { s_base[t] = acc; acc += p.tile_cnt[b * 16 + t]; m = fmaxf(m, p.tile_max[b * 16 + t]); }
        s_base[p.tiles] = acc;
        s_max = m;
    }
    __syncthreads();
    const int n = s_base[p.tiles];
    const float max1 = __fadd_rn(s_max, 1.0f);
    // ---- rule choice, as torchvision's batched_nms makes it from boxes.numel() = 4 * n:
    //   4 n <= 20000  the coordinate trick: one NMS over boxes + float(cls) * (max + 1)
    //   otherwise     per class ("vanilla"): each class is suppressed on its own un-offset boxes and the survivors are re-sorted by score,
    //                 stable.  One greedy pass in global score order in which a pair can suppress only when both class ids are equal keeps
    //                 exactly the per-class loops' survivors (a candidate's fate depends on the earlier kept candidates of its own class only,
    //                 and those come in the same relative order), and it emits them in descending score with ties to the lower candidate
    //                 index, which is what the stable re-sort of the ascending kept indices gives.
    const bool trick = n <= NMSW_TRICK_MAX;
    int npow = 1;
    while (npow < n) npow <<= 1;
    // ---- 3. keys: descending score, ties to the lower slot (= lower anchor); dense position = tile base + position in the tile
    for (int i = n + tid; i < npow; i += NMSW_TILE) keybuf[i] = ~0ull;
    for (int t = 0; t < p.tiles; ++t) {
        const int base = s_base[t];
        if (tid < s_base[t + 1] - base) {
            const int s = t * NMSW_TILE + tid;
            keybuf[base + tid] = ((unsigned long long)(~order_encode(rec[long(s) * 8 + 4])) << 32) | unsigned(s);
        }
    }
    __syncthreads();
    // bitonic sort, ascending keys; a thread takes whole compare-exchange pairs
    for (int k = 2; k <= npow; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (npow >> 1); t += NMSW_TILE) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), ixj = i | j;
                const unsigned long long x = keybuf[i], y = keybuf[ixj];
                const bool up = (i & k) == 0;
                if ((x > y) == up) { keybuf[i] = y; keybuf[ixj] = x; }
            }
            __syncthreads();
        }
    // ---- 4. sorted boxes (offset under the trick rule; with their class ids under the per-class rule): behind the keys in LDS when they
    // fit, else in global scratch (at most 245 KB per image, L2-resident).  The keys stay: their low bits are the sorted order.
    constexpr unsigned long long SLOT_MASK = (1ull << NMSW_IDX_BITS) - 1ull;
    float4* sbox = n <= NMSW_LDS_BOXES ? reinterpret_cast<float4*>(keybuf + NMSW_LDS_BOXES) : reinterpret_cast<float4*>(p.sbox) + long(b) * p.A;
    int* scls = p.scls + long(b) * p.A;
    for (int i = tid; i < n; i += NMSW_TILE) {
        const float* q = rec + long(keybuf[i] & SLOT_MASK) * 8;
        supp[i] = 0;
        if (trick) {
            const float off = __fmul_rn(q[7], max1);
            sbox[i] = make_float4(__fadd_rn(q[0], off), __fadd_rn(q[1], off), __fadd_rn(q[2], off), __fadd_rn(q[3], off));
        } else {
            sbox[i] = make_float4(q[0], q[1], q[2], q[3]);
            scls[i] = int(q[7]);
        }
    }
    __syncthreads();
    // ---- 5. greedy suppression in sorted order, 64 candidates per round, as nms_kernel's step 5 with the round's candidates staged in LDS:
    //   s. the first 64 threads: the round's boxes, areas and classes into LDS
    //   a. all threads: the 64x64 "row suppresses column" bits inside the chunk (4 pairs per thread)
    //   b. wave 0: lane l assembles row l's mask; the greedy pass over the chunk runs in registers; kept candidates write their output rows
    //   c. all threads: every later, still-alive candidate is tested against the boxes the chunk kept (of its class, under the per-class rule)
    int kept_total = 0;                             // same value in every thread
    for (int c0 = 0; c0 < n && kept_total < p.max_det; c0 += 64) {
        if (tid < 64) {   // s.
            const int i = c0 + tid;
            if (i < n) {
                const float4 bi = sbox[i];
                cbox[tid] = bi;
                carea[tid] = __fmul_rn(__fsub_rn(bi.z, bi.x), __fsub_rn(bi.w, bi.y));
                ccls[tid] = trick ? 0 : scls[i];
            }
        }
        __syncthreads();
        {   // a.
            const int row = tid >> 4, cb = (tid & 15) * 4;
            const int i = c0 + row;
            unsigned bits = 0;
            if (i < n && supp[i] == 0) {
                const float4 bi = cbox[row];
                const float ai = carea[row];
                const int ci = ccls[row];
                ACH_UNROLL
                for (int e = 0; e < 4; ++e) {
                    const int col = cb + e, j = c0 + col;
                    if (col > row && j < n && ccls[col] == ci && nms_overlaps(bi, ai, cbox[col], p.iou)) bits |= 1u << e;
                }
            }
            pm[row][tid & 15] = (unsigned char)bits;
        }
        __syncthreads();
        if (tid < 64) {   // b.
            const int i = c0 + tid;
            const bool alive = i < n && supp[i] == 0;
            unsigned long long m = 0;
            ACH_UNROLL
            for (int q = 0; q < 16; ++q) m |= (unsigned long long)(pm[tid][q]) << (4 * q);
            const unsigned long long alive_bits = wave_ballot64(alive);
            unsigned long long removed = ~alive_bits, keep = 0;
            for (int l = 0; l < 64; ++l) {
                const unsigned long long ml = wave_read64(m, l);
                if (!((removed >> l) & 1ull)) { keep |= 1ull << l; removed |= ml; }
            }
            if (tid == 0) s_keep = keep;
            // the kept candidates split by class: a later candidate then walks the kept boxes of its own class only (lanes of a wave hold different
            // classes, so a class test inside that walk would skip nothing)
            const bool mine = (keep >> tid) & 1ull;
            const int nc = trick ? 1 : p.num_classes;
            for (int c = 0; c < nc; ++c) {
                const unsigned long long mc = wave_ballot64(mine && ccls[tid] == c);
                if (tid == 0) s_keepc[c] = mc;
            }
            if (mine) {
                const int slot = kept_total + __popcll(keep & ((1ull << tid) - 1ull));
                if (slot < p.max_det) {
                    const int s = int(keybuf[i] & SLOT_MASK);
                    const float* q = rec + long(s) * 8;
                    float* r = p.rows + (long(b) * p.max_det + slot) * 7;
                    // the corners are recomputed from the decoded row, as the reference gathers them
                    const int a = ranchor[s];
                    const float* d = dec + long(a) * p.NC5;
                    const float hw = __fdiv_rn(d[2], 2.0f), hh = __fdiv_rn(d[3], 2.0f);
                    r[0] = __fsub_rn(d[0], hw); r[1] = __fsub_rn(d[1], hh); r[2] = __fadd_rn(d[0], hw); r[3] = __fadd_rn(d[1], hh);
                    r[4] = q[6]; r[5] = q[5]; r[6] = q[7];
                    p.kept[long(b) * p.max_det + slot] = a;
                }
            }
        }
        __syncthreads();
        const unsigned long long keep = s_keep;
        kept_total += __popcll(keep);
        for (int j = c0 + 64 + tid; j < n; j += NMSW_TILE) {   // c.
            if (supp[j]) continue;
            const float4 bj = sbox[j];
            unsigned long long k = s_keepc[trick ? 0 : scls[j]];
            while (k) {
                const int l = __ffsll((long long)k) - 1;
                k &= k - 1ull;
                if (nms_overlaps(cbox[l], carea[l], bj, p.iou)) { supp[j] = 1; break; }
            }
        }
        __syncthreads();
    }
    // unused output slots: zero rows, index -1 (the caller hands over uninitialised buffers; kept_total is uniform)
    for (int slot = (kept_total < p.max_det ? kept_total : p.max_det) + tid; slot < p.max_det; slot += NMSW_TILE) {
        float* r = p.rows + (long(b) * p.max_det + slot) * 7;
        ACH_UNROLL
        for (int c = 0; c < 7; ++c) r[c] = 0.f;
        p.kept[long(b) * p.max_det + slot] = -1;
    }
    if (tid == 0) p.count[b] = kept_total < p.max_det ? kept_total : p.max_det;
}

}  // namespace ach
