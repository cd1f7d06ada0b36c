// k_scatter.h — the picture of the radar point classes the reference's detect_image makes (achelous.py:261-271) for a whole ragged batch: per frame the table
// np.unique(concat[u, v, rcs, class], axis=0) of the sampled points, and every row of it painted as a disc in its class colour IN PLACE into a packed HWC uint8 arena
// (the overlay arena of k_serve.h), later rows over earlier ones.  Two launches whatever the batch, no host read, no float atomics; the result depends neither on the
// launch geometry nor on the batch a frame sits in.
//
//   scatter_rows_kernel   one workgroup per frame (N <= SCATTER_MAX_POINTS sampled points).  Gathers (u, v, s, c) through the frame's cloud table and the index array
//                         (identity without one), drops a row whose index is outside [0, n) — nothing is read for it —, whose u, v or s is not finite or whose class is
//                         outside [0, num_classes), sorts the rest ascending by (u, v, s, c) BY VALUE (-0.0 == 0.0; rows equal in all four fields are ordered by their
//                         sample position, so the output is one fixed sequence) with a bitonic sort of 16-bit row ids in LDS whose comparator reads u from LDS and the
//                         other fields only on a tie, removes equal rows, and writes: rows float64 [B][N][4] (rows past the count zero), count, the classes' (lo, hi),
//                         and per kept row the record launch 2 paints from — `discs` float64 [B][N][4] = (u, v, r2, colour r | g << 8 | b << 16; r2 = -1: covers
//                         nothing) and `boxes` int32 [B][N][4] = the disc's bounding box clipped to the frame, inclusive (x1 < x0: nothing).  `discs` doubles as the
//                         scratch the unsorted rows are gathered into.
//   scatter_tiles_kernel  one workgroup per SCATTER_TW x SCATTER_TH tile of a frame (grid = (largest frame's tiles, B); surplus workgroups return at once).  It walks
//                         the frame's records that can reach its columns (they are sorted by u: two binary searches) in chunks of 256: a thread tests one record's box
//                         against the tile, the hits are compacted IN ORDER into LDS (wave ballot and prefix, wave offsets through LDS) with their (u, v, r2, colour),
//                         and every pixel applies the chunk's list in order before the next chunk is
//                         culled — the list is bounded and the order kept by construction.  A thread owns four neighbouring pixels of a row (three aligned dwords: tile
//                         origin, frame offset and pitch are multiples of 4) and stores them only if a disc covered one; a partial last group stores its own bytes.
//
//   frame table int64 [B][16]: 0 byte offset of the frame in the arena (a multiple of 4), 1 H, 2 W, 3 pitch (>= 3 W, a multiple of 4), 4 element offset of the frame's
//                cloud, 5 n (its rows), 6 F (columns per row), 7 row stride in elements (>= F), 8 / 9 / 10 the columns of u, v and s (the marker size: rcs), 11-15 unused.
//
// The rules.  Coverage: pixel (x, y), centre at integer coordinates, is covered iff s > 0 and dx * dx + dy * dy <= r2, dx = x - u, dy = y - v, r2 = min(k * s, r2max),
// every operation ONE rounded float64 operation, never contracted.  Colour: mode 0 = table[idx], idx = 0 when hi == lo else min(((c - lo) * 256) / (hi - lo), 255) in
// integers over the frame's own (lo, hi) — matplotlib's Normalize and a 256-entry colour map; mode 1 = the same over a fixed (lo, hi), ids clamped to it; mode 2 =
// table[c], a per-class palette.  Paint: per channel (uint8)(p + alpha * (colour - p)) in float32, not contracted (PIL's Image.blend: serve_mix of k_serve.h).
//
// u, v and s are DEVICE data the host never sees: a row leaves on NaN / inf before anything is converted, the bounding box is computed from values already tested in
// double against the frame (a centre further than the radius from it gives an empty box), every loop is bounded by N or the tile, every index is range-tested against
// n.  The C entry (api_frames.cpp ach_scatter_points_frames, declared in include/achelous_points.h) checks the host copy of the table before the first launch.
#pragma once
#include "ach_platform.h"
#include "k_serve.h"       // serve_mix

// rows of pixels per thread of the tile kernel: the tile is 64 x (16 * ACH_SCATTER_RY) pixels (profiles/scatter_timing.txt)
#ifndef ACH_SCATTER_RY
#define ACH_SCATTER_RY 2
#endif

namespace ach {

constexpr int SCATTER_TABLE_COLS = 16;
constexpr int SCATTER_MAX_POINTS = 4096, SCATTER_MAX_CLASSES = 256, SCATTER_MAX_RADIUS = 256;
constexpr int SCATTER_RY = ACH_SCATTER_RY, SCATTER_TW = 64, SCATTER_TH = 16 * SCATTER_RY, SCATTER_CHUNK = 256;
constexpr int SCATTER_NONE = 0xffff;               // a sort slot without a row: padding to the power of two, and dropped rows; sorts last
enum ScatterIn : int { SCATTER_IN_F32 = 0, SCATTER_IN_F64 = 1 };
enum ScatterColour : int { SCATTER_CMAP_AUTO = 0, SCATTER_CMAP_FIXED = 1, SCATTER_PALETTE = 2 };

struct ScatterParams {
    const void* clouds; const long long* table; const long long* indices; const long long* cls;   // indices: null = row j of the cloud is sample j
    const uint8_t* colours;                     // uint8 [256][3]
    uint8_t* arena;
    double* rows; int* count; int* range; double* discs; int* boxes;
    double k, r2max;
    int N, P, num_classes, kind, mode, flo, fhi;
    float alpha;
};

__host__ __device__ __forceinline__ int scatter_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
__host__ __device__ __forceinline__ bool scatter_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }      // false for NaN
// min(k * s, r2max), the product rounded once; the caller has s > 0
__host__ __device__ __forceinline__ double scatter_r2(double k, double s, double r2max) {
#pragma clang fp contract(off)
    const double t = k * s;
    return t < r2max ? t : r2max;
}
// dx * dx + dy2 <= r2 with dx = x - u: three rounded operations
__host__ __device__ __forceinline__ bool scatter_covers(double x, double u, double dy2, double r2) {
#pragma clang fp contract(off)
    const double dx = x - u;
    const double dx2 = dx * dx;
    const double d = dx2 + dy2;
    return d <= r2;
}
__host__ __device__ __forceinline__ double scatter_dy2(double y, double v) {
#pragma clang fp contract(off)
    const double dy = y - v;
    return dy * dy;
}
// matplotlib's Normalize(lo, hi) and a 256-entry map, in integers; lo <= c <= hi
__host__ __device__ __forceinline__ int scatter_index(int c, int lo, int hi) {
    if (hi <= lo) return 0;
    const int i = ((c - lo) * 256) / (hi - lo);
    return i > 255 ? 255 : i;
}
__device__ __forceinline__ double scatter_ld(const void* clouds, int kind, long i) {
    return kind == SCATTER_IN_F64 ? static_cast<const double*>(clouds)[i] : double(static_cast<const float*>(clouds)[i]);
}
// strict order of two sort slots: rows by (u, v, s, c) by value, equal rows by sample position, empty slots last.  ukey: u per sample in LDS, raw: (u, v, s, c) per sample
__device__ __forceinline__ bool scatter_less(int a, int b, const double* ukey, const double* raw) {
    if (a == b || a == SCATTER_NONE) return false;
    if (b == SCATTER_NONE) return true;
    const double ua = ukey[a], ub = ukey[b];
    if (ua != ub) return ua < ub;
    const double* ra = raw + 4L * a;
    const double* rb = raw + 4L * b;
    ACH_UNROLL
    for (int f = 1; f < 4; ++f)
        if (ra[f] != rb[f]) return ra[f] < rb[f];
    return a < b;
}
__device__ __forceinline__ bool scatter_same(int a, int b, const double* raw) {
    const double* ra = raw + 4L * a;
    const double* rb = raw + 4L * b;
    return ra[0] == rb[0] && ra[1] == rb[1] && ra[2] == rb[2] && ra[3] == rb[3];
}

static __global__ __launch_bounds__(256) void scatter_rows_kernel(const ScatterParams p) {
    __shared__ double ukey[SCATTER_MAX_POINTS];                              // 32 KB
    __shared__ unsigned short ids[SCATTER_MAX_POINTS];                       // 8 KB
    __shared__ int scan[256];
    __shared__ int s_hi, s_nlo;
    const int tid = threadIdx.x, N = p.N, P = p.P;                           // P: the power of two >= N, <= SCATTER_MAX_POINTS (the C entry computes it)
    const long b = blockIdx.x;
    const long long* f = p.table + b * SCATTER_TABLE_COLS;
    const int H = int(f[1]), W = int(f[2]);
    const long off = f[4], n = f[5], stride = f[7], cu = f[8], cv = f[9], cs = f[10];
    double* raw = p.discs + b * N * 4;
    double* rows = p.rows + b * N * 4;
    if (tid == 0) { s_hi = 0; s_nlo = 0; }
    for (int j = tid; j < P; j += 256) {
        int id = SCATTER_NONE;
        if (j < N) {
            const long long row = p.indices ? p.indices[b * N + j] : (long long)j;
            const long long c = p.cls[b * N + j];
            if (row >= 0 && row < n && c >= 0 && c < p.num_classes) {        // a bad index or class id: the row is dropped, nothing is read
                const long r = off + long(row) * stride;
                const double u = scatter_ld(p.clouds, p.kind, r + cu), v = scatter_ld(p.clouds, p.kind, r + cv), s = scatter_ld(p.clouds, p.kind, r + cs);
                if (scatter_finite(u) && scatter_finite(v) && scatter_finite(s)) {
                    id = j;
                    ukey[j] = u;
                    raw[4 * j] = u; raw[4 * j + 1] = v; raw[4 * j + 2] = s; raw[4 * j + 3] = double(int(c));
                }
            }
        }
        ids[j] = (unsigned short)id;
    }
    __syncthreads();                                                         // (also orders the gathered rows in global memory before the comparator reads them)
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int x = i ^ j;
                if (x > i) {
                    const int a = ids[i], c = ids[x];
                    const bool up = (i & k) == 0;
                    if (up ? scatter_less(c, a, ukey, raw) : scatter_less(a, c, ukey, raw)) { ids[i] = (unsigned short)c; ids[x] = (unsigned short)a; }
                }
            }
            __syncthreads();
        }
    // the kept positions: a row that differs from the one before it.  A thread owns `per` neighbouring positions; their count goes through a scan over the threads
    const int per = P >= 256 ? P / 256 : 1, i0 = tid * per;
    unsigned keep = 0;
    int mine = 0, hi = 0, nlo = 0;
    for (int q = 0; q < per; ++q) {
        const int i = i0 + q;
        if (i >= P) break;
        const int id = ids[i];
        if (id == SCATTER_NONE || (i > 0 && scatter_same(id, ids[i - 1], raw))) continue;
        keep |= 1u << q;
        ++mine;
        const int c = int(raw[4L * id + 3]);
        hi = c > hi ? c : hi;
        nlo = 255 - c > nlo ? 255 - c : nlo;
    }
    scan[tid] = mine;
    if (mine) { atomicMax(&s_hi, hi); atomicMax(&s_nlo, nlo); }
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const int total = scan[255];
    int pos = scan[tid] - mine;
    for (int q = 0; q < per; ++q) {
        if (!(keep >> q & 1u)) continue;
        const double* r = raw + 4L * ids[i0 + q];
        ACH_UNROLL
        for (int k = 0; k < 4; ++k) rows[4L * pos + k] = r[k];
        ++pos;
    }
    __syncthreads();                                                         // the sorted rows are written and every read of the scratch is done: `discs` becomes the records
    const int lo = total ? 255 - s_nlo : 0, top = total ? s_hi : 0;
    if (tid == 0) { p.count[b] = total; p.range[2 * b] = lo; p.range[2 * b + 1] = top; }
    int* boxes = p.boxes + b * N * 4;
    for (int j = tid; j < N; j += 256) {
        if (j >= total) {
            ACH_UNROLL
            for (int k = 0; k < 4; ++k) rows[4L * j + k] = 0.0;
            continue;
        }
        const double u = rows[4L * j], v = rows[4L * j + 1], s = rows[4L * j + 2];
        const int c = int(rows[4L * j + 3]);
        int idx;
        if (p.mode == SCATTER_PALETTE) idx = c;
        else if (p.mode == SCATTER_CMAP_FIXED) idx = scatter_index(c < p.flo ? p.flo : c > p.fhi ? p.fhi : c, p.flo, p.fhi);
        else idx = scatter_index(c, lo, top);
        const double colour = double(int(p.colours[3 * idx]) | int(p.colours[3 * idx + 1]) << 8 | int(p.colours[3 * idx + 2]) << 16);
        double r2 = -1.0;
        int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
        if (s > 0.0) {
            r2 = scatter_r2(p.k, s, p.r2max);
            // the box: every covered pixel has |dx|, |dy| <= sqrt(r2) (1 + 2^-51) < ri - 1, whatever the last bit of the device's sqrt.  u and v are tested in
            // double against the frame before they become integers
            const int ri = int(sqrt(r2)) + 2;                               // r2 <= r2max <= 2^16
            if (u >= -double(ri) - 1.0 && u <= double(W) + double(ri) && v >= -double(ri) - 1.0 && v <= double(H) + double(ri)) {
                const int fu = int(floor(u)), fv = int(floor(v));
                x0 = fu - ri < 0 ? 0 : fu - ri; x1 = fu + 1 + ri > W - 1 ? W - 1 : fu + 1 + ri;
                y0 = fv - ri < 0 ? 0 : fv - ri; y1 = fv + 1 + ri > H - 1 ? H - 1 : fv + 1 + ri;
                if (y1 < y0 || x1 < x0) { x0 = 0; x1 = -1; }
            }
        }
        double* d = p.discs + (b * N + j) * 4;
        d[0] = u; d[1] = v; d[2] = r2; d[3] = colour;
        *reinterpret_cast<uint4*>(boxes + 4L * j) = make_uint4(uint32_t(x0), uint32_t(y0), uint32_t(x1), uint32_t(y1));
    }
}

static __global__ __launch_bounds__(256) void scatter_tiles_kernel(const ScatterParams p) {
    __shared__ double rec[SCATTER_CHUNK * 4];                                // the chunk's hits, in order: u, v, r2, colour
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = p.N;
    const long b = blockIdx.y;
    const long long* f = p.table + b * SCATTER_TABLE_COLS;
    const int H = int(f[1]), W = int(f[2]);
    const int ntx = (W + SCATTER_TW - 1) / SCATTER_TW, nty = (H + SCATTER_TH - 1) / SCATTER_TH;
    if (long(blockIdx.x) >= long(ntx) * nty) return;                         // (the whole workgroup: the grid is sized for the batch's largest frame)
    const int trow = int(blockIdx.x) / ntx, tx0 = (int(blockIdx.x) - trow * ntx) * SCATTER_TW, ty0 = trow * SCATTER_TH;
    const int tx1 = (tx0 + SCATTER_TW < W ? tx0 + SCATTER_TW : W) - 1, ty1 = (ty0 + SCATTER_TH < H ? ty0 + SCATTER_TH : H) - 1;
    int total = p.count[b];
    total = total < 0 ? 0 : total > N ? N : total;
    const int x4 = tx0 + 4 * (tid & 15), ybase = ty0 + (tid >> 4);
    const int npx = x4 >= W ? 0 : W - x4 < 4 ? W - x4 : 4, nbytes = 3 * npx;
    int px[SCATTER_RY][12];
    bool loaded = false, touched[SCATTER_RY];
    ACH_UNROLL
    for (int r = 0; r < SCATTER_RY; ++r) touched[r] = false;
    const uint4* boxes = reinterpret_cast<const uint4*>(p.boxes) + b * N;
    const double* discs = p.discs + b * N * 4;
    // the records are sorted by u and a disc reaches at most sqrt(r2max) pixels: only those with u within that of the tile's columns can touch it.  Two binary searches
    // (at most 13 steps each, the same for every thread) bound the walk; the order inside the bounds is untouched
    const double reach = sqrt(p.r2max) + 2.0;
    auto first_not_below = [&](double key, bool strictly_above) {
        int lo = 0, hi = total;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const double u = discs[4L * mid];
            if (strictly_above ? u > key : u >= key) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    const int begin = first_not_below(double(tx0) - reach, false), end = first_not_below(double(tx1) + reach, true);
    for (int base = begin; base < end; base += SCATTER_CHUNK) {
        const int j = base + tid;
        bool hit = false;
        if (j < end) {
            const uint4 bb = boxes[j];
            hit = int(bb.x) <= tx1 && int(bb.z) >= tx0 && int(bb.y) <= ty1 && int(bb.w) >= ty0;
        }
        const unsigned long long votes = wave_ballot64(hit);
        if (lane == 0) wcnt[wave] = __popcll(votes);
        __syncthreads();                                                     // the counts are in; the previous chunk's list has been applied by everyone
        int at = __popcll(votes & ((1ull << lane) - 1ull)), nh = 0;
        ACH_UNROLL
        for (int w = 0; w < 4; ++w) { at += w < wave ? wcnt[w] : 0; nh += wcnt[w]; }
        if (hit) {
            ACH_UNROLL
            for (int k = 0; k < 4; ++k) rec[4 * at + k] = discs[4L * j + k];
        }
        __syncthreads();
        if (nh == 0 || npx == 0) continue;
        if (!loaded) {                                                       // the thread's pixels: three aligned dwords per row, inside the row's pitch
            loaded = true;
            ACH_UNROLL
            for (int r = 0; r < SCATTER_RY; ++r) {
                const int y = ybase + 16 * r;
                uint32_t w[3] = {0u, 0u, 0u};
                if (y < H) {
                    const uint32_t* row = reinterpret_cast<const uint32_t*>(p.arena + f[0] + long(y) * f[3] + 3L * x4);
                    ACH_UNROLL
                    for (int k = 0; k < 3; ++k)
                        if (4 * k < nbytes) w[k] = row[k];
                }
                ACH_UNROLL
                for (int k = 0; k < 12; ++k) px[r][k] = int((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
            }
        }
        for (int s = 0; s < nh; ++s) {
            const double u = rec[4 * s], v = rec[4 * s + 1], r2 = rec[4 * s + 2];
            const int colour = int(rec[4 * s + 3]);
            ACH_UNROLL
            for (int r = 0; r < SCATTER_RY; ++r) {
                const int y = ybase + 16 * r;
                if (y >= H) continue;
                const double dy2 = scatter_dy2(double(y), v);
                if (!(dy2 <= r2)) continue;                                  // dx * dx >= 0 and rounding is monotone: no pixel of the row is covered
                ACH_UNROLL
                for (int i = 0; i < 4; ++i) {
                    if (i >= npx || !scatter_covers(double(x4 + i), u, dy2, r2)) continue;
                    ACH_UNROLL
                    for (int ch = 0; ch < 3; ++ch) {
                        const int q = px[r][3 * i + ch];
                        px[r][3 * i + ch] = int(serve_mix(float(q), p.alpha, float(((colour >> (8 * ch)) & 0xff) - q)));
                    }
                    touched[r] = true;
                }
            }
        }
    }
    ACH_UNROLL
    for (int r = 0; r < SCATTER_RY; ++r) {
        if (!touched[r]) continue;
        uint8_t* row = p.arena + f[0] + long(ybase + 16 * r) * f[3] + 3L * x4;
        if (npx == 4) {
            ACH_UNROLL
            for (int k = 0; k < 3; ++k)
                reinterpret_cast<uint32_t*>(row)[k] = uint32_t(px[r][4 * k]) | uint32_t(px[r][4 * k + 1]) << 8 | uint32_t(px[r][4 * k + 2]) << 16 | uint32_t(px[r][4 * k + 3]) << 24;
        } else {                                                             // the row's last, partial group: its own bytes only
            ACH_UNROLL
            for (int k = 0; k < 9; ++k)
                if (k < nbytes) row[k] = uint8_t(px[r][k]);
        }
    }
}

}  // namespace ach
