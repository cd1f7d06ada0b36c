// k_data.h — training batches assembled on the device from ragged frames (achelous_amd/data.py): what the reference's dataset does per frame on the host
// (utils/dataloader.py:87-148, 153-233: a PIL BICUBIC letterbox of the camera image, two PIL NEAREST letterboxes of the label maps, the label clamps, the
// float64 normalisation), for a whole batch in three launches whatever its size.
//
// All images of a batch sit in ONE packed uint8 arena (HWC rows, any pitch), all label maps in another; a host-built table says where.  No arrays of pointers.
//   image table  int64 [B][16]: 0 byte offset, 1 H, 2 W, 3 pitch (bytes per row), 4 nw, 5 nh, 6 dx, 7 dy (the resized size and where it is pasted: any sign, any
//                size), 8 / 9 / 10 horizontal bounds [nw][2], coefficients [nw][ks] and ks, 11 / 12 / 13 the same for the vertical axis ([nh]), 14 byte offset of
//                the frame's part of the intermediate arena, 15 unused.  Table offsets count int32 elements of `tabs`.
//   label table  int64 [B][16]: 0 nw, 1 nh, 2 dx, 3 dy, then per map (semantic at 4, water line at 10): byte offset (< 0: no such map -> zeros), H, W, pitch,
//                column index table [nw], row index table [nh] (source index per resized sample, -1: none).
// Bounds / coefficients are Pillow's precompute_coeffs + normalize_coeffs_8bpc over the whole axis (22-bit fixed point), as for resample_pass_kernel
// (k_prepost.h); the index tables are Pillow's running double sum, which no closed form reproduces.  The C entries (api_frames.cpp) check every extent
// and every table entry on the host before anything is launched: the kernels themselves trust the tables.
#pragma once
#include "ach_platform.h"

namespace ach {

constexpr int DATA_TABLE_COLS = 16;
constexpr int DATA_LDS_BYTES = 48 * 1024;          // staged source rows of one workgroup of the horizontal pass
constexpr int DATA_ROWS = 8;                       // source rows per workgroup (fewer when a row does not fit eight times)
enum DataOut : int { DATA_F32 = 0, DATA_BF16 = 1, DATA_F16 = 2, DATA_U8_HWC = 3 };

// the visible part of a frame's window on the R x R canvas, and the source rows / columns it needs
struct DataWindow { int vx0, vx1, vy0, vy1; };
__host__ __device__ __forceinline__ DataWindow data_window(long nw, long nh, long dx, long dy, int R) {
    DataWindow w;
    w.vx0 = int(dx > 0 ? (dx < R ? dx : R) : 0);
    w.vy0 = int(dy > 0 ? (dy < R ? dy : R) : 0);
    const long x1 = dx + nw, y1 = dy + nh;
    w.vx1 = int(x1 < 0 ? 0 : (x1 > R ? R : x1));
    w.vy1 = int(y1 < 0 ? 0 : (y1 > R ? R : y1));
    return w;
}
__host__ __device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// a byte times a 22-bit fixed-point coefficient (|k| < 2^23: a normalised BICUBIC tap is at most 1.0) as a full-rate 24-bit multiply; the product is exact
#if defined(ACH_HOSTEMU)
inline int tap_mul(int v, int k) { return v * k; }
#else
__device__ __forceinline__ int tap_mul(int v, int k) { return __mul24(v, k); }
#endif

// ---- horizontal pass: workgroup = (block of source rows, frame).  The rows' needed bytes are staged into LDS with aligned 16-byte loads (a row may start at
// any byte: the load starts at the 16-byte line below it, `shift` bytes early); a thread owns one (column, channel) of the visible window for all staged rows,
// so a coefficient is loaded once per DATA_ROWS products.  Output: the 8-bit intermediate as PLANES [row][channel][R4] indexed by CANVAS column, so the vertical
// pass reads four neighbouring pixels of one channel as one aligned dword.  Only the rows the visible output rows need are computed.
struct DataHParams { const uint8_t* arena; const long long* table; const int* tabs; uint8_t* mid; int R, R4, rows_pb, lstride; };
static __global__ __launch_bounds__(256) void data_hpass_kernel(const DataHParams p) {
    __shared__ uint4 stage[DATA_LDS_BYTES / 16];
    const long long* f = p.table + long(blockIdx.y) * DATA_TABLE_COLS;
    const long off = f[0], pitch = f[3], dx = f[6], dy = f[7];
    const DataWindow w = data_window(f[4], f[5], dx, dy, p.R);
    if (w.vx0 >= w.vx1 || w.vy0 >= w.vy1) return;
    const int* hb = p.tabs + f[8];
    const int* hk = p.tabs + f[9];
    const int hks = int(f[10]);
    const int* vb = p.tabs + f[11];
    const int r0 = vb[2 * (w.vy0 - dy)], r1 = vb[2 * (w.vy1 - 1 - dy)] + vb[2 * (w.vy1 - 1 - dy) + 1];
    const int row0 = r0 + int(blockIdx.x) * p.rows_pb;
    if (row0 >= r1) return;
    const int nrows = r1 - row0 < p.rows_pb ? r1 - row0 : p.rows_pb;
    const int sx0 = hb[2 * (w.vx0 - dx)], sx1 = hb[2 * (w.vx1 - 1 - dx)] + hb[2 * (w.vx1 - 1 - dx) + 1];
    const int span = (sx1 - sx0) * 3;
    const long a00 = off + long(row0) * pitch + long(sx0) * 3;          // first needed byte of the block's first row
    const int cpr = p.lstride >> 4;
    for (int i = threadIdx.x; i < nrows * cpr; i += 256) {
        const int r = i / cpr, ch = i - r * cpr;
        const long a0 = a00 + long(r) * pitch, A0 = a0 & ~15L;
        if (A0 + long(ch) * 16 < a0 + span) stage[i] = *reinterpret_cast<const uint4*>(p.arena + A0 + long(ch) * 16);
    }
    __syncthreads();
    const uint8_t* lds = reinterpret_cast<const uint8_t*>(stage);
    const int visw = w.vx1 - w.vx0;
    uint8_t* mid = p.mid + f[14] + long(row0 - r0) * 3 * p.R4;
    int rb[DATA_ROWS];                                                   // LDS byte address of each staged row's first needed byte
    ACH_UNROLL
    for (int r = 0; r < DATA_ROWS; ++r) rb[r] = r < nrows ? r * p.lstride + int((a00 + long(r) * pitch) & 15) : 0;
    for (int it = threadIdx.x; it < visw * 3; it += 256) {
        const int c = it / visw, xi = it - c * visw;
        const long ox = w.vx0 + xi - dx;
        const int first = hb[2 * ox], count = hb[2 * ox + 1];
        const int* k = hk + ox * hks;
        const int base = (first - sx0) * 3 + c;
        int acc[DATA_ROWS];
        ACH_UNROLL
        for (int r = 0; r < DATA_ROWS; ++r) acc[r] = 1 << 21;
        if (nrows == DATA_ROWS) {                                         // a full block: eight independent LDS reads per tap, no branch between them
            for (int t = 0; t < count; ++t) {
                const int kt = k[t];
                ACH_UNROLL
                for (int r = 0; r < DATA_ROWS; ++r) acc[r] += tap_mul(int(lds[rb[r] + base + 3 * t]), kt);
            }
        } else {
            for (int t = 0; t < count; ++t) {
                const int kt = k[t];
                ACH_UNROLL
                for (int r = 0; r < DATA_ROWS; ++r)
                    if (r < nrows) acc[r] += tap_mul(int(lds[rb[r] + base + 3 * t]), kt);
            }
        }
        ACH_UNROLL
        for (int r = 0; r < DATA_ROWS; ++r)
            if (r < nrows) mid[(long(r) * 3 + c) * p.R4 + w.vx0 + xi] = uint8_t(clip8(acc[r] >> 22));
    }
}

// ---- vertical pass, fused with the paste, the grey canvas, the normalisation and the layout change: a thread owns four neighbouring canvas pixels; per
// channel and tap ONE aligned dword of the intermediate.  The 8-bit result indexes a 768-entry table [channel][value] of ((v / 255) - mean) / std computed in
// double on the host and rounded once to fp32 (what the reference's float64 arithmetic followed by FloatTensor gives), then one RNE rounding to a 16-bit type.
// Pixels outside the window take the table's value for 128: nothing is filled beforehand.  T = uint8_t: the bytes themselves, HWC.
struct DataVParams { const long long* table; const int* tabs; const uint8_t* mid; const float* lut; void* out; int R, R4; };
template <class T>
__global__ __launch_bounds__(256) void data_vpass_kernel(const DataVParams p) {
    __shared__ float lut[768];
    if constexpr (!std::is_same<T, uint8_t>::value) {
        for (int i = threadIdx.x; i < 768; i += 256) lut[i] = p.lut[i];
        __syncthreads();
    }
    const int q = p.R4 >> 2;
    const long idx = long(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= long(p.R) * q) return;
    const int y = int(idx / q), x = int(idx - long(y) * q) * 4;
    const long b = blockIdx.y;
    const long long* f = p.table + b * DATA_TABLE_COLS;
    const long dx = f[6], dy = f[7];
    const DataWindow w = data_window(f[4], f[5], dx, dy, p.R);
    int v[3][4];
    ACH_UNROLL
    for (int c = 0; c < 3; ++c) { ACH_UNROLL for (int i = 0; i < 4; ++i) v[c][i] = 128; }
    if (w.vx0 < w.vx1 && y >= w.vy0 && y < w.vy1 && x + 3 >= w.vx0 && x < w.vx1) {
        const int* vb = p.tabs + f[11];
        const int r0 = vb[2 * (w.vy0 - dy)];
        const long oy = y - dy;
        const int first = vb[2 * oy], count = vb[2 * oy + 1];
        const int* k = p.tabs + f[12] + oy * f[13];
        const uint8_t* m = p.mid + f[14] + long(first - r0) * 3 * p.R4 + x;
        ACH_UNROLL
        for (int c = 0; c < 3; ++c) {
            int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
            for (int t = 0; t < count; ++t) {
                const uint32_t px = *reinterpret_cast<const uint32_t*>(m + (long(t) * 3 + c) * p.R4);
                const int kt = k[t];
                ACH_UNROLL
                for (int i = 0; i < 4; ++i) acc[i] += tap_mul(int((px >> (8 * i)) & 0xffu), kt);
            }
            ACH_UNROLL
            for (int i = 0; i < 4; ++i)
                if (x + i >= w.vx0 && x + i < w.vx1) v[c][i] = clip8(acc[i] >> 22);
        }
    }
    const long RR = long(p.R) * p.R;
    ACH_UNROLL
    for (int i = 0; i < 4; ++i) {
        if (x + i >= p.R) break;
        ACH_UNROLL
        for (int c = 0; c < 3; ++c) {
            if constexpr (std::is_same<T, uint8_t>::value) static_cast<uint8_t*>(p.out)[(b * RR + long(y) * p.R + x + i) * 3 + c] = uint8_t(v[c][i]);
            else Store<T>::st(static_cast<T*>(p.out) + (b * 3 + c) * RR + long(y) * p.R + x + i, lut[c * 256 + v[c][i]]);
        }
    }
}

// ---- both label maps of every frame in one launch: blockIdx.y = map (0 semantic, clamp n_seg; 1 water line, clamp 2), blockIdx.z = frame.  NEAREST through
// the two index tables, pasted on zeros; a frame without the map gives zeros.  Whole [B, R, R] planes are written, as uint8 or int64.
struct DataLabelParams { const uint8_t* arena; const long long* table; const int* tabs; void* out[2]; int R, n_seg, wide; };
static __global__ __launch_bounds__(256) void data_labels_kernel(const DataLabelParams p) {
    const long idx = long(blockIdx.x) * 256 + threadIdx.x;
    const long RR = long(p.R) * p.R;
    if (idx >= RR) return;
    const int y = int(idx / p.R), x = int(idx - long(y) * p.R);
    const int m = blockIdx.y;
    const long b = blockIdx.z;
    const long long* f = p.table + b * DATA_TABLE_COLS;
    const long long* g = f + 4 + 6 * m;
    const long dx = f[2], dy = f[3];
    const DataWindow w = data_window(f[0], f[1], dx, dy, p.R);
    int v = 0;
    if (g[0] >= 0 && x >= w.vx0 && x < w.vx1 && y >= w.vy0 && y < w.vy1) {
        const int sx = p.tabs[g[4] + (x - dx)], sy = p.tabs[g[5] + (y - dy)];
        if (sx >= 0 && sy >= 0) {
            v = p.arena[g[0] + long(sy) * g[3] + sx];
            const int n = m == 0 ? p.n_seg : 2;
            v = v < n ? v : n;
        }
    }
    if (p.wide) static_cast<long long*>(p.out[m])[b * RR + idx] = v;
    else static_cast<uint8_t*>(p.out[m])[b * RR + idx] = uint8_t(v);
}

}  // namespace ach
