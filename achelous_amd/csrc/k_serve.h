// k_serve.h — what the reference's detect_image does AFTER the forward (achelous.py:283-345) for a whole ragged batch in ONE launch: both segmentation heads'
// class maps at every frame's own size (softmax -> crop the letterbox window -> cv2 INTER_LINEAR -> argmax, the arithmetic of seg_resize_argmax_kernel,
// k_prepost.h) and the overlay image (palette lookup, two PIL Image.blend, ImageEnhance.Brightness), written next to the camera bytes they were computed from.
//
// The original images sit in the packed uint8 arena they were uploaded in (HWC, any pitch >= 3 W: achelous_amd/data.py `Arena`); every output is a packed arena
// of its own with 16-byte aligned frame starts and row pitches that are multiples of 16, so a thread that owns four neighbouring pixels stores whole dwords.
// A host-built table says where; no arrays of pointers.
//   frame table int64 [B][16]: 0 byte offset of the image in the arena, 1 H, 2 W, 3 image pitch, 4 y0, 5 x0, 6 nh, 7 nw (the window of the R x R network map
//                that is stretched over the frame: the letterbox's, or (0, 0, R, R)), 8 byte offset of the semantic map in its arena, 9 of the water-line map
//                in its arena, 10 pitch of both maps, 11 byte offset of the overlay in its arena, 12 overlay pitch, 13-15 unused.
//   constants   2304 bytes on the device: semantic palette [256][3], water-line palette [256][3], semantic remap [256], water-line remap [256], brightness
//                table [256].  overlay = lut[blend(blend(image, pal_se[remap_se[class]], a1), pal_line[remap_line[line class]], a2)].
// The C entry (api_frames.cpp ach_seg_overlay_frames) checks every extent, pitch and alignment on the host before the launch: the kernel trusts the table.
//
// Arithmetic.  Class maps: coordinate float((double(d) + 0.5) * s - 0.5), the clamps, horizontal blend then vertical blend in fp32, first maximum — operation for
// operation what seg_resize_argmax_kernel computes (serve_hblend / serve_vblend below say exactly what that is on the device).  That order rules out a vertical-first separable pass, but the HORIZONTAL blends are shared: at a
// 6x up-scale a source row serves about six output rows as `top` and again as `bot`.  A workgroup owns SERVE_TW output columns x the output rows whose upper
// source row falls in a band of `rows - 1` source rows; it blends the band's `rows` source rows horizontally for every class of both heads once into LDS, then a
// thread owns 4 neighbouring pixels of a row: two LDS reads of 16 bytes per class, the vertical blend and the running arg-max in registers.  Down-scaling frames
// take the same path (fewer output rows per band).  Overlay: PIL's Image.blend is out = (UINT8)(in1 + alpha * (in2 - in1)) in float32 WITHOUT contraction;
// Brightness.enhance(f) is a blend of black and the image: a 256-entry table built on the host.
#pragma once
#include "ach_platform.h"

namespace ach {

constexpr int SERVE_TABLE_COLS = 16;
constexpr int SERVE_TW = 128;                 // output columns per workgroup: 32 threads x 4 pixels
constexpr int SERVE_LDS_FLOATS = 8192;        // 32 KB of horizontally blended rows per workgroup: [row][class][SERVE_TW]
constexpr int SERVE_MAX_ROWS = 8;             // staged source rows per workgroup (at least 2: a band of one row and the row below it)
constexpr int SERVE_CONST_BYTES = 2304;
constexpr int SERVE_PAL_LINE = 768, SERVE_REMAP_SE = 1536, SERVE_REMAP_LINE = 1792, SERVE_LUT = 2048;

// one axis of INTER_LINEAR exactly as seg_resize_argmax_kernel computes it: the two source indices and the weight of the second
struct ServeAxis { int i0, i1; float f; };
__host__ __device__ __forceinline__ ServeAxis serve_axis(int d, double s, int n) {
    float f = float((double(d) + 0.5) * s - 0.5);
    int i = int(floorf(f));
    f -= float(i);
    if (i < 0) { i = 0; f = 0.f; }
    if (i >= n - 1) { i = n - 1; f = 0.f; }
    ServeAxis a;
    a.i0 = i; a.i1 = i + 1 < n ? i + 1 : i; a.f = f;
    return a;
}
__host__ __device__ __forceinline__ int serve_rows(int classes) {
    const int r = SERVE_LDS_FLOATS / (classes * SERVE_TW);
    return r < SERVE_MAX_ROWS ? r : SERVE_MAX_ROWS;
}

// The arithmetic, stated so that the compiler has no choice.  HIP's __fmul_rn / __fadd_rn are plain operators on this target and do NOT stop contraction: as hipcc
// compiles seg_resize_argmax_kernel, each horizontal blend is ONE fused multiply-add on the rounded second product, fma(q[ix], 1 - fx, rn(q[ix1] * fx)), and the vertical
// blend is two rounded products and an add.  That — not the uncontracted sequence its source spells — is what the shipped path computes on the device, so it is what
// this kernel computes there (bit for bit: profiles/scripts/serve_timing.py compares 133 M pixels per head before it times anything); under the CPU emulation both
// kernels run the uncontracted sequence, which is the oracle's.  PIL's Image.blend is never contracted.
#if defined(ACH_HOSTEMU)
inline float serve_hblend(float q0, float q1, float w0, float w1) { return __fadd_rn(__fmul_rn(q0, w0), __fmul_rn(q1, w1)); }
inline float serve_vblend(float t, float u, float w0, float w1) { return __fadd_rn(__fmul_rn(t, w0), __fmul_rn(u, w1)); }
inline float serve_mix(float a, float t, float d) { return __fadd_rn(a, __fmul_rn(t, d)); }
#else
__device__ __forceinline__ float serve_hblend(float q0, float q1, float w0, float w1) {
#pragma clang fp contract(off)
    const float r = q1 * w1;
    return __builtin_fmaf(q0, w0, r);
}
__device__ __forceinline__ float serve_vblend(float t, float u, float w0, float w1) {
#pragma clang fp contract(off)
    const float x = t * w0, y = u * w1;
    return x + y;
}
__device__ __forceinline__ float serve_mix(float a, float t, float d) {      // a + t * d, the product rounded
#pragma clang fp contract(off)
    const float x = t * d;
    return a + x;
}
#endif

struct ServeParams {
    const float* P0; const float* P1;          // probabilities [B, C0, R, R] and [B, C1, R, R]; C0 / C1 = 0: that head is not needed
    const uint8_t* arena; const long long* table; const uint8_t* consts;
    uint8_t* sem; uint8_t* line; uint8_t* ovl;  // null: not wanted
    int R, C0, C1, rows;
    float a1, a2;
    int use_lut;
};

static __global__ __launch_bounds__(256) void seg_overlay_frames_kernel(const ServeParams p) {
    __shared__ float4 hb4[SERVE_LDS_FLOATS / 4];
    __shared__ uint32_t cst[SERVE_CONST_BYTES / 4];
    float* hb = reinterpret_cast<float*>(hb4);
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const long long* f = p.table + b * SERVE_TABLE_COLS;
    const int H = int(f[1]), W = int(f[2]), y0 = int(f[4]), x0 = int(f[5]), nh = int(f[6]), nw = int(f[7]);
    const int ntx = (W + SERVE_TW - 1) / SERVE_TW, band = p.rows - 1, nb = (nh + band - 1) / band;
    if (long(blockIdx.x) >= long(ntx) * nb) return;
    const int bnd = int(blockIdx.x) / ntx, ox0 = (int(blockIdx.x) - bnd * ntx) * SERVE_TW;
    const int r0 = bnd * band;                                           // this workgroup: output rows whose upper source row iy is in [r0, rend)
    const int rend = r0 + band < nh ? r0 + band : nh;
    const int nrows = (r0 + band < nh - 1 ? r0 + band : nh - 1) - r0 + 1;   // staged source rows r0 .. min(r0 + band, nh - 1)
    const double sy = double(nh) / double(H), sx = double(nw) / double(W);
    const int Ct = p.C0 + p.C1;
    const long HW = long(p.R) * p.R;
    if (p.ovl)
        for (int i = tid; i < SERVE_CONST_BYTES / 4; i += 256) cst[i] = reinterpret_cast<const uint32_t*>(p.consts)[i];
    {   // horizontal blends of the staged rows: a thread keeps ONE output column, so its coordinate and weights are computed once
        const int col = tid & (SERVE_TW - 1), x = ox0 + col;
        if (x < W) {
            const ServeAxis ax = serve_axis(x, sx, nw);
            const float ax0 = 1.f - ax.f;
            for (int k = tid / SERVE_TW; k < nrows * Ct; k += 256 / SERVE_TW) {
                const int row = k / Ct, c = k - row * Ct;
                const float* q = (c < p.C0 ? p.P0 + (b * p.C0 + c) * HW : p.P1 + (b * p.C1 + (c - p.C0)) * HW) + long(y0 + r0 + row) * p.R + x0;
                hb[k * SERVE_TW + col] = serve_hblend(q[ax.i0], q[ax.i1], ax0, ax.f);
            }
        }
    }
    __syncthreads();
    // the output rows of the band: iy is non-decreasing in dy, so they are one range, found with the kernel's own coordinate function
    auto first_row = [&](int target) {
        int lo = 0, hi = H;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (serve_axis(mid, sy, nh).i0 >= target) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    const int dy_lo = first_row(r0), dy_hi = rend >= nh ? H : first_row(rend);
    const int cg = tid & 31, x4 = ox0 + 4 * cg;
    if (x4 >= W) return;
    const int npx = W - x4 < 4 ? W - x4 : 4;
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(cst);
    for (int dy = dy_lo + (tid >> 5); dy < dy_hi; dy += 8) {
        const ServeAxis ay = serve_axis(dy, sy, nh);
        const float ay0 = 1.f - ay.f;
        const float* top = hb + (ay.i0 - r0) * Ct * SERVE_TW + 4 * cg;
        const float* bot = hb + (ay.i1 - r0) * Ct * SERVE_TW + 4 * cg;
        int cls[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        ACH_UNROLL
        for (int head = 0; head < 2; ++head) {
            const int c0 = head ? p.C0 : 0, c1 = head ? Ct : p.C0;
            float best[4] = {-1.f, -1.f, -1.f, -1.f};
            for (int c = c0; c < c1; ++c) {
                const float4 t4 = *reinterpret_cast<const float4*>(top + c * SERVE_TW), u4 = *reinterpret_cast<const float4*>(bot + c * SERVE_TW);
                const float t[4] = {t4.x, t4.y, t4.z, t4.w}, u[4] = {u4.x, u4.y, u4.z, u4.w};
                ACH_UNROLL
                for (int i = 0; i < 4; ++i) {
                    const float v = serve_vblend(t[i], u[i], ay0, ay.f);
                    if (v > best[i]) { best[i] = v; cls[head][i] = c - c0; }
                }
            }
            ACH_UNROLL
            for (int i = 0; i < 4; ++i)
                if (i >= npx) cls[head][i] = 0;                          // past the row's end: the padding gets zeros
        }
        if (p.sem) *reinterpret_cast<uint32_t*>(p.sem + f[8] + long(dy) * f[10] + x4) = uint32_t(cls[0][0]) | uint32_t(cls[0][1]) << 8 | uint32_t(cls[0][2]) << 16 | uint32_t(cls[0][3]) << 24;
        if (p.line) *reinterpret_cast<uint32_t*>(p.line + f[9] + long(dy) * f[10] + x4) = uint32_t(cls[1][0]) | uint32_t(cls[1][1]) << 8 | uint32_t(cls[1][2]) << 16 | uint32_t(cls[1][3]) << 24;
        if (p.ovl) {
            // the 3 * npx image bytes start at any byte: aligned dwords (the arena is 16-byte aligned and padded, a dword that holds a needed byte is inside it)
            const long a = f[0] + long(dy) * f[3] + 3L * x4, A = a & ~3L;
            const int nbytes = 3 * npx, sh = int(a & 3) * 8;
            uint32_t w[4], in[3], out[3] = {0u, 0u, 0u};
            ACH_UNROLL
            for (int k = 0; k < 4; ++k) w[k] = A + 4 * k < a + nbytes ? *reinterpret_cast<const uint32_t*>(p.arena + A + 4 * k) : 0u;
            ACH_UNROLL
            for (int k = 0; k < 3; ++k) in[k] = sh ? (w[k] >> sh) | (w[k + 1] << (32 - sh)) : w[k];
            ACH_UNROLL
            for (int i = 0; i < 4; ++i) {
                if (i >= npx) break;
                const int ps = 3 * cb[SERVE_REMAP_SE + cls[0][i]], pl = SERVE_PAL_LINE + 3 * cb[SERVE_REMAP_LINE + cls[1][i]];
                ACH_UNROLL
                for (int ch = 0; ch < 3; ++ch) {
                    const int j = 3 * i + ch;
                    const int v = int((in[j >> 2] >> (8 * (j & 3))) & 0xffu);
                    const int o1 = int(serve_mix(float(v), p.a1, float(int(cb[ps + ch]) - v)));
                    int o2 = int(serve_mix(float(o1), p.a2, float(int(cb[pl + ch]) - o1)));
                    if (p.use_lut) o2 = cb[SERVE_LUT + o2];
                    out[j >> 2] |= uint32_t(o2) << (8 * (j & 3));
                }
            }
            uint32_t* o = reinterpret_cast<uint32_t*>(p.ovl + f[11] + long(dy) * f[12] + 3L * x4);
            ACH_UNROLL
            for (int k = 0; k < 3; ++k)
                if (4 * k < nbytes) o[k] = out[k];
        }
    }
}

}  // namespace ach
