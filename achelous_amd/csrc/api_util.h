// api_util.h — what the files of the extern "C" boundary (api.cpp, api_train.cpp, api_frames.cpp) share: the handle, the two guards that keep every
// exception on this side of the boundary, and the argument checks and dispatches more than one entry needs.  Host code only, and no kernel header: a kernel is compiled
// into the one file that launches it.
#pragma once
#include <cstdint>
#include <string>
#include <type_traits>
#include <utility>

#include "engine.h"

struct ach_handle {
    ach::EngineBase* eng = nullptr;
    std::string err;
};

// the text behind ach_last_error(NULL), per thread: ach_create's failures and those of every entry without a handle (defined in api.cpp)
extern thread_local std::string g_stateless_error;

template <class F>
static int caught(std::string& err, F&& f) {
    try { f(); return ACH_OK; }
    catch (const ach::AchError& e) { err = e.msg; return e.code; }
    catch (const std::exception& e) { err = e.what(); return ACH_ERR_INVALID; }
    catch (...) { err = "unknown error"; return ACH_ERR_INVALID; }
}
static void launch_check() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw ach::AchError{ACH_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e)};
}
// an entry with a handle: the failure's text goes to the handle.  Whether the launch error is looked at is the entry's own business (ach_forward does).
template <class F>
static int guarded(ach_handle* h, F&& f) { return (h && h->eng) ? caught(h->err, f) : int(ACH_ERR_INVALID); }
// an entry without one, f(its stream): the text goes to g_stateless_error, and a launch that failed is an error of the call
template <class F>
static int stateless(void* stream, F&& f) { return caught(g_stateless_error, [&] { f(static_cast<hipStream_t>(stream)); launch_check(); }); }

static void need(bool ok, const char* what) { if (!ok) throw ach::AchError{ACH_ERR_INVALID, std::string("bad arguments: ") + what}; }
static hipStream_t as_stream(void* stream) { return static_cast<hipStream_t>(stream); }

// four elements per thread: a count that divides by four and 16-byte aligned pointers (a null pointer is aligned)
template <class... P>
static bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15u) == 0; }
template <class... P>
static bool quad_ok(long n, const P*... p) { return (n & 3) == 0 && aligned16(p...); }

// f(std::integral_constant<int, k>) for the kernel sizes that have an unrolled instantiation; false, and no call, for any other k
template <class F>
static bool odd_k(int k, F&& f) {
    if (k == 3) f(std::integral_constant<int, 3>{});
    else if (k == 5) f(std::integral_constant<int, 5>{});
    else if (k == 7) f(std::integral_constant<int, 7>{});
    else if (k == 9) f(std::integral_constant<int, 9>{});
    else return false;
    return true;
}

// f(elem<T>) for the element kind of a tensor: fp32, bf16, fp16 and, where the entry has one, U8 for kind 3.  Entries check the range before; the last kind takes the rest.
// The kernel headers number their kinds themselves (DATA_*, CONF_*): each file that dispatches holds its header's numbering to this one with a static_assert.
enum ElemKind : int { KIND_F32 = 0, KIND_BF16 = 1, KIND_F16 = 2, KIND_U8 = 3 };
template <class T> struct elem { using type = T; };
template <class U8 = void, class F>
static void by_kind(int kind, F&& f) {
    if (kind == KIND_F32) f(elem<float>{});
    else if (kind == KIND_BF16) f(elem<ach::bf16_t>{});
    else if constexpr (std::is_void_v<U8>) f(elem<ach::f16_t>{});
    else if (kind == KIND_F16) f(elem<ach::f16_t>{});
    else f(elem<U8>{});
}

// host-table checks.  Sizes: both at least 1 and at most `top`.
static bool dims_ok(int64_t a, int64_t b, int64_t top) { return a >= 1 && b >= 1 && a <= top && b <= top; }
// a resized frame's placement on the canvas: a size below 2^30 at an offset of either sign inside +-2^30
static bool placement_ok(int64_t nw, int64_t nh, int64_t dx, int64_t dy) {
    return dims_ok(nw, nh, (1L << 30) - 1) && dx > -(1L << 30) && dx < (1L << 30) && dy > -(1L << 30) && dy < (1L << 30);
}
// `rows` rows (checked by the caller) of `row` units at `pitch` from `off` inside an arena of `arena` units: the pitch holds a row and stays below `cap`, offset and pitch are
// multiples of `align`, and (rows - 1) * pitch + last fits behind the offset — `last` is the entry's own: the row itself where the last row may end short, the pitch where it may not
static bool frame_fits(int64_t off, int64_t rows, int64_t row, int64_t pitch, int64_t last, int64_t arena, int64_t align = 1, int64_t cap = 1L << 32) {
    return pitch >= row && pitch < cap && pitch % align == 0 && off >= 0 && off % align == 0 && off <= arena && (rows - 1) * pitch + last <= arena - off;
}
