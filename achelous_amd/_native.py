"""The one place where the training, data and serving modules meet ctypes for the STATELESS entries of the C ABI (include/achelous.h: `ach_train_*`, `ach_eval_*`,
`ach_data_*`, the resample pass) and for the engine handle that serves the stateless pre / post-processing kernels.  Nothing here knows a model: library choice
with its one test hook, the return-code check, tensor -> pointer / stream, and the GEMM call forms with their strides read from the tensors.
(`engine.py` binds the library and owns `NativeEngine`; this module is what sits between it and train_functional / losses / metrics / data / prepost.)
"""
import ctypes

import torch

from . import engine as _eng

NULL = ctypes.c_void_p()
DTYPE_CODE = {torch.float32: _eng.DTYPE_F32, torch.bfloat16: _eng.DTYPE_BF16, torch.float16: _eng.DTYPE_F16}


def lib(t):
    """The library that serves tensors like `t`: the HIP library for GPU tensors.  `lib.test_library` (tests only) replaces it by the emulation build and admits CPU
    tensors.  ONE function object under every name it is known by (`train_ops._lib`, `prepost._pass_lib`), so the hook set through any of them holds for all modules."""
    test = getattr(lib, 'test_library', None)
    if test is None and not t.is_cuda:
        raise RuntimeError("achelous_amd needs GPU tensors (HIP kernels; there is no CPU path)")
    return test or _eng.hip_library()


def check(lib, rc, errors=None, what='native call'):
    """rc != 0 -> `errors[rc]` (default and fallback: RuntimeError) with the text of ach_last_error(NULL)"""
    if rc != 0:
        raise (errors or {}).get(rc, RuntimeError)((lib.lib.ach_last_error(None) or f'{what} failed'.encode()).decode())


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else NULL


def stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0)


def f32c(t, what):
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: the native kernels are float32 (got {t.dtype}); cast, or run under torch.autocast where the function supports it")
    return t.contiguous()


def empty(like, *shape):
    return torch.empty(*shape, dtype=torch.float32, device=like.device)


# ------------------------------------------------------------------------------------------------------------------ the stand-in engine handle
_handles = {}


def stateless_handle(num_det, resolution, dtype, lib=None):
    """The engine handle behind the kernels that need none of a model's weights (decode, NMS, box correction, pre-processing, class maps): the smallest configuration,
    cached per (current device — or `lib`, a test library —, num_det, resolution, dtype)."""
    if dtype not in DTYPE_CODE:
        # the kernels exist for fp32, bf16 and fp16 tensors only; any other element size would be read / written with the wrong stride
        raise TypeError(f"achelous_amd kernels take float32, bfloat16 or float16 tensors, got {dtype}")
    key = (torch.cuda.current_device() if lib is None else lib, num_det, resolution, DTYPE_CODE[dtype])
    if key not in _handles:
        _handles[key] = _eng.NativeEngine(lib or _eng.hip_library(), num_det=num_det, num_seg=1, phi='S0', backbone='en', resolution=resolution, pc_channels=3,
                                          pc_classes=1, num_points=16, nano_head=True, spp=True, dtype=key[3])
    return _handles[key]


# ------------------------------------------------------------------------------------------------------------------ GEMM forms (ach_train_gemm_p)
def prec(lib):
    """The operand type a training forward runs its GEMMs with (ach_train_set_gemm_precision, set by the module's forward): recorded on the autograd ctx so that the
    node's backward launches use the same one whatever another module or thread has set meanwhile (ach_train_gemm_p)."""
    return int(lib.lib.ach_train_get_gemm_precision())


def _gemm(lib, s, A, B, C, bias, M, N, K, lda, ldb, ldc, sA, sB, sC, tA, tB, batch, reduce, prec):
    """C[b] = op(A[b]) op(B[b]) (+ bias per row) for b < batch; reduce: ONE C = the sum over b.  Row-major leading dimensions, element strides between batches."""
    check(lib, lib.lib.ach_train_gemm_p(ptr(A), ptr(B), ptr(C), ptr(bias), M, N, K, lda, ldb, ldc, sA, sB, sC, tA, tB, batch, reduce, 0, int(prec), s), what='train gemm')


def _batch_cols(act):
    """(B, O) of an activation [B, channels, ...]: O = everything behind the channel axis"""
    B = act.shape[0]
    return B, act.numel() // (B * act.shape[1])


def gemm_w_cols(lib, s, w2, cols, out, bias, prec):
    """out[b] = w2 cols[b] (+ bias): w2 [Co, K], cols [B, K, O], out [B, Co, O] (trailing axes may be split, as in [B, Co, Ho, Wo])"""
    (Co, K), (B, O) = w2.shape, _batch_cols(cols)
    _gemm(lib, s, w2, cols, out, bias, Co, O, K, K, O, O, 0, K * O, Co * O, 0, 0, B, 0, prec)


def gemm_wt_dz(lib, s, w2, dz, dcols, prec):
    """dcols[b] = w2^T dz[b]: dz [B, Co, O], dcols [B, K, O]"""
    (Co, K), (B, O) = w2.shape, _batch_cols(dz)
    _gemm(lib, s, w2, dz, dcols, None, K, O, Co, K, O, O, 0, Co * O, K * O, 1, 0, B, 0, prec)


def gemm_dw(lib, s, dz, cols, dw, prec):
    """dw = sum_b dz[b] cols[b]^T: dz [B, Co, O], cols [B, K, O]; dw holds [Co, K] in memory, in any parameter shape"""
    Co, K, (B, O) = dz.shape[1], cols.shape[1], _batch_cols(dz)
    _gemm(lib, s, dz, cols, dw, None, Co, K, O, O, O, K, Co * O, K * O, 0, 0, 1, B, 1, prec)


def gemm_batched(lib, s, a, b, c, ta, tb, prec):
    """c[t] = op(a[t]) op(b[t]) for contiguous 3-D tensors; ta / tb: the operand is stored transposed"""
    T, M, N = c.shape
    K = a.shape[1] if ta else a.shape[2]
    _gemm(lib, s, a, b, c, None, M, N, K, a.shape[2], b.shape[2], N, a.shape[1] * a.shape[2], b.shape[1] * b.shape[2], M * N, int(ta), int(tb), T, 0, prec)
