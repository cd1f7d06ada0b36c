"""The native calls the Python glue makes, case by case (tests/test_native_calls.py; fixture tests/golden/native_calls.json, written by
tests/golden/gen_native_calls_golden.py at the commit the fixture names).

`Recorder` stands in for the emulation library behind `train_ops._lib.test_library`: every `ach_train_*`, `ach_eval_*` and `ach_data_*` entry called through it is
logged as [name, argument, ...] before it runs — integers as they are, floats as `float.hex`, pointers as 0 (null) or 1 (addresses depend on the allocator, not on the
glue).  `ach_train_get_gemm_precision` is a query, asked a different number of times by equivalent code, and is left out.  The cases are the smallest shapes that reach
every branch of the Python layer above the C ABI: which kernel the C side dispatches for a shape is not what this pins.  Only names that exist on both sides of a
refactor are used: the public functions, the autograd Functions train_graph.py imports, and the `train_ops._lib.test_library` hook."""
import ctypes
import hashlib
import json

import torch

from achelous_amd import train_ops, train_functional as TF

PREFIXES = ('ach_train_', 'ach_eval_', 'ach_data_')
NOT_RECORDED = ('ach_train_get_gemm_precision',)
_FLOATS = (ctypes.c_float, ctypes.c_double)
KEEP_DEFAULT = 1 << 30          # train_functional.KEEP_COLUMN_BYTES without the environment variable


def _encode(ctype, v):
    if ctype is ctypes.c_void_p:
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        return 1 if v else 0
    if ctype in _FLOATS:
        return float(v).hex()
    return int(v)


class _Entries:
    def __init__(self, real, log):
        self.__dict__.update(_real=real, _log=log)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith(PREFIXES) or name in NOT_RECORDED:
            return fn

        def recorded(*args):
            assert len(args) == len(fn.argtypes), name
            self._log.append([name] + [_encode(t, v) for t, v in zip(fn.argtypes, args)])
            return fn(*args)
        return recorded


class Recorder:
    """`NativeLibrary`-shaped: `.lib` logs into `.log` and forwards to the wrapped library"""

    def __init__(self, library):
        self.log = []
        self.path = library.path
        self.lib = _Entries(library.lib, self.log)


def canonical(trace):
    return json.dumps(trace, separators=(',', ':'))


def digest(trace):
    return hashlib.sha256(canonical(trace).encode()).hexdigest()


def counts(trace):
    out = {}
    for call in trace:
        out[call[0]] = out.get(call[0], 0) + 1
    return dict(sorted(out.items()))


# ------------------------------------------------------------------------------------------------------------------ the cases
def _r(*shape, seed=0, grad=False):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).requires_grad_(grad)


def _back(y):
    y.square().sum().backward()


def _shared_mlp():
    m = train_ops.SharedMLP1d(3, 5).train()
    _back(m(_r(2, 3, 7, grad=True)))
    with torch.no_grad():
        m.eval()(_r(2, 3, 7, seed=1))               # the running-statistics branch


def _linear(bias):
    _back(train_ops._LinearFn.apply(_r(2, 3, 7, grad=True), _r(5, 3, seed=1, grad=True), _r(5, seed=2, grad=True) if bias else None))


def _with_keep(limit, fn):
    old, TF.KEEP_COLUMN_BYTES = TF.KEEP_COLUMN_BYTES, limit
    try:
        fn()
    finally:
        TF.KEEP_COLUMN_BYTES = old


def _conv3x3(keep, x_grad):
    _with_keep(keep, lambda: _back(TF.conv2d(_r(2, 3, 6, 5, grad=x_grad), _r(4, 3, 3, 3, seed=1, grad=True), _r(4, seed=2, grad=True), stride=2, padding=1)))


def _conv_direct():
    _back(TF.conv2d(_r(2, 3, 6, 5, grad=True), _r(4, 3, 1, 1, seed=1, grad=True), _r(4, seed=2, grad=True)))


def _conv1x1():
    _back(TF.conv1x1(_r(2, 3, 6, 5, grad=True), _r(4, 3, 1, 1, seed=1, grad=True), _r(4, seed=2, grad=True)))


def _deform(stride, keep, x_grad):
    Ho, Wo = (6 + 2 - 3) // stride + 1, (5 + 2 - 3) // stride + 1
    _with_keep(keep, lambda: _back(TF.deform_conv3x3(_r(2, 3, 6, 5, grad=x_grad), _r(2, 18, Ho, Wo, seed=1, grad=True), torch.sigmoid(_r(2, 9, Ho, Wo, seed=2)).requires_grad_(True),
                                                     _r(4, 3, 3, 3, seed=3, grad=True), stride=stride, pad=1)))


def _ghost_module():
    _back(train_ops.GhostModule(3, 5).train()(_r(2, 3, 6, 5, grad=True)))


def _ghost_bottleneck():
    _back(train_ops.GhostBottleneck(3, 4, 5).train()(_r(2, 3, 6, 5, grad=True)))


def _pointnet_seg():
    _back(train_ops.PointNetSeg(8, 5).train()(_r(2, 5, 16, grad=True)))


def _batchnorm():
    _back(TF.batchnorm(_r(2, 3, 6, 5, grad=True), _r(3, seed=1, grad=True), _r(3, seed=2, grad=True), torch.zeros(3), torch.ones(3), True, relu=True))


def _dwconv():
    _back(TF.dwconv(_r(2, 3, 6, 5, grad=True), _r(3, 1, 5, 5, seed=1, grad=True), _r(3, seed=2, grad=True)))


def _bmm_nt():
    _back(TF.bmm_nt(_r(2, 3, 7, grad=True), _r(2, 5, 7, seed=1, grad=True)))


def _bmm_nn():
    _back(TF.bmm_nn(_r(2, 3, 7, grad=True), _r(2, 7, 5, seed=1, grad=True)))


def _bmm_points():
    _back(train_ops._BmmPointsFn.apply(_r(2, 3, 7, grad=True), _r(2, 3, 3, seed=1, grad=True)))


CASES = {'shared_mlp': _shared_mlp, 'linear_bias': lambda: _linear(True), 'linear_no_bias': lambda: _linear(False)}
for _keep, _kname in ((KEEP_DEFAULT, 'kept'), (0, 'recomputed')):
    for _g in (True, False):
        CASES[f'conv3x3_s2_{_kname}_xgrad{int(_g)}'] = lambda k=_keep, g=_g: _conv3x3(k, g)
CASES.update({'conv2d_direct': _conv_direct, 'conv1x1': _conv1x1})
for _stride in (1, 2):
    for _keep, _kname in ((KEEP_DEFAULT, 'kept'), (0, 'recomputed')):
        for _g in (True, False):
            CASES[f'deform_s{_stride}_{_kname}_xgrad{int(_g)}'] = lambda s=_stride, k=_keep, g=_g: _deform(s, k, g)
CASES.update({'ghost_module': _ghost_module, 'ghost_bottleneck': _ghost_bottleneck, 'batchnorm_relu': _batchnorm, 'dwconv5_bias': _dwconv, 'bmm_nt': _bmm_nt,
              'bmm_nn': _bmm_nn, 'bmm_points': _bmm_points, 'pointnet_seg': _pointnet_seg})


def record(fn):
    """the calls `fn()` makes, with the recorder behind `train_ops._lib.test_library`"""
    from emu_util import emu_library
    rec = Recorder(emu_library())
    train_ops._lib.test_library = rec
    try:
        fn()
    finally:
        train_ops._lib.test_library = None
    return rec.log


def train_step():
    """the whole-model step of tests/test_train_graph.py on its committed fixture"""
    import test_train_graph
    test_train_graph._step('cpu')
