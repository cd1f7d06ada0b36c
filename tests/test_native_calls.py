"""The Python layer above the C ABI makes the native calls it made at the commit tests/golden/native_calls.json names — entry by entry, argument for argument.

The numeric tests hold results to tolerances; a wrong stride among the 18 integers of a GEMM call can hide inside one.  Here every `ach_train_*`, `ach_eval_*` and
`ach_data_*` call of the cases in tests/native_call_cases.py is recorded under the CPU emulation library (integers as they are, floats as `float.hex`, pointers as
null / non-null) and compared EXACTLY with the recording made before the glue was moved into achelous_amd/_native.py.  The fixture is never regenerated from the code
under test (tests/golden/gen_native_calls_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

import native_call_cases as NC
from achelous_amd import data, prepost, train_ops, train_functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'native_calls.json')) as _f:
    FIXTURE = json.load(_f)


def test_the_fixture_holds_every_case():
    assert set(FIXTURE['cases']) == set(NC.CASES) and all(FIXTURE['cases'].values())


@pytest.mark.parametrize('name', list(NC.CASES))
def test_case_makes_the_recorded_calls(name):
    got, want = NC.record(NC.CASES[name]), FIXTURE['cases'][name]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, f'call {k}', g, w)
    assert len(got) == len(want), (name, [c[0] for c in got], [c[0] for c in want])


def test_whole_model_step_makes_the_recorded_calls():
    """tests/test_train_graph.py::_step on its committed fixture: the count per entry first, so that a mismatch names an entry, then the hash of the whole trace"""
    trace, want = NC.record(NC.train_step), FIXTURE['train_step']
    got = NC.counts(trace)
    assert got == want['counts'], {k: (got.get(k), want['counts'].get(k)) for k in sorted(set(got) | set(want['counts'])) if got.get(k) != want['counts'].get(k)}
    assert len(trace) == want['calls']
    assert NC.digest(trace) == want['sha256']


@pytest.mark.parametrize('hook', ['train_ops._lib', 'prepost._pass_lib'])
def test_either_hook_selects_the_test_library_for_every_module(hook):
    from emu_util import emu_library
    fn = train_ops._lib if hook == 'train_ops._lib' else prepost._pass_lib
    x = torch.linspace(-1, 1, 12).reshape(3, 4)
    frame = (np.arange(6 * 9 * 3) % 251).astype(np.uint8).reshape(6, 9, 3)
    with pytest.raises(RuntimeError):
        TF.act(x, TF.ACT_RELU)                                # no test library: CPU tensors are refused
    fn.test_library = emu_library()
    try:
        assert torch.equal(TF.act(x, TF.ACT_RELU), x.clamp(min=0))
        got = data.letterbox_batch([frame], 8, dtype=torch.uint8, device='cpu')
        assert tuple(got.shape) == (1, 8, 8, 3) and torch.equal(got[0], prepost.resize_image(torch.from_numpy(frame), (8, 8)))
    finally:
        fn.test_library = None
    assert getattr(train_ops._lib, 'test_library', None) is None and getattr(prepost._pass_lib, 'test_library', None) is None
    with pytest.raises(RuntimeError):
        prepost.resize_image(torch.from_numpy(frame), (8, 8))
