"""tests/test_engine_envelope.py's comparison on the MI355X: the HIP library against the oracle (computed on the CPU), every output and every
tap the oracle also has, at the widths around and past 32 sixteen-pixel segments per radar row — batch 2, so the per-sample strides matter.
On the GPU the columns rc_front_kernel once skipped held whatever the arena held before, not zeros."""
import pytest
import torch

from achelous_amd import engine as eng_mod
from emu_util import alloc_outputs, make_engine
from test_emulated_engine import TORCH_DTYPE, _setup
from test_engine_envelope import DT, RADAR_TAPS, TOL, compare, oracle_forward, radar_sequence

pytestmark = pytest.mark.gpu

CASES = [('en_s0', r, d) for r in (512, 544, 640) for d in ('f32', 'bf16', 'f16')] + [('en_s0_cdf', 640, 'bf16'), ('mv_s2', 640, 'bf16')]


def gpu_forward(eng, xs, outs):
    eng.forward(*xs, outs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize('name,res,dt', CASES, ids=[f'{n}-{r}-{d}' for n, r, d in CASES])
def test_gpu_envelope_forward_matches_oracle_tap_by_tap(name, res, dt):
    dtype, td = DT[dt], TORCH_DTYPE[DT[dt]]
    ref_outs, ref_taps = oracle_forward(name, res, 2)
    kw, sd, inputs = _setup(name, res, 2, 16)
    eng = make_engine(eng_mod.hip_library(), kw, 2, sd, 16, dtype)
    outs = alloc_outputs(kw, 2, 16, td, 'cuda')
    got = gpu_forward(eng, [t.cuda().to(td) for t in inputs], outs)
    seen = compare(eng, got, ref_outs, ref_taps, TOL[dtype], report=f'{name}-{res}-{dt}')
    missing = [t for t in RADAR_TAPS if t not in seen]
    assert not missing, missing


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_gpu_second_forward_at_544_with_other_radar_cells(dt):
    """Two forwards on one plan with different radar cells: a value of the first forward left in the columns past 512 would show in the second."""
    dtype, td = DT[dt], TORCH_DTYPE[DT[dt]]
    kw, sd, (x, xr, xp) = _setup('en_s0', 544, 2, 16)
    eng = make_engine(eng_mod.hip_library(), kw, 2, sd, 16, dtype)
    outs = alloc_outputs(kw, 2, 16, td, 'cuda')
    gpu_forward(eng, [t.cuda().to(td) for t in (x, xr, xp)], outs)
    ref_outs, ref_taps = oracle_forward('en_s0', 544, 2, seed=8)
    inputs = _setup('en_s0', 544, 2, 16, seed=8)[2]
    assert not torch.equal(inputs[1], xr)
    got = gpu_forward(eng, [t.cuda().to(td) for t in inputs], outs)
    seen = compare(eng, got, ref_outs, ref_taps, TOL[dtype], report=f'en_s0-544-{dt}-second')
    assert all(t in seen for t in RADAR_TAPS)


def test_gpu_radar_skip_is_bit_identical_over_five_forwards_at_512():
    """The 32-segment edge on the hardware: 40 cells, dense, all-zero, 3 cells, 40 cells on one bf16 plan, default options against radar_skip = 0."""
    kw, sd, (x, _, xp) = _setup('en_s0', 512, 1, 16)
    engines = []
    for opts in ({}, {'radar_skip': 0}):
        eng = eng_mod.NativeEngine(eng_mod.hip_library(), num_det=kw['num_det'], num_seg=kw['num_seg'], phi=kw['phi'], backbone=kw['backbone'], resolution=512,
                                   pc_channels=kw['pc_channels'], pc_classes=kw['pc_classes'], num_points=16, nano_head=kw['nano_head'], spp=kw['spp'], dtype=eng_mod.DTYPE_BF16)
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_option('full_taps', 1)
        eng.load_state_dict(sd)
        eng.plan(1)
        engines.append(eng)
    outs = alloc_outputs(kw, 1, 16, torch.bfloat16, 'cuda')
    xg, pg = x.cuda().bfloat16(), xp.cuda().bfloat16()
    for step, xr in enumerate(radar_sequence(512)):
        taps = []
        for eng in engines:
            gpu_forward(eng, [xg, xr.cuda().bfloat16(), pg], outs)
            taps.append([eng.read_tap(t) for t in ('radar.b0', 'radar.b1', 'r5')])
        for t, a, b in zip(('radar.b0', 'radar.b1', 'r5'), *taps):
            assert torch.isfinite(a).all() and torch.equal(a, b), (step, t)
