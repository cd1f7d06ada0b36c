"""The engine against its oracle over the resolution envelope it accepts (multiples of 32 from 64 up), on the CPU emulation build,
TAP BY TAP.  A radar map wider than 512 pixels has more than 32 sixteen-pixel segments per row; rc_front_kernel (k_conv3.h) once walked
them through one 32-bit mask and left the columns from 512 on of the first RCBlock's output unwritten.  Every OUTPUT of the bf16 engine
stayed inside its bound with `radar.b0` 97 % wrong, so this file holds every tap the oracle also has to the bound, and requires the
radar taps to be among them."""
import pytest
import torch

from achelous_amd.engine import DTYPE_BF16, DTYPE_F16, DTYPE_F32, NativeEngine
from achelous_amd.synth import make_inputs
from emu_util import alloc_outputs, emu_library, make_engine, rel_err
from oracle.achelous_oracle import AchelousOracle
from test_emulated_engine import ORACLE_KEYS, TORCH_DTYPE, _setup

# the bounds of test_emulated_forward_matches_oracle against this oracle
TOL = {DTYPE_F32: 2e-5, DTYPE_BF16: 6e-2, DTYPE_F16: 8e-3}
DT = {'f32': DTYPE_F32, 'bf16': DTYPE_BF16, 'f16': DTYPE_F16}
RADAR_TAPS = [f'radar.b{i}' for i in range(8)] + ['r3', 'r4', 'r5']
OUT_NAMES = ('det0', 'det1', 'det2', 'se', 'lane', 'pc')
MAX_RESOLUTION = 864          # the largest resolution the engine plans: 54 segments per radar row (a full span of 32 and a partial one), a 27 x 27 map in the SPP tile

# en_s0: the multiples of 32 the other files leave out below 416; 352 / 384: 11 x 11 and 12 x 12 maps at stride 32; 448 / 480: past the device NMS limit;
# 512: exactly 32 segments, the last width with the occupancy forms; 544 / 576 / 640: 34 / 36 / 40 segments, the head's unfused layer form from 544
CASES = [('en_s0', r, d) for r in (192, 224, 256, 288, 352, 384, 416, 448, 480, 512, 544, 576, 640) for d in ('f32', 'bf16', 'f16')]
CASES += [(n, r, d) for n in ('en_s1', 'en_s2', 'en_s0_cdf') for r in (352, 512, 544) for d in ('f32', 'bf16')]
CASES += [('mv_s2', r, d) for r in (512, 640) for d in ('f32', 'bf16')]
CASES += [('en_s0', MAX_RESOLUTION, 'f32')]

_oracle = {}


def oracle_forward(name, res, batch=1, seed=7):
    """(outputs, taps) of the oracle on the `_setup` weights and inputs; the cases of one (name, res) are adjacent, so one entry is kept."""
    if (name, res, batch, seed) not in _oracle:
        _oracle.clear()
        kw, sd, (x, xr, xp) = _setup(name, res, batch, 16, seed)
        orc = AchelousOracle(sd, **{k: kw[k] for k in ORACLE_KEYS})
        with torch.no_grad():
            det, se, lane, pc = orc.forward(x, xr, xp)
        _oracle[(name, res, batch, seed)] = ((det[0], det[1], det[2], se, lane, pc), dict(orc.taps))
    return _oracle[(name, res, batch, seed)]


def compare(eng, outs, ref_outs, ref_taps, tol, report=None):
    """Every output and every tap the oracle also has: finite, and within `tol`.  Returns the names compared; the first miss in plan order is the one reported.
    `report`: print the worst tap and the worst output under that label before asserting."""
    seen = []
    for n, a, b in zip(OUT_NAMES, outs, ref_outs):
        assert torch.isfinite(a.float()).all(), n
    errs = []
    for tap in eng.tap_names():
        if tap in ref_taps:
            t = eng.read_tap(tap)
            assert torch.isfinite(t).all(), tap
            errs.append((tap, rel_err(t, ref_taps[tap])))
            seen.append(tap)
    errs += [(n, rel_err(a.float(), b)) for n, a, b in zip(OUT_NAMES, outs, ref_outs)]
    worst_out = max(e for n, e in errs if n in OUT_NAMES)
    if report:
        wt = max((e, n) for n, e in errs if n not in OUT_NAMES)
        print(f'{report}: worst tap {wt[1]} {wt[0]:.3g}, worst output {worst_out:.3g}, radar.b0 {dict(errs)["radar.b0"]:.3g} (bound {tol:g})')
    for n, e in errs:
        assert e < tol, f'{n}: {e:.3g} against {tol:g} (worst output {worst_out:.3g})'
    return seen


@pytest.mark.parametrize('name,res,dt', CASES, ids=[f'{n}-{r}-{d}' for n, r, d in CASES])
def test_envelope_forward_matches_oracle_tap_by_tap(name, res, dt):
    dtype, td = DT[dt], TORCH_DTYPE[DT[dt]]
    ref_outs, ref_taps = oracle_forward(name, res)
    kw, sd, (x, xr, xp) = _setup(name, res, 1, 16)
    eng = make_engine(emu_library(), kw, 1, sd, 16, dtype)
    outs = alloc_outputs(kw, 1, 16, td, 'cpu')
    eng.forward(x.to(td), xr.to(td), xp.to(td), outs)
    seen = compare(eng, outs, ref_outs, ref_taps, TOL[dtype], report=f'{name}-{res}-{dt}')
    missing = [t for t in RADAR_TAPS if t not in seen]
    assert not missing, missing


@pytest.mark.parametrize('res', [416, 544])
def test_mobilevit_refuses_an_odd_token_grid(res):
    """R / 32 odd: the reference's rearrange into 2 x 2 patches (and the oracle) cannot run; the engine refuses when the plan is built."""
    kw, sd, _ = _setup('mv_s2', res, 1, 16)
    eng = NativeEngine(emu_library(), num_det=kw['num_det'], num_seg=kw['num_seg'], phi=kw['phi'], backbone=kw['backbone'], resolution=res,
                       pc_channels=kw['pc_channels'], pc_classes=kw['pc_classes'], num_points=16, nano_head=kw['nano_head'], spp=kw['spp'], dtype=DTYPE_F32)
    eng.load_state_dict(sd)
    with pytest.raises(NotImplementedError, match='MobileViT token count'):
        eng.plan(1)


def radar_sequence(res):
    """Five radar maps for consecutive forwards on one plan: 40 cells, dense, all-zero, 3 cells, 40 cells."""
    maps = []
    for seed, cells in ((21, 40), (22, -1), (23, 0), (24, 3), (25, 40)):
        xr = make_inputs(1, seed, resolution=res, num_points=16, pc_channels=3, radar_cells=max(cells, 1), dense_radar=cells < 0)[1]
        maps.append(torch.zeros_like(xr) if cells == 0 else xr)
    return maps


VARIANTS = [{}, {'radar_skip': 0, 'radar_bg': 0, 'radar_pool_sparse': 0}, {'radar_rows4': 2}, {'radar_rows4': 2, 'radar_compact': 0}]


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('res', [512, 544, 640])
def test_envelope_radar_options_are_bit_identical_over_five_forwards(res, dt):
    """test_emulated_radar_skip_is_bit_identical's check at the 32-segment edge (512: `1u << ctiles`, `lane < 32` and the segment masks on their
    boundary, with stale state from the previous forward in the background mode) and past it (544 / 640: the occupancy forms are off, the
    options must be no-ops).  The f32 engine is also held to the oracle after every forward, dense map included."""
    dtype, td = DT[dt], TORCH_DTYPE[DT[dt]]
    kw, sd, (x, _, xp) = _setup('en_s0', res, 1, 16)
    maps = radar_sequence(res)
    engines = []
    for opts in VARIANTS:
        eng = NativeEngine(emu_library(), num_det=kw['num_det'], num_seg=kw['num_seg'], phi=kw['phi'], backbone=kw['backbone'], resolution=res,
                           pc_channels=kw['pc_channels'], pc_classes=kw['pc_classes'], num_points=16, nano_head=kw['nano_head'], spp=kw['spp'], dtype=dtype)
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_option('full_taps', 1)
        eng.load_state_dict(sd)
        eng.plan(1)
        engines.append(eng)
    orc = AchelousOracle(sd, **{k: kw[k] for k in ORACLE_KEYS}) if dtype == DTYPE_F32 else None
    outs = alloc_outputs(kw, 1, 16, td, 'cpu')
    for step, xr in enumerate(maps):
        taps = []
        for eng in engines:
            eng.forward(x.to(td), xr.to(td), xp.to(td), outs)
            taps.append([eng.read_tap(t) for t in ('radar.b0', 'radar.b1', 'r5')])
        for v, other in enumerate(taps[1:], 1):
            for t, a, b in zip(('radar.b0', 'radar.b1', 'r5'), taps[0], other):
                assert torch.isfinite(a).all() and torch.equal(a, b), (step, VARIANTS[v], t)
        if orc is not None:
            with torch.no_grad():
                orc.forward(x, xr, xp)
            for t, a in zip(('radar.b0', 'radar.b1', 'r5'), taps[0]):
                assert rel_err(a, orc.taps[t]) < TOL[DTYPE_F32], (step, t, rel_err(a, orc.taps[t]))


@pytest.mark.parametrize('res', [MAX_RESOLUTION + 32, 1056])
def test_plan_refuses_resolutions_past_the_verified_envelope(res):
    """The forward is verified up to MAX_RESOLUTION.  Above it the SPP pooling tile is too small for the stride-32 map and nothing else has been
    looked at (1056: 66 segments per radar row, more than a wavefront has lanes), so the engine says so, naming the limit."""
    kw, sd, _ = _setup('en_s0', res, 1, 16)
    with pytest.raises(NotImplementedError, match=str(MAX_RESOLUTION)):
        make_engine(emu_library(), kw, 1, sd, 16, DTYPE_F32)
