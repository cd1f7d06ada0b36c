"""RepViT backbone ('rv'), CPU side (`-m "not gpu"`): the state-dict contract against the reference's key lists, the constructor message, the C ABI, and the engine's
kernels (csrc/k_repvit.h) and plan-time folds through the CPU emulation library against the rv_* fixtures of the imported reference and against the float64 restatement
tests/repvit_ref.py; one emulated training step against train_rv_s0.  tests/test_gpu_repvit.py runs the same sources on the MI355X."""
import ctypes
import os

import pytest
import torch

import achelous_amd
from achelous_amd import engine as eng_mod, train_ops
from achelous_amd.engine import DTYPE_F16, DTYPE_F32
from achelous_amd.spec import REPVIT, repvit_rows, state_dict_spec
from achelous_amd.synth import condition_state_dict, make_inputs
from emu_util import alloc_outputs, emu_library, make_engine, rel_err
from golden_util import GOLDEN_DIR, Golden
from repvit_cases import F32_TOL, NUM_POINTS, fixture_case, fixture_errors, fixture_keys, h16_bound, train_check
from repvit_ref import repvit_forward

TORCH_DTYPE = {DTYPE_F32: torch.float32, DTYPE_F16: torch.float16}
MAPS = ('map2', 'map3', 'map4', 'map5')
CTOR = ('num_det', 'num_seg', 'phi', 'resolution', 'backbone', 'neck', 'pc_seg', 'pc_channels', 'pc_classes', 'nano_head', 'spp')
BB = 'image_radar_encoder.fpn.backbone.'
SMALL = {'S0': 'rv_s0_r64', 'S1': 'rv_s1_r96', 'S2': 'rv_s2_cdf_r64'}


def _run(kw, sd, inputs, dtype, batch=None, full_taps=True, npts=NUM_POINTS):
    """one emulated forward: (engine, outputs)"""
    x, xr, xp = inputs
    B = x.shape[0] if batch is None else batch
    eng = make_engine(emu_library(), kw, B, sd, npts, dtype, full_taps=full_taps)
    td = TORCH_DTYPE[dtype]
    outs = alloc_outputs(kw, B, npts, td, 'cpu')
    eng.forward(x[:B].to(td), xr[:B].to(td), xp[:B].to(td), outs)
    return eng, outs


def _s0_at_64():
    """(constructor keywords, conditioned state dict, inputs) of an RV-S0 net at 64 x 64, batch 1, 48 points: the cheapest whole network"""
    kw = dict(num_det=7, num_seg=9, phi='S0', backbone='rv', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True, resolution=64)
    sd = condition_state_dict({k: torch.zeros_like(v) for k, v in achelous_amd.Achelous(**kw).state_dict().items()}, seed=0)
    return kw, sd, make_inputs(1, 7, resolution=64, num_points=48, pc_channels=5, radar_cells=40)


def _backbone_errors(eng, sd, image, phi):
    """rel err of every features[i] that runs and of the four maps against tests/repvit_ref.py"""
    blocks = {}
    want = repvit_forward(sd, image, phi, blocks=blocks)
    errs = {t: rel_err(eng.read_tap(t), w) for t, w in zip(MAPS, want)}
    errs.update({'backbone.' + k: rel_err(eng.read_tap('backbone.' + k), w) for k, w in blocks.items()})
    return errs


@pytest.mark.parametrize('phi', ['S0', 'S1', 'S2'])
def test_state_dict_contract(phi):
    """Key list, shapes and dtypes of spec.py and of the drop-in module equal the reference's (captured by gen_rv_golden.py into the fixture); strict loading round-trips;
    the keys of the dead tail block (features[26] of S0) are part of the state dict."""
    g = Golden(SMALL[phi])
    meta, keys = g.meta, fixture_keys(g)
    c = meta['ctor']
    spec = state_dict_spec(c['num_det'], c['num_seg'], c['phi'], c['backbone'], c['pc_channels'], c['pc_classes'], c['nano_head'], 3, c['neck'])
    assert [(k, list(s)) for k, s, _ in spec] == [(k, s) for k, s, _ in keys]
    m = achelous_amd.Achelous(**{k: c[k] for k in CTOR}).eval()
    sd = m.state_dict()
    assert list(sd.keys()) == [k for k, _, _ in keys]
    assert all(list(sd[k].shape) == s and str(sd[k].dtype).endswith(dt) for k, s, dt in keys)
    assert sum(v.numel() for v in sd.values()) == meta['n_elements'] and len(sd) == meta['n_keys']
    assert sum(k.startswith(BB) for k in sd) == {'S0': 676, 'S1': 624, 'S2': 884}[phi]
    n = len(repvit_rows(phi))
    assert n == {'S0': 26, 'S1': 24, 'S2': 34}[phi] and f'{BB}features.{n}.channel_mixer.m.2.bn.weight' in sd and (n > REPVIT[phi]['out'][-1]) == (phi == 'S0')
    drawn = condition_state_dict(sd, seed=3)
    m2 = achelous_amd.Achelous(**{k: c[k] for k in CTOR}).eval()
    m2.load_state_dict(drawn, strict=True)
    assert all(torch.equal(v, drawn[k]) for k, v in m2.state_dict().items())


def test_a_state_dict_whose_se_width_is_a_multiple_of_8_loads_and_runs():
    """The SE reduced width is read from fc1.weight: round(C / 4) = 12 / 44 at C = 48 / 176 in the fixtures, 16 / 48 where timm rounds to a multiple of 8.  Such a state dict loads
    strictly into the module, and the engine's maps equal the float64 restatement's."""
    kw, sd, inputs = _s0_at_64()
    wide, changed = {}, 0
    for k, v in sd.items():
        if '.token_mixer.1.fc' in k:
            c = sd[k.split('.token_mixer.1.')[0] + '.token_mixer.1.fc2.bias'].shape[0]
            rd = max(8, (c // 4 + 4) // 8 * 8)
            shape = {'fc1.weight': (rd, c, 1, 1), 'fc1.bias': (rd,), 'fc2.weight': (v.shape[0], rd, 1, 1), 'fc2.bias': tuple(v.shape)}[k.split('.token_mixer.1.')[1]]
            changed += tuple(v.shape) != shape
            v = torch.zeros(shape)
        wide[k] = v
    wide = condition_state_dict(wide, seed=5)
    assert changed and wide[BB + 'features.5.token_mixer.1.fc1.weight'].shape[0] == 16 and wide[BB + 'features.25.token_mixer.1.fc1.weight'].shape[0] == 48
    m = achelous_amd.Achelous(**kw).eval()
    m.load_state_dict(wide, strict=True)
    assert all(torch.equal(v, wide[k]) for k, v in m.state_dict().items())
    eng, _ = _run(kw, wide, inputs, DTYPE_F32, npts=48)
    errs = _backbone_errors(eng, wide, inputs[0], 'S0')
    assert max(errs.values()) < F32_TOL, errs


def test_constructor_message_names_repvit_and_keeps_its_phrases():
    with pytest.raises(NotImplementedError) as e:
        achelous_amd.Achelous(7, 9)
    msg = str(e.value)
    assert all(s in msg for s in ("backbone='ef'", "'pf' PoolFormer", "'rv' RepViT", 'A call that works'))
    with pytest.raises(NotImplementedError):
        state_dict_spec(7, 9, 'S0', 'ev')
    assert achelous_amd.Achelous(7, 9, phi='S0', resolution=64, backbone='rv', pc_channels=5, pc_classes=8, nano_head=True).train().training


def test_c_abi_accepts_backbone_4():
    assert eng_mod.BACKBONES['rv'] == 4
    assert 'ACH_BACKBONE_REPVIT = 4' in open(os.path.join(os.path.dirname(GOLDEN_DIR), '..', 'include', 'achelous.h')).read()
    L = emu_library().lib
    h = ctypes.c_void_p()
    cfg = eng_mod.AchConfig(7, 9, 0, 4, 64, 5, 8, 512, 1, 1, 0, 0, 0)
    assert L.ach_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    L.ach_destroy(h)


@pytest.mark.parametrize('name', ['rv_s1_r96', 'rv_s0_r64', 'rv_s2_cdf_r64'])
def test_emulated_fp32_engine_matches_the_reference_fixtures(name):
    """Every tap the fixture stores — every features[i] that runs among them — and the six outputs within the fp32 contract; a second forward on the same plan is
    bit-identical to the first."""
    g, kw, sd, inputs = fixture_case(name)
    eng, outs = _run(kw, sd, inputs, DTYPE_F32)
    errs = fixture_errors(g, outs, eng.read_tap, eng.tap_names())
    print(f'{name}: worst fp32 rel err {max(errs.values()):.2e} ({max(errs, key=errs.get)}) over {len(errs)} tensors; maps', {k: f'{errs[k]:.1e}' for k in MAPS})
    last = REPVIT[kw['phi']]['out'][-1]
    assert all(f'backbone.f{i}' in errs for i in range(last + 1)) and f'backbone.f{last + 1}' not in eng.tap_names()
    bad = {k: v for k, v in errs.items() if not v < F32_TOL}
    assert not bad, bad
    first = [o.clone() for o in outs] + [eng.read_tap(t).clone() for t in MAPS]
    x, xr, xp = inputs
    eng.forward(x, xr, xp, outs)
    assert all(torch.equal(a, b) for a, b in zip(first, list(outs) + [eng.read_tap(t) for t in MAPS]))


def test_emulated_16bit_engine_at_96():
    """fp16 storage on rv_s1_r96 (odd maps, C = 120 / 224): the bounds of the GPU test (repvit_cases.h16_bound)."""
    g, kw, sd, inputs = fixture_case('rv_s1_r96')
    eng, outs = _run(kw, sd, inputs, DTYPE_F16)
    errs = fixture_errors(g, outs, eng.read_tap, eng.tap_names(), check_sums=False)
    bound = {k: h16_bound(g, k) for k in errs}
    print('rv_s1_r96 fp16', {k: f'{v:.1e} ({bound[k]:.1e})' for k, v in sorted(errs.items(), key=lambda kv: -kv[1] / bound[kv[0]])[:12]})
    bad = {k: (v, bound[k]) for k, v in errs.items() if not v < bound[k]}
    assert not bad, bad


@pytest.mark.parametrize('var', [0.5, 1.5])
def test_folds_match_the_float64_restatement(var):
    """The plan-time folds (RepVGGDW to one depthwise 3x3, every Conv2d_BN to weights + bias) with every backbone running_var near 0.5 / near 1.5 — s = gamma /
    sqrt(var + eps) differs by a factor 1.7 between the two: every features[i] and the four maps against tests/repvit_ref.py."""
    kw, sd, inputs = _s0_at_64()
    sd = dict(sd)
    g = torch.Generator().manual_seed(11)
    for k in sd:
        if k.startswith(BB) and k.endswith('running_var'):
            sd[k] = var + 0.02 * (torch.rand(sd[k].shape, generator=g) - 0.5)
    eng, _ = _run(kw, sd, inputs, DTYPE_F32, npts=48)
    errs = _backbone_errors(eng, sd, inputs[0], 'S0')
    print(f'running_var ~ {var}: worst {max(errs.values()):.2e} ({max(errs, key=errs.get)})')
    assert len(errs) == 30 and max(errs.values()) < F32_TOL, errs


def test_changed_weights_change_the_output():
    """The folds are rebuilt when weights change: a changed running_var of a conv1.bn (inside the folded centre tap) and a changed SE fc2.bias each move map2, and the
    moved result is the restatement's."""
    kw, sd, inputs = _s0_at_64()
    base = _run(kw, sd, inputs, DTYPE_F32, npts=48)[0].read_tap('map2').clone()
    for key, new in ((BB + 'features.1.token_mixer.0.conv1.bn.running_var', lambda v: v * 4.0), (BB + 'features.1.token_mixer.1.fc2.bias', lambda v: v + 1.5)):
        mod = dict(sd)
        mod[key] = new(sd[key])
        eng, _ = _run(kw, mod, inputs, DTYPE_F32, npts=48)
        got = eng.read_tap('map2')
        want = repvit_forward(mod, inputs[0], 'S0')[0]
        assert rel_err(got, base) > 1e-2, key
        assert rel_err(got, want) < F32_TOL, key


@pytest.mark.parametrize('dtype', [pytest.param(DTYPE_F32, id='f32'), pytest.param(DTYPE_F16, id='f16')])
def test_emulated_frame_is_bit_identical_whatever_batch_it_sits_in(dtype):
    """The SE partial sums are cut by the map alone and merged in a fixed order, MLP tiles are cut per sample: frame 1 of the B = 3 run equals the B = 1 run of that
    frame, bit for bit — at 64 x 64, where the last map has 4 pixels per sample and a 16-pixel tile would hold all three."""
    g, kw, sd, (x, xr, xp) = fixture_case('rv_s0_r64')
    e3, o3 = _run(kw, sd, (x, xr, xp), dtype)
    e1, o1 = _run(kw, sd, (x[1:2], xr[1:2], xp[1:2]), dtype)
    for a, b in zip(o3, o1):
        assert torch.equal(a[1:2], b)
    for t in MAPS:
        assert torch.equal(e3.read_tap(t)[1:2], e1.read_tap(t)), t


@pytest.mark.parametrize('phi', ['S0', 'S1', 'S2'])
def test_repvit_is_one_in_order_segment_within_the_launch_budget(phi):
    """2 per stride-1 block that runs + 3 per stride-2 block + 2 for the stem, plus one gate launch per SE block (the gate is its own launch); the dead tail block of
    S0 plans nothing; all on the caller's stream in plan order."""
    g, kw, sd, _ = fixture_case(SMALL[phi])
    eng = make_engine(emu_library(), kw, 1, sd, 48, DTYPE_F32, full_taps=False)
    ops = [o for o in eng.op_schedule() if o['op'].startswith(BB)]
    rows = repvit_rows(phi)[:REPVIT[phi]['out'][-1]]
    s1, s2, se = sum(r[2] == 1 for r in rows), sum(r[2] == 2 for r in rows), sum(r[3] for r in rows)
    assert (s1, s2, se) == {'S0': (22, 3, 10), 'S1': (21, 3, 9), 'S2': (31, 3, 14)}[phi]
    assert len(ops) == 2 * s1 + 3 * s2 + 2 + se and all(o['stream'] == 0 for o in ops)
    names = [o['op'].rsplit('.', 1)[-1] for o in ops]
    assert names.count('dw') == s1 + s2 and names.count('mlp') == s1 + s2 and names.count('gate') == se and names.count('pw') == s2
    assert not any(f".features.{REPVIT[phi]['out'][-1] + 1}." in o['op'] for o in ops)


def test_emulated_training_step_matches_the_reference():
    """train_graph.TrainGraph.repvit on the emulated training kernels against one float64 training step of the imported reference (repvit_cases.train_check)."""
    train_ops._lib.test_library = emu_library()
    try:
        worst = train_check('cpu')
        print('largest relative errors (ours, torch fp32):', [(f'{e:.1e}', f'{r:.1e}', k) for e, r, k in worst])
    finally:
        train_ops._lib.test_library = None
