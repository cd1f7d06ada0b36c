"""PoolFormer backbone ('pf'), CPU side (`-m "not gpu"`): the state-dict contract against the reference's key lists, the constructor / training-mode errors, the C ABI,
and the engine's kernels (csrc/k_poolformer.h) through the CPU emulation library against the pf_* fixtures of the imported reference and against the float64
restatement tests/poolformer_ref.py.  tests/test_gpu_poolformer.py runs the same sources on the MI355X."""
import ctypes
import json
import os

import pytest
import torch

import achelous_amd
from achelous_amd import engine as eng_mod
from achelous_amd.engine import DTYPE_BF16, DTYPE_F16, DTYPE_F32
from achelous_amd.spec import state_dict_spec
from achelous_amd.synth import condition_state_dict, make_inputs
from emu_util import alloc_outputs, emu_library, make_engine, rel_err
from golden_util import GOLDEN_DIR, Golden
from poolformer_cases import F32_TOL, FIXTURES, NUM_POINTS, OUTPUTS, fixture_case, fixture_errors, fixture_keys, h16_bound
from poolformer_ref import poolformer_forward

TORCH_DTYPE = {DTYPE_F32: torch.float32, DTYPE_BF16: torch.bfloat16, DTYPE_F16: torch.float16}
MAPS = ('map2', 'map3', 'map4', 'map5')
CTOR = ('num_det', 'num_seg', 'phi', 'resolution', 'backbone', 'neck', 'pc_seg', 'pc_channels', 'pc_classes', 'nano_head', 'spp')


def _run(kw, sd, inputs, dtype, batch=None, full_taps=True, npts=NUM_POINTS):
    """one emulated forward: (engine, outputs)"""
    x, xr, xp = inputs
    B = x.shape[0] if batch is None else batch
    eng = make_engine(emu_library(), kw, B, sd, npts, dtype, full_taps=full_taps)
    td = TORCH_DTYPE[dtype]
    outs = alloc_outputs(kw, B, npts, td, 'cpu')
    eng.forward(x[:B].to(td), xr[:B].to(td), xp[:B].to(td), outs)
    return eng, outs


@pytest.mark.parametrize('name', FIXTURES)
def test_state_dict_contract(name):
    """Key list, shapes and dtypes of spec.py and of the drop-in module equal the reference's (captured by gen_pf_golden.py into the fixture); strict loading round-trips."""
    g = Golden(name)
    meta, keys = g.meta, fixture_keys(g)
    c = meta['ctor']
    spec = state_dict_spec(c['num_det'], c['num_seg'], c['phi'], c['backbone'], c['pc_channels'], c['pc_classes'], c['nano_head'], 3, c['neck'])
    assert [(k, list(s)) for k, s, _ in spec] == [(k, s) for k, s, _ in keys]
    m = achelous_amd.Achelous(**{k: c[k] for k in CTOR}).eval()
    sd = m.state_dict()
    assert list(sd.keys()) == [k for k, _, _ in keys]
    assert all(list(sd[k].shape) == s and str(sd[k].dtype).endswith(dt) for k, s, dt in keys)
    assert sum(v.numel() for v in sd.values()) == meta['n_elements'] and len(sd) == meta['n_keys']
    n_backbone = sum(k.startswith('image_radar_encoder.fpn.backbone.') for k in sd)
    assert (len(sd), n_backbone) == {('S0', 'gdf'): (747, 136), ('S0', 'cdf'): (735, 136), ('S1', 'gdf'): (867, 256), ('S2', 'gdf'): (987, 376)}[c['phi'], c['neck']]
    drawn = condition_state_dict(sd, seed=3)
    m2 = achelous_amd.Achelous(**{k: c[k] for k in CTOR}).eval()
    m2.load_state_dict(drawn, strict=True)
    assert all(torch.equal(v, drawn[k]) for k, v in m2.state_dict().items())


def test_layer_scales_are_drawn_like_gamma_and_no_other_key_moves():
    """synth.condition_state_dict: layer_scale_1 / layer_scale_2 in U(0.2, 0.6) — under the generic U(-0.1, 0.1) rule an error inside the MLP would reach the block
    output attenuated twenty-fold and pass an fp32 tolerance.  The draw is a function of (seed, key): the keys of an EdgeNeXt model are what they were."""
    m = achelous_amd.Achelous(7, 9, phi='S0', resolution=64, backbone='pf', pc_channels=5, pc_classes=8, nano_head=True).eval()
    sd = condition_state_dict(m.state_dict(), seed=0)
    scales = [v for k, v in sd.items() if k.rsplit('.', 1)[-1] in ('layer_scale_1', 'layer_scale_2')]
    assert len(scales) == 24 and all(0.2 <= float(v.min()) and float(v.max()) <= 0.6 for v in scales)
    meta = json.load(open(os.path.join(GOLDEN_DIR, 'en_s0.keys.json')))
    blank = {k: torch.zeros(s, dtype=getattr(torch, dt)) for k, s, dt in meta['keys']}
    en = condition_state_dict(blank, seed=0)
    k = 'image_radar_encoder.fpn.backbone.stages.0.0.gamma'
    # (recorded from the draw as it was before the layer-scale rule: one tensor, and the sum of |value| over all 771 tensors)
    assert abs(float(en[k].double().sum()) - 13.920533865690231) < 1e-9
    assert abs(sum(float(v.double().abs().sum()) for v in en.values()) - 227500.12114285014) < 1e-6


def test_bad_arguments_still_raise_one_message_and_training_is_refused():
    with pytest.raises(NotImplementedError) as e:
        achelous_amd.Achelous(7, 9)
    assert "backbone='ef'" in str(e.value) and "'pf' PoolFormer" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        achelous_amd.Achelous(7, 99, phi='L', backbone='xx', neck='rdf', image_channels=1)
    msg = str(e.value)
    assert msg.count('unsupported constructor arguments') == 1 and all(s in msg for s in ("backbone='xx'", "phi='L'", "neck='rdf'", 'image_channels=1'))
    with pytest.raises(NotImplementedError):
        state_dict_spec(7, 9, 'S0', 'pv')
    m = achelous_amd.Achelous(7, 9, phi='S0', resolution=64, backbone='pf', pc_channels=5, pc_classes=8, nano_head=True)
    assert m.eval() is m
    with pytest.raises(NotImplementedError, match="'pf'"):
        m.train()
    assert not m.training
    from achelous_amd.train_graph import TrainGraph
    with pytest.raises(NotImplementedError, match="'pf'"):
        TrainGraph(m)
    assert achelous_amd.Achelous(7, 9, phi='S0', resolution=64, backbone='en', pc_channels=5, pc_classes=8, nano_head=True).train().training


def test_c_abi_accepts_backbone_2_and_refuses_3():
    assert eng_mod.BACKBONES['pf'] == 2
    assert 'ACH_BACKBONE_POOLFORMER = 2' in open(os.path.join(os.path.dirname(GOLDEN_DIR), '..', 'include', 'achelous.h')).read()
    L = emu_library().lib
    h = ctypes.c_void_p()
    cfg = eng_mod.AchConfig(7, 9, 0, 2, 64, 5, 8, 512, 1, 1, 0, 0, 0)
    assert L.ach_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    L.ach_destroy(h)
    h = ctypes.c_void_p()
    cfg = eng_mod.AchConfig(7, 9, 0, 3, 64, 5, 8, 512, 1, 1, 0, 0, 0)
    assert L.ach_create(ctypes.byref(cfg), ctypes.byref(h)) == -2 and L.ach_last_error(None) == b"backbone must be 'en' or 'mv'" and not h.value


@pytest.mark.parametrize('name', ['pf_s0_r64', 'pf_s1_r96', 'pf_s0_cdf_r64'])
def test_emulated_fp32_engine_matches_the_reference_fixtures(name):
    """Every tap the fixture stores and the six outputs within the fp32 contract (measured worst: 4.3e-6 / 7.8e-6 / 4.3e-6; the four maps 2.8e-7 .. 8.4e-7);
    a second forward on the same plan is bit-identical to the first."""
    g, kw, sd, inputs = fixture_case(name)
    eng, outs = _run(kw, sd, inputs, DTYPE_F32)
    errs = fixture_errors(g, outs, eng.read_tap, eng.tap_names())
    print(f'{name}: worst fp32 rel err {max(errs.values()):.2e} ({max(errs, key=errs.get)}) over {len(errs)} tensors; maps', {k: f'{errs[k]:.1e}' for k in MAPS})
    assert len(errs) >= 40 and all(f'backbone.s{i}.b0' in errs for i in range(4))
    bad = {k: v for k, v in errs.items() if not v < F32_TOL}
    assert not bad, bad
    first = [o.clone() for o in outs] + [eng.read_tap(t).clone() for t in MAPS]
    x, xr, xp = inputs
    eng.forward(x, xr, xp, outs)
    assert all(torch.equal(a, b) for a, b in zip(first, list(outs) + [eng.read_tap(t) for t in MAPS]))


@pytest.mark.parametrize('name', ['pf_s0_r64', 'pf_s1_r96'])
def test_emulated_one_tile_per_wave_mlp_form_matches_the_fixtures(name):
    """Maps of more than 1024 pixels per sample run pf_mlp_kernel with one tile per wave (four tiles per workgroup) — none of the small fixtures has such a map, so
    the form is forced here with the existing option mlp_split = 0: tiles are cut per sample, so at 64 x 64 the stride-32 tile holds 4 valid rows of 16."""
    from achelous_amd.engine import NativeEngine
    g, kw, sd, (x, xr, xp) = fixture_case(name)
    B = x.shape[0]
    eng = NativeEngine(emu_library(), num_det=kw['num_det'], num_seg=kw['num_seg'], phi=kw['phi'], backbone=kw['backbone'], resolution=kw['resolution'],
                       pc_channels=kw['pc_channels'], pc_classes=kw['pc_classes'], num_points=NUM_POINTS, nano_head=kw['nano_head'], spp=kw['spp'], dtype=DTYPE_F32,
                       neck=kw['neck'], pc_seg=kw['pc_seg'])
    eng.set_option('full_taps', 1)
    eng.set_option('mlp_split', 0)
    eng.load_state_dict(sd)
    eng.plan(B)
    outs = alloc_outputs(kw, B, NUM_POINTS, torch.float32, 'cpu')
    eng.forward(x, xr, xp, outs)
    errs = fixture_errors(g, outs, eng.read_tap, eng.tap_names())
    assert max(errs.values()) < F32_TOL, {k: v for k, v in errs.items() if not v < F32_TOL}


def test_emulated_s2_widths_match_the_float64_restatement():
    """S2 (64 / 144 / 288 channels, 36 blocks) has no small fixture: the four maps at 64 x 64 against tests/poolformer_ref.py, same bound."""
    kw = dict(num_det=7, num_seg=9, phi='S2', backbone='pf', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True, resolution=64)
    sd = condition_state_dict({k: torch.zeros_like(v) for k, v in achelous_amd.Achelous(**kw).state_dict().items()}, seed=0)
    inputs = make_inputs(1, 7, resolution=64, num_points=48, pc_channels=5, radar_cells=40)
    blocks = {}
    want = poolformer_forward(sd, inputs[0], 'S2', blocks=blocks)
    eng, _ = _run(kw, sd, inputs, DTYPE_F32, npts=48)
    errs = {t: rel_err(eng.read_tap(t), w) for t, w in zip(MAPS, want)}
    errs.update({'backbone.' + k: rel_err(eng.read_tap('backbone.' + k), w) for k, w in blocks.items()})
    print('S2 at 64 x 64, fp32 against poolformer_ref: worst', f'{max(errs.values()):.2e}', {k: f'{errs[k]:.1e}' for k in MAPS})
    assert len(errs) == 40 and max(errs.values()) < F32_TOL, errs


@pytest.mark.parametrize('dtype', [pytest.param(DTYPE_F32, id='f32'), pytest.param(DTYPE_F16, id='f16')])
def test_emulated_frame_is_bit_identical_whatever_batch_it_sits_in(dtype):
    """The partial moments are cut by (H, W, C) alone and reduced in a fixed order: frame 1 of the B = 3 run equals the B = 1 run of that frame, bit for bit —
    at 64 x 64, where the stride-32 map has 4 pixels per sample and a 16-pixel tile would hold all three."""
    g, kw, sd, (x, xr, xp) = fixture_case('pf_s0_r64')
    e3, o3 = _run(kw, sd, (x, xr, xp), dtype)
    e1, o1 = _run(kw, sd, (x[1:2], xr[1:2], xp[1:2]), dtype)
    for a, b in zip(o3, o1):
        assert torch.equal(a[1:2], b)
    for t in MAPS:
        assert torch.equal(e3.read_tap(t)[1:2], e1.read_tap(t)), t


@pytest.mark.parametrize('dtype', [pytest.param(DTYPE_F16, id='f16'), pytest.param(DTYPE_BF16, id='bf16')])
def test_emulated_16bit_engines_at_96(dtype):
    """fp16 and bf16 storage on pf_s1_r96 (odd maps, C = 120): the bounds of the GPU test (poolformer_cases.h16_bound)."""
    g, kw, sd, inputs = fixture_case('pf_s1_r96')
    eng, outs = _run(kw, sd, inputs, dtype)
    errs = fixture_errors(g, outs, eng.read_tap, eng.tap_names(), check_sums=False)
    bound = {k: h16_bound(g, k) for k in errs}
    print('pf_s1_r96', TORCH_DTYPE[dtype], {k: f'{v:.1e} ({bound[k]:.1e})' for k, v in sorted(errs.items(), key=lambda kv: -kv[1] / bound[kv[0]])[:12]})
    bad = {k: (v, bound[k]) for k, v in errs.items() if not v < bound[k]}
    assert not bad, bad


def test_emulated_f16_storage_saturates_and_counts_instead_of_overflowing():
    """A patch-embedding weight scaled so that activations exceed 65 504: the fp16 engine's outputs stay finite and ach_count_saturated counts the clamped elements (the
    PoolFormer kernels store through the clamping Store<T> path and take their moments from the values as stored); with the conditioned weights it counts none."""
    g, kw, sd, (x, xr, xp) = fixture_case('pf_s0_r64')
    big = dict(sd)
    k = 'image_radar_encoder.fpn.backbone.patch_embed.proj.weight'
    big[k] = sd[k] * 3e5
    counts = {}
    for tag, state in (('conditioned', sd), ('large', big)):
        eng, outs = _run(kw, state, (x, xr, xp), DTYPE_F16, full_taps=False)
        counts[tag] = eng.count_saturated()
        assert all(torch.isfinite(o.float()).all() for o in outs), tag
    assert counts['conditioned'] == 0 and counts['large'] > 0, counts


def test_existing_plan_schedules_come_out_unchanged():
    """The listing tests/golden/gen_plan_schedules.py writes for the existing configurations equals the committed file: PoolFormer changes no schedule."""
    import plan_schedules as PS
    with open(PS.SCHEDULES_JSON) as f:
        want = json.load(f)['plans']
    got = {pid: PS.summary(full) for pid, full in PS.all_plans(emu_library())}
    assert len(want) == 160 and list(got) == list(want) and [pid for pid in want if got[pid] != want[pid]] == []


def test_poolformer_is_one_in_order_segment_within_the_launch_budget():
    """The backbone's launches run on the caller's stream in plan order, two per block, at most 2 * blocks + 12 in all (stem, 3 down-sampling convs, 3 moments passes,
    4 fork norms = 11)."""
    g, kw, sd, _ = fixture_case('pf_s0_r64')
    eng = make_engine(emu_library(), kw, 1, sd, 48, DTYPE_F32, full_taps=False)
    ops = [o for o in eng.op_schedule() if o['op'].startswith('image_radar_encoder.fpn.backbone.')]
    assert len(ops) == 2 * 12 + 11 and all(o['stream'] == 0 for o in ops)
    names = [o['op'].rsplit('.', 1)[-1] for o in ops]
    assert names.count('mixer') == 12 and names.count('mlp') == 12 and names.count('moments') == 3 and names[0] == 'patch_embed'
