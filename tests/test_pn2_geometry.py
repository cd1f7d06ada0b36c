"""The geometry kernels of the PointNet++ branch (csrc/k_pn2.h: farthest-point sampling, ball query + grouping, 3-NN interpolation; their adjoints in csrc/k_train3.h) on
the inputs where their tie rules decide the result: clouds of a few dozen distinct points among N (tests/pn2_cases.py `resampled`: what the reference's loader produces),
lattice clouds whose squared distances are exact in fp32 (`lattice`: members ON a ball's boundary, ties at equal non-zero distances), ragged sizes, every supported
`num_points` bucket edge, every launch form, the empty ball and — under emulation only — non-finite coordinates.

Truth is oracle/pointnet2_oracle.py.  Index selections, gathers and single fp32 subtractions are compared BIT for bit; floating sums are held to the rule of
tests/test_train_functional.py: max(FLOOR, F_YARD x yardstick) in the max-norm relative metric, the yardstick being the same statement evaluated in float32 on the CPU
against float64.  Every case asserts, from the oracle alone, that it holds the ties it was built for.  CPU: the kernel sources under the emulation library; `-m gpu`: the
HIP kernels on the MI355X, inputs built the same way.  DESIGN.md section 5b lists the cases and the measured error / yardstick pairs."""
import numpy as np
import pytest
import torch

import achelous_amd
from achelous_amd import train_ops, train_functional as TF
from achelous_amd.engine import DTYPE_BF16, DTYPE_F32
from achelous_amd.synth import condition_state_dict, make_inputs
from oracle import pointnet2_oracle as po
from oracle.achelous_oracle import AchelousOracle

import pn2_cases as pc
from test_pointnet2 import KWS, _is_index_tap, _state_dict
from test_pointnet2 import _rel as _rel_tap
from test_train_functional import FLOOR, F_YARD, _r, _rel

LATTICE = 'lattice'          # in the `distinct` column of a case: a lattice cloud instead of a resampled one


def _emulated(fn, *a):
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        fn('cpu', *a)
    finally:
        train_ops._lib.test_library = None


def _clouds(batch, n, distinct, seed):
    """[batch, n, 3] float32"""
    return pc.lattice_clouds(batch, n, seed) if distinct == LATTICE else pc.cloud(batch, n, distinct, seed)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _bit_equal(got, want):
    want = torch.as_tensor(want)
    return tuple(got.shape) == tuple(want.shape) and torch.equal(_bits(got), _bits(want))


def _held(what, name, got, truth, f32):
    err, yard = _rel(got, truth), _rel(f32, truth)
    bound = max(FLOOR, F_YARD * yard)
    print(f'{what}: {name}: error {err:.2e}, yardstick {yard:.2e}, bound {bound:.2e}')
    assert err < bound, (what, name, err, yard, bound)


# ------------------------------------------------------------------------------------------------------------------ farthest-point sampling
# (n, npoint, distinct): full and partial lanes at every points-per-lane template (1, 4, 8, 16), n = 65 (one point in the second slot), npoint = n, one single point
FPS_CASES = [(512, 256, 40), (512, 256, 5), (512, 256, 300), (1024, 512, 60), (1000, 300, 60), (200, 64, 7), (65, 65, 3), (64, 64, 64), (640, 320, 1), (500, 250, LATTICE)]


def _fps_case(dev, n, npoint, distinct):
    B = 3
    xyz = _clouds(B, n, distinct, seed=n + npoint)
    idx, new_xyz = TF.pn2_fps(xyz.to(dev), npoint)
    ties = zeros = 0
    for b in range(B):
        t, z = pc.fps_tie_picks(xyz[b].numpy(), npoint)
        ties, zeros = ties + t, zeros + z
    print(f'fps {(n, npoint, distinct)}: {ties} of {B * (npoint - 1)} picks are ties, {zeros} of them at an all-zero maximum')
    assert zeros >= 1                                              # the case holds what it is for
    if distinct == LATTICE:
        assert ties - zeros >= 1                                   # ties at equal non-zero distances too
    for b in range(B):
        ref = po.farthest_point_sample(xyz[b].numpy(), npoint)
        assert torch.equal(idx[b].cpu(), torch.from_numpy(ref)), (b, 'idx')
        assert _bit_equal(new_xyz[b], xyz[b][torch.from_numpy(ref).long()]), (b, 'new_xyz')


@pytest.mark.parametrize('n,npoint,distinct', FPS_CASES)
def test_emulated_fps_matches_the_oracle(n, npoint, distinct):
    _emulated(_fps_case, n, npoint, distinct)


@pytest.mark.gpu
@pytest.mark.parametrize('n,npoint,distinct', FPS_CASES)
def test_gpu_fps_matches_the_oracle(n, npoint, distinct):
    _fps_case('cuda', n, npoint, distinct)


# ------------------------------------------------------------------------------------------------------------------ ball query + grouping
# (n, S, nsample, C, distinct, radius): row widths 3 + C below and above 64 (the flattened and the four-rows-at-a-time walks), nsample divisible by four and not,
# B * S no multiple of the four centroids of a workgroup, a cloud of one partial ballot, nsample at its maximum
GROUP_CASES = [(512, 256, 32, 5, 40, .03), (512, 64, 32, 64, 40, .06), (200, 50, 16, 3, 7, .03), (1000, 16, 64, 61, 60, .12), (130, 7, 5, 2, 130, .03), (512, 4, 32, 256, 5, .24),
               (300, 40, 16, 4, LATTICE, pc.lattice_radius(2)), (200, 30, 32, 70, LATTICE, pc.lattice_radius(3))]
GROUP_B = 2
GROUP_IDS = ['-'.join(str(v) for v in c[:5]) for c in GROUP_CASES]


def _group_inputs(n, S, C, distinct):
    return _clouds(GROUP_B, n, distinct, seed=n + S + C), _r(GROUP_B, n, C, seed=S)


def _group_reference(xyz, new_xyz, feats, nsample, radius):
    """-> (group indices [B, S, nsample], rows [B, S, nsample, 3 + C]) by the oracle: gathers and single fp32 subtractions"""
    idx, rows = [], []
    for b in range(xyz.shape[0]):
        x, c, f = xyz[b].numpy(), new_xyz[b].numpy(), feats[b].numpy()
        g = po.ball_query(radius, nsample, x, c)
        idx.append(g)
        rows.append(np.concatenate([x[g] - c[:, None, :], f[g]], -1).astype(np.float32))
    return torch.from_numpy(np.stack(idx)), torch.from_numpy(np.stack(rows))


def _check_group(dev, what, xyz, new_xyz, feats, nsample, radius):
    B, n, C = feats.shape
    S = new_xyz.shape[1]
    gi, rows = _group_reference(xyz, new_xyz, feats, nsample, radius)
    f = feats.clone().to(dev).requires_grad_(True)
    g = TF.pn2_group(xyz.to(dev), new_xyz.to(dev), f, nsample, radius * radius)
    got_idx = g.grad_fn.saved_tensors[0]
    assert torch.equal(got_idx.cpu().reshape(gi.shape), gi), (what, 'group_idx')
    assert _bit_equal(g.reshape(rows.shape), rows), (what, 'rows')
    dg = _r(*g.shape, seed=7)
    g.backward(dg.to(dev))
    d = dg.reshape(B, S * nsample, 3 + C)[:, :, 3:]
    truth, f32 = (torch.stack([torch.zeros(n, C, dtype=dt).index_add_(0, gi[b].reshape(-1).long(), d[b].to(dt)) for b in range(B)])       # padded slots repeat an index: they accumulate
                  for dt in (torch.float64, torch.float32))
    _held(what, 'dfeats', f.grad, truth, f32)
    return gi


def _group_case(dev, n, S, nsample, C, distinct, radius):
    xyz, feats = _group_inputs(n, S, C, distinct)
    _, new_xyz = TF.pn2_fps(xyz.to(dev), S)
    new_xyz = new_xyz.cpu()
    for b in range(GROUP_B):
        assert _bit_equal(new_xyz[b], xyz[b][torch.from_numpy(po.farthest_point_sample(xyz[b].numpy(), S)).long()])
    short, over, edge = (sum(v) for v in zip(*(pc.ball_fill(radius, nsample, xyz[b].numpy(), new_xyz[b].numpy()) for b in range(GROUP_B))))
    print(f'group {(n, S, nsample, C, distinct)}: {short} balls short of nsample, {over} over, {edge} with a member on the boundary')
    if distinct == LATTICE:
        assert edge >= 1                                           # the `<=` of the ball decides memberships here
    _check_group(dev, f'group {(n, S, nsample, C, distinct)}', xyz, new_xyz, feats, nsample, radius)


def test_group_cases_hold_short_and_overfull_balls():
    """From the oracle alone: across the grouping cases some balls are padded and some overflow; the sa1-shaped case at 40 distinct points has both."""
    tally = {}
    for n, S, nsample, C, distinct, radius in GROUP_CASES:
        xyz, _ = _group_inputs(n, S, C, distinct)
        fill = [pc.ball_fill(radius, nsample, xyz[b].numpy(), xyz[b].numpy()[po.farthest_point_sample(xyz[b].numpy(), S)]) for b in range(GROUP_B)]
        tally[(n, S, nsample, distinct)] = (sum(f[0] for f in fill), sum(f[1] for f in fill))
    print(tally)
    assert sum(v[0] for v in tally.values()) > 0 and sum(v[1] for v in tally.values()) > 0
    assert min(tally[(512, 256, 32, 40)]) > 0


@pytest.mark.parametrize('n,S,nsample,C,distinct,radius', GROUP_CASES, ids=GROUP_IDS)
def test_emulated_group_matches_the_oracle(n, S, nsample, C, distinct, radius):
    _emulated(_group_case, n, S, nsample, C, distinct, radius)


@pytest.mark.gpu
@pytest.mark.parametrize('n,S,nsample,C,distinct,radius', GROUP_CASES, ids=GROUP_IDS)
def test_gpu_group_matches_the_oracle(n, S, nsample, C, distinct, radius):
    _group_case('cuda', n, S, nsample, C, distinct, radius)


# An EMPTY ball — a finite centroid farther than the radius from every point — is filled with point 0.  (nsample, C): the flattened and the four-rows walks.
EMPTY_CASES = [(5, 3), (32, 70)]


def _empty_ball_case(dev, nsample, C):
    xyz, feats = _group_inputs(200, 6, C, 7)
    new_xyz = torch.stack([xyz[b][torch.from_numpy(po.farthest_point_sample(xyz[b].numpy(), 6)).long()] for b in range(GROUP_B)])
    new_xyz[:, 3] = torch.tensor([3.0, -3.0, 3.0])                 # the columns of the cloud have unit norm: every coordinate is within [-1, 1]
    assert float(po.sqdist(new_xyz[0, 3:4].numpy(), xyz[0].numpy()).min()) > 1.0
    gi = _check_group(dev, f'empty ball {(nsample, C)}', xyz, new_xyz, feats, nsample, .03)
    assert (gi[:, 3] == 0).all() and (gi[:, :3] != 0).any()


@pytest.mark.parametrize('nsample,C', EMPTY_CASES)
def test_emulated_group_fills_an_empty_ball_with_point_0(nsample, C):
    _emulated(_empty_ball_case, nsample, C)


@pytest.mark.gpu
@pytest.mark.parametrize('nsample,C', EMPTY_CASES)
def test_gpu_group_fills_an_empty_ball_with_point_0(nsample, C):
    _empty_ball_case('cuda', nsample, C)


# ------------------------------------------------------------------------------------------------------------------ 3-NN interpolation
# (n, s, C1, C2, distinct): s at its minimum (3) and maximum (512), no skip features, row widths below and above 64 (more than one column round per lane), B * n no multiple
# of the four points of a workgroup
INTERP_CASES = [(512, 256, 5, 64, 40), (256, 64, 64, 128, 40), (64, 3, 0, 7, 3), (200, 50, 3, 70, 7), (512, 512, 0, 130, 300), (100, 5, 2, 2, 1), (301, 120, 3, 9, LATTICE)]
INTERP_B = 2


def _interp_case(dev, n, s, C1, C2, distinct):
    what = f'interp {(n, s, C1, C2, distinct)}'
    B = INTERP_B
    xyz1 = _clouds(B, n, distinct, seed=n + s + C2)
    _, xyz2 = TF.pn2_fps(xyz1.to(dev), s)
    xyz2 = xyz2.cpu()
    skip = _r(B, n, C1, seed=1) if C1 else None
    sparse = _r(B, s, C2, seed=2)
    nn, w, tied = [], [], 0
    for b in range(B):
        assert _bit_equal(xyz2[b], xyz1[b][torch.from_numpy(po.farthest_point_sample(xyz1[b].numpy(), s)).long()])
        i, ww = po.three_nn_weights(xyz1[b].numpy(), xyz2[b].numpy())
        nn.append(torch.from_numpy(i).long())
        w.append(torch.from_numpy(ww))
        tied += pc.interp_tied_rows(xyz1[b].numpy(), xyz2[b].numpy())
    print(f'{what}: {tied} of {B * n} rows have their 3rd and 4th neighbour at equal distance')
    assert tied >= 1 or s == 3                                     # (s = 3, the kernel's minimum, has no 4th neighbour)
    sk = skip.clone().to(dev).requires_grad_(True) if C1 else None
    sp = sparse.clone().to(dev).requires_grad_(True)
    out = TF.pn2_interp(xyz1.to(dev), xyz2.to(dev), sk, sp)
    assert tuple(out.shape) == (B * n, C1 + C2)
    dout = _r(B * n, C1 + C2, seed=3)
    out.backward(dout.to(dev))
    ref = {}
    for dt in (torch.float64, torch.float32):
        fwd, dsp = [], []
        for b in range(B):
            p2, wb, d = sparse[b].to(dt), w[b].to(dt), dout.reshape(B, n, -1)[b, :, C1:].to(dt)
            fwd.append((wb[:, 0:1] * p2[nn[b][:, 0]] + wb[:, 1:2] * p2[nn[b][:, 1]]) + wb[:, 2:3] * p2[nn[b][:, 2]])
            acc = torch.zeros(s, C2, dtype=dt)
            for j in range(3):
                acc.index_add_(0, nn[b][:, j], wb[:, j:j + 1] * d)
            dsp.append(acc)
        ref[dt] = (torch.stack(fwd).reshape(B * n, C2), torch.stack(dsp))
    if C1:
        assert _bit_equal(out[:, :C1], skip.reshape(B * n, C1)), (what, 'skip columns')
        want = dout[:, :C1].reshape(B, n, C1)
        _held(what, 'dskip', sk.grad, want.double(), want)
    _held(what, 'interpolated', out[:, C1:], ref[torch.float64][0], ref[torch.float32][0])
    _held(what, 'dsparse', sp.grad, ref[torch.float64][1], ref[torch.float32][1])


@pytest.mark.parametrize('n,s,C1,C2,distinct', INTERP_CASES)
def test_emulated_interp_matches_the_oracle(n, s, C1, C2, distinct):
    _emulated(_interp_case, n, s, C1, C2, distinct)


@pytest.mark.gpu
@pytest.mark.parametrize('n,s,C1,C2,distinct', INTERP_CASES)
def test_gpu_interp_matches_the_oracle(n, s, C1, C2, distinct):
    _interp_case('cuda', n, s, C1, C2, distinct)


# ------------------------------------------------------------------------------------------------------------------ non-finite coordinates: EMULATION ONLY
def test_emulated_non_finite_coordinates_keep_every_index_in_range():
    """A bad radar frame (one NaN and one infinite coordinate) gives unspecified VALUES, but no kernel may form an index outside its cloud: the sampling and grouping
    indices are asserted to be in range, the interpolation and its adjoint (whose indices stay inside the kernel: a dense NaN point finds no neighbour at all, a sparse level
    of three with one infinite point finds two) run to completion on them.  No `gpu` twin: non-finite coordinates are never fed to the device."""
    def case(dev):
        n, S, nsample = 200, 50, 16
        xyz = pc.cloud(2, n, 40, seed=5)
        xyz[0, 17, 1] = float('nan')
        xyz[1, 5, 2] = float('inf')
        idx, new_xyz = TF.pn2_fps(xyz, S)
        assert int(idx.min()) >= 0 and int(idx.max()) < n
        assert not torch.isfinite(new_xyz).all()                   # the bad points are sampled (an untouched running distance stays at its start value): centroids that own no ball
        feats = _r(2, n, 4, seed=1).requires_grad_(True)
        g = TF.pn2_group(xyz, new_xyz, feats, nsample, .03 * .03)
        gi = g.grad_fn.saved_tensors[0]
        assert int(gi.min()) >= 0 and int(gi.max()) < n
        g.backward(torch.ones_like(g))
        assert feats.grad.shape == feats.shape
        for s in (S, 3):
            sparse = _r(2, s, 6, seed=2).requires_grad_(True)
            out = TF.pn2_interp(xyz, new_xyz[:, :s].contiguous(), None, sparse)
            out.backward(torch.ones_like(out))
            assert tuple(out.shape) == (2 * n, 6) and sparse.grad.shape == sparse.shape
    _emulated(case)


# ------------------------------------------------------------------------------------------------------------------ the engine: every level, every size, every launch form
# (variant, N, distinct, dtype): N = 384 -> levels of 192 / 48 / 12 / 3 points (partial sampling lanes, a ball query whose only ballot is partial, interpolation at s = 3);
# N = 1024 -> pn2_fps_level<16> and a full PN2_INTERP_SPL
ENGINE_CASES = [('pn2', 512, 40, 'f32'), ('pn2', 512, 2, 'f32'), ('pn2', 384, None, 'f32'), ('pn2', 384, 25, 'bf16'), ('pn2_msg', 1024, None, 'f32'), ('pn2_msg', 1024, 70, 'f32')]
GPU_ENGINE_CASES = ENGINE_CASES + [('pn2', 512, 40, 'bf16'), ('pn2', 512, 40, 'f16')]
TORCH_DTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
ENGINE_B = 2


def _engine_inputs(N, distinct, resolution, td):
    x, xr, xp = make_inputs(ENGINE_B, 7 + N, resolution=resolution, num_points=N, pc_channels=5, radar_cells=40)
    if distinct is not None:
        xp = pc.resampled(xp, distinct, seed=N + distinct)
    return x, xr, xp.to(td)                                        # (16-bit: the oracle is given the rounded coordinates, as the engine sees them)


def _oracle(sd, kw, x, xr, xp, distinct):
    orc = AchelousOracle(sd, **kw)
    pc_ref = orc.forward(x, xr, xp.float())[3]
    if distinct is not None:                                       # an all-zero maximum goes to index 0: point 0 is sampled again and again
        assert all(int((orc.taps['pc.sa1.fps'][b] == 0).sum()) > 1 for b in range(ENGINE_B))
    return orc, pc_ref


def _compare_taps(names, read, orc, tol, variant):
    seen, worst, worst_tap = 0, 0.0, ''
    for tap in names:
        if not tap.startswith('pc.'):
            continue
        b = torch.as_tensor(orc.taps[tap])
        a = read(tap).cpu().reshape(b.shape)
        if _is_index_tap(tap):
            assert torch.equal(a, b.float()), tap                  # index selection: bit-exact
        else:
            err = _rel_tap(a, b.float())
            worst, worst_tap = max((worst, worst_tap), (err, tap))
            assert err < tol, (tap, err)
        seen += 1
    print(f'{seen} taps compared; worst value tap {worst_tap}: {worst:.1e} (tolerance {tol:.0e})')
    assert seen == (4 * 4 + 4 if variant == 'pn2' else 4 * 5 + 4)


@pytest.mark.parametrize('variant,N,distinct,dtype', ENGINE_CASES)
def test_emulated_engine_matches_the_self_oracle(variant, N, distinct, dtype):
    from emu_util import alloc_outputs, emu_library, make_engine
    kw, td = KWS[variant], TORCH_DTYPE[dtype]
    sd = _state_dict(variant=variant)
    x, xr, xp = _engine_inputs(N, distinct, 64, td)
    orc, pc_ref = _oracle(sd, kw, x, xr, xp, distinct)
    eng = make_engine(emu_library(), kw, ENGINE_B, sd, N, DTYPE_F32 if dtype == 'f32' else DTYPE_BF16)
    outs = alloc_outputs(kw, ENGINE_B, N, td, 'cpu')
    eng.forward(x.to(td), xr.to(td), xp, outs)
    tol = 2e-5 if dtype == 'f32' else 6e-2
    assert _rel_tap(outs[5].float(), pc_ref) < tol
    _compare_taps(eng.tap_names(), eng.read_tap, orc, tol, variant)


def _gpu_module(variant, options=None):
    kw = {**KWS[variant], 'resolution': 96}
    m = achelous_amd.Achelous(**kw).eval()
    m.debug_taps = True
    m.engine_options = dict(options or {})
    sd = condition_state_dict(m.state_dict(), seed=0)
    m.load_state_dict(sd, strict=True)
    return kw, sd, m.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('variant,N,distinct,dtype', GPU_ENGINE_CASES)
def test_gpu_engine_matches_the_self_oracle(variant, N, distinct, dtype):
    td = TORCH_DTYPE[dtype]
    kw, sd, m = _gpu_module(variant)
    x, xr, xp = _engine_inputs(N, distinct, 96, td)
    orc, pc_ref = _oracle({k: v.cpu() for k, v in sd.items()}, kw, x, xr, xp, distinct)
    with torch.no_grad():
        out = m(x.cuda().to(td), xr.cuda().to(td), xp.cuda())[3]
    torch.cuda.synchronize()
    tol = 1e-3 if dtype == 'f32' else 6e-2
    assert out.shape == (ENGINE_B, N, 8) and _rel_tap(out.float(), pc_ref) < tol
    e = m.native_engine(td)
    _compare_taps(e.tap_names(), e.read_tap, orc, tol, variant)


# The launch forms (engine.h: "identical selections", "bit-identical"): all four levels' sampling in one launch or one launch per level, a workgroup or a wave per centroid in
# the grouping, a workgroup or a wave per ball in the shared MLP's maximum.  Every pc.* tap and the output, bit for bit, between the four plans.
PLANS = [{}, {'pn2_fps_all': 0}, {'group_wpc': 0}, {'group_max': 1}]
FORM_CASES = [(512, 40, 'f32'), (512, 40, 'bf16'), (384, None, 'f32'), (384, None, 'bf16')]


def _assert_plans_identical(results):
    out0, taps0 = results[0]
    assert len(taps0) == 20
    for plan, (out, taps) in zip(PLANS[1:], results[1:]):
        assert _bit_equal(out, out0), (plan, 'pc_seg')
        assert taps.keys() == taps0.keys()
        for t in taps0:
            assert _bit_equal(taps[t], taps0[t]), (plan, t)


@pytest.mark.parametrize('N,distinct,dtype', FORM_CASES)
def test_emulated_launch_forms_are_bit_identical(N, distinct, dtype):
    from achelous_amd.engine import NativeEngine
    from emu_util import alloc_outputs, emu_library
    kw, td = KWS['pn2'], TORCH_DTYPE[dtype]
    sd = _state_dict()
    x, xr, xp = _engine_inputs(N, distinct, 64, td)
    results = []
    for plan in PLANS:
        eng = NativeEngine(emu_library(), num_det=kw['num_det'], num_seg=kw['num_seg'], phi=kw['phi'], backbone=kw['backbone'], resolution=kw['resolution'],
                           pc_channels=kw['pc_channels'], pc_classes=kw['pc_classes'], num_points=N, nano_head=kw['nano_head'], spp=kw['spp'],
                           dtype=DTYPE_F32 if dtype == 'f32' else DTYPE_BF16, neck='gdf', pc_seg='pn2')
        eng.set_option('full_taps', 1)
        for k, v in plan.items():
            eng.set_option(k, v)
        eng.load_state_dict(sd)
        eng.plan(ENGINE_B)
        outs = alloc_outputs(kw, ENGINE_B, N, td, 'cpu')
        eng.forward(x.to(td), xr.to(td), xp, outs)
        results.append((outs[5].clone(), {t: eng.read_tap(t).clone() for t in eng.tap_names() if t.startswith('pc.')}))
    _assert_plans_identical(results)


@pytest.mark.gpu
@pytest.mark.parametrize('N,distinct,dtype', FORM_CASES)
def test_gpu_launch_forms_are_bit_identical(N, distinct, dtype):
    td = TORCH_DTYPE[dtype]
    x, xr, xp = (t.cuda().to(td) for t in _engine_inputs(N, distinct, 96, td))
    _, _, m = _gpu_module('pn2')
    results = []
    for plan in PLANS:
        m.reset_engines()
        m.engine_options = dict(plan)
        with torch.no_grad():
            out = m(x, xr, xp)[3]
        torch.cuda.synchronize()
        e = m.native_engine(td)
        results.append((out.clone(), {t: e.read_tap(t).cpu().clone() for t in e.tap_names() if t.startswith('pc.')}))
    _assert_plans_identical(results)
