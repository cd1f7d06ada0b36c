"""RepViT backbone ('rv') on the MI355X: the engine with csrc/k_repvit.h against the rv_* fixtures of the imported reference (tests/golden/gen_rv_golden.py),
batch invariance, the pipelined plan, one ragged serving call, and training mode (train_graph.TrainGraph.repvit) against train_rv_s0.  The per-tensor table the 16-bit test prints is committed as profiles/rv_parity_table.txt."""
import numpy as np
import pytest
import torch

from achelous_amd import Achelous, decode_outputs
from achelous_amd import engine as eng_mod
from achelous_amd.postprocess import nms_device
from achelous_amd.synth import make_inputs
from achelous_amd.synth import condition_state_dict
from repvit_cases import F32_TOL, FIXTURES, OUTPUTS, fixture_case, fixture_errors, h16_bound, train_check

pytestmark = pytest.mark.gpu
MAPS = ('map2', 'map3', 'map4', 'map5')


def _model(name, debug_taps=False):
    g, kw, sd, inputs = fixture_case(name)
    m = Achelous(**kw).eval()
    m.debug_taps = debug_taps
    m.load_state_dict(sd, strict=True)
    return g, kw, m.cuda(), inputs


def _flat(o):
    return (*o[0], o[1], o[2], o[3])


@pytest.mark.parametrize('name', FIXTURES)
def test_forward_fp32_matches_reference_fixtures(name):
    """Every stored tap and output within 1e-3, decoded boxes within 1e-4, NMS kept-index sequences on the fixture's `decoded` bit-exact."""
    g, kw, m, (x, xr, xp) = _model(name, debug_taps=True)
    with torch.no_grad():
        det, se, lane, pc = m(x.cuda(), xr.cuda(), xp.cuda())
    torch.cuda.synchronize()
    assert [tuple(d.shape) for d in det] == [g.shape('det0'), g.shape('det1'), g.shape('det2')] and se.dtype == torch.float32
    e = m.native_engine(torch.float32)
    errs = fixture_errors(g, (*det, se, lane, pc), e.read_tap, e.tap_names())
    print(f'{name}: worst fp32 rel err {max(errs.values()):.2e} ({max(errs, key=errs.get)}) over {len(errs)} tensors; maps', {k: f'{errs[k]:.1e}' for k in MAPS})
    bad = {k: v for k, v in errs.items() if not v < F32_TOL}
    assert not bad, bad
    assert g.rel_err('decoded', decode_outputs(det, [kw['resolution']] * 2)) < 1e-4
    _, val = g.expected('decoded')
    dec = torch.from_numpy(val.reshape(g.shape('decoded')).copy()).cuda()
    for conf, iou in g.meta['nms_settings']:
        rows, idx, cnt = nms_device(dec, kw['num_det'], conf, iou)
        for b in range(g.meta['batch']):
            exp_rows, exp_idx = g.nms(conf, iou, b)
            k = int(cnt[b])
            assert k == len(exp_idx), (conf, iou, b, k, len(exp_idx))
            assert np.array_equal(idx[b, :k].cpu().numpy().astype(np.int64), exp_idx)


@pytest.mark.parametrize('io', ['bf16', 'f16'])
@pytest.mark.parametrize('name', ['rv_s0', 'rv_s2', 'rv_s1_r96'])
def test_forward_16bit_matches_reference_fixtures(name, io):
    """The production 16-bit engine (fp16 storage) behind bf16 or fp16 tensors: each output within max(H16_TOL, 2 x the reference's own drift under bf16 autocast),
    each internal tap within max(2e-2, 3 x that figure) (repvit_cases.h16_bound)."""
    g, kw, m, (x, xr, xp) = _model(name, debug_taps=True)
    dt = torch.bfloat16 if io == 'bf16' else torch.float16
    with torch.no_grad():
        det, se, lane, pc = m(x.cuda().to(dt), xr.cuda().to(dt), xp.cuda().to(dt))
    torch.cuda.synchronize()
    assert se.dtype == dt and det[0].dtype == dt and pc.dtype == dt
    e = m.native_engine(dt)
    assert e.dtype == eng_mod.DTYPE_F16 and m.f16_saturated == 0
    errs = fixture_errors(g, (*det, se, lane, pc), e.read_tap, e.tap_names(), check_sums=False)
    bound = {k: h16_bound(g, k) for k in errs}
    print(f'{name} [{io} in/out, fp16 storage]: rel err per tensor (bound):')
    for k, v in sorted(errs.items(), key=lambda kv: -kv[1] / bound[kv[0]]):
        print(f'    {k:18s} {v:.2e}  ({bound[k]:.2e})')
    bad = {k: (v, bound[k]) for k, v in errs.items() if not v < bound[k]}
    assert not bad, bad


def test_frame_is_bit_identical_whatever_batch_it_sits_in():
    """fp16 engine at 96 x 96 (maps 24 / 12 / 6 / 3: 9 pixels per sample at stride 32): frame i of a B = 5 batch equals its B = 1 run on map2..map5 and the outputs."""
    g, kw, m, _ = _model('rv_s1_r96', debug_taps=True)
    x, xr, xp = (t.cuda().half() for t in make_inputs(5, 41, resolution=96, pc_channels=kw['pc_channels']))
    with torch.no_grad():
        o5 = [t.clone() for t in _flat(m(x, xr, xp))]
        e = m.native_engine(torch.float16)
        m5 = [e.read_tap(t).clone() for t in MAPS]
        for i in range(5):
            o1 = _flat(m(x[i:i + 1], xr[i:i + 1], xp[i:i + 1]))
            torch.cuda.synchronize()
            assert all(torch.equal(a[i:i + 1], b) for a, b in zip(o5, o1)), i
            assert all(torch.equal(a[i:i + 1], e.read_tap(t)) for a, t in zip(m5, MAPS)), i


def test_pipelined_submit_wait_and_single_stream_equal_plain_calls():
    """submit_detect / wait over 4 batches (two in flight) returns, bit for bit, what forward_detect returns; so does the single-stream plan."""
    g, kw, m, _ = _model('rv_s0')
    for dt in (torch.float32, torch.bfloat16):
        batches = []
        for i in range(4):
            x, xr, xp = make_inputs(8, 700 + i, resolution=kw['resolution'], pc_channels=kw['pc_channels'], dense_radar=(i % 2 == 1))
            batches.append((x.cuda().to(dt), xr.cuda().to(dt), xp.cuda().to(dt)))
        with torch.no_grad():
            want = [m.forward_detect(*b, 0.05, 0.5, 100) for b in batches]
            torch.cuda.synchronize()
            for rep in range(2):
                got, prev = [], None
                for b in batches:
                    nxt = m.submit_detect(*b, 0.05, 0.5, 100)
                    if prev is not None:
                        got.append(prev.wait())
                    prev = nxt
                got.append(prev.wait())
                torch.cuda.synchronize()
                for (o1, d1), (o2, d2) in zip(got, want):
                    assert all(torch.equal(a, b_) for a, b_ in zip((*_flat(o1), *d1), (*_flat(o2), *d2))), (dt, rep)
            assert int(want[0][1][2].max()) > 0
            e = m.native_engine(dt)
            e.set_option('streams', 0)
            e.plan(8)
            single = [m.forward_detect(*b, 0.05, 0.5, 100) for b in batches[:2]]
            torch.cuda.synchronize()
            e.set_option('streams', 1)
            e.plan(8)
            for (o1, d1), (o2, d2) in zip(single, want):
                assert all(torch.equal(a, b_) for a, b_ in zip((*_flat(o1), *d1), (*_flat(o2), *d2))), dt


def test_detect_frames_serves_a_repvit_net():
    """One prepost.detect_frames call on two small ragged frames: shapes and dtypes only (the serving path is backbone-agnostic; tests/test_serve.py holds it exactly)."""
    from achelous_amd import data as D, prepost as P
    g, kw, m, _ = _model('rv_s0_r64')
    shapes = [(40, 72), (64, 48)]
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in shapes]
    radar = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda() * 30.0
    pts = torch.randn(2, 512, kw['pc_channels'], generator=torch.Generator().manual_seed(2)).cuda()
    got = P.detect_frames(m, D.pack_arena(frames, 3, 'cuda', 'rv_serve'), radar, pts, 0.05, 0.5, True, 50)
    torch.cuda.synchronize()
    assert tuple(got['boxes'].shape) == (2, 50, 7) and got['boxes'].dtype == torch.float32 and tuple(got['count'].shape) == (2,) and got['count'].dtype == torch.int32
    assert tuple(got['point_class'].shape) == (2, 512) and got['point_class'].dtype == torch.int64
    for b, (H, W) in enumerate(shapes):
        assert tuple(got['semantic'][b].shape) == (H, W) and got['semantic'][b].dtype == torch.uint8
        assert tuple(got['waterline'][b].shape) == (H, W) and tuple(got['overlay'][b].shape) == (H, W, 3) and got['overlay'][b].dtype == torch.uint8


def test_training_step_matches_the_reference():
    """One training step on the HIP training kernels against the reference's float64 step (repvit_cases.train_check: outputs, every gradient, every running statistic —
    the dead tail block's among them — and the list of parameters without gradient)."""
    worst = train_check('cuda')
    print('largest relative errors (ours, torch fp32):', [(f'{e:.1e}', f'{r:.1e}', k) for e, r, k in worst])


def test_train_then_eval_uses_the_updated_weights_and_statistics():
    """Two SGD steps in `.train()`, then `.eval()` runs the inference engine on the NEW weights and running statistics (the folds are rebuilt): equal, bit for bit, to a
    fresh module loaded from the trained state dict, and different from before."""
    g, kw, _, _ = fixture_case('rv_s1_r96')
    m = Achelous(**kw)
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=0))
    m = m.cuda()
    x, xr, xp = (t.cuda() for t in make_inputs(2, 41, resolution=96, num_points=32, pc_channels=kw['pc_channels'], radar_cells=10))
    m.eval()
    with torch.no_grad():
        before = [t.clone() for t in _flat(m(x, xr, xp))]
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    m.train()
    for _ in range(2):
        det, se, lane, pc = m(x, xr, xp)
        loss = sum((o ** 2).mean() for o in (*det, se, lane, pc))
        opt.zero_grad()
        loss.backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        after = _flat(m(x, xr, xp))
        fresh = Achelous(**kw)
        fresh.load_state_dict(m.state_dict())
        ref = _flat(fresh.cuda().eval()(x, xr, xp))
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    assert all(torch.equal(a, b) for a, b in zip(after, ref))
