"""`Achelous.forward` in `.train()` (achelous_amd/train_graph.py: the whole EN-GDF-PN model on native forward / backward kernels)
against one training step of the imported reference (tests/golden/train_en_s0.npz, written by gen_train_golden.py from
/root/reference in this container): the six outputs, the gradient of EVERY parameter and every BatchNorm running statistic.

Truth is the reference evaluated in float64.  The fixture also records, per tensor, how far torch's own float32 evaluation of the
same graph lands from that truth; the float32 HIP kernels are held to a small multiple of that (training-mode BatchNorm over two
frames of 3x3 maps is badly conditioned: torch's fp32 loss itself differs from the fp64 one by 4e-4).  CPU: the kernels under the
emulation library; `-m gpu`: the HIP kernels."""
import json
import os

import numpy as np
import pytest
import torch

from achelous_amd import Achelous, train_ops
from achelous_amd.synth import condition_state_dict, make_inputs

# A bias in front of a training-mode BatchNorm has a TRUE gradient of zero: every float32 evaluation returns rounding noise around it, at the scale of the step's gradients — and on
# the GPU not the same noise twice (the deformable conv's input gradient is summed with atomics in an order that differs from run to run).  Such tensors are held to this fraction of
# the step's largest gradient instead of a relative bound (measured over repeated runs on the MI355X: up to 2.5e-6).
ZERO_GRAD_FLOOR = 5e-6

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, 'golden', 'train_en_s0')


def _step(dev):
    meta = json.load(open(FIX + '.meta.json'))
    fx = np.load(FIX + '.npz')
    m = Achelous(**meta['ctor'])
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=meta['weight_seed']), strict=True)
    m = m.to(dev).train()
    x, xr, xp = make_inputs(meta['batch'], meta['input_seed'], resolution=meta['ctor']['resolution'], num_points=meta['num_points'],
                            pc_channels=meta['ctor']['pc_channels'], radar_cells=meta['radar_cells'])
    det, se, lane, pc = m(x.to(dev), xr.to(dev), xp.to(dev))
    outs = [*det, se, lane, pc]
    g = torch.Generator().manual_seed(meta['cotangent_seed'])
    cot = [torch.randn(o.shape, generator=g, dtype=torch.float64).float().to(dev) for o in outs]
    loss = sum((o * c).sum() for o, c in zip(outs, cot))
    loss.backward()
    return meta, fx, m, outs, float(loss.detach())


def _compare(fx, name, t):
    """-> (relative L2 error over the stored samples, the same for torch's own float32 run (whole tensor), |truth|_inf, max abs error)"""
    idx, val, stat = fx[name + '::idx'], fx[name + '::val'], fx[name + '::stat']
    ours = t.detach().double().cpu().reshape(-1).numpy()[idx]
    err = np.linalg.norm(ours - val) / (np.linalg.norm(val) + 1e-300)
    return err, stat[2] / (stat[0] + 1e-300), stat[1], np.abs(ours - val).max()


def _check(dev):
    meta, fx, m, outs, loss = _step(dev)
    report = []
    assert abs(loss - meta['loss']) <= 5 * abs(meta['loss_torch_f32'] - meta['loss']) + 1e-4 * abs(meta['loss']), (loss, meta['loss'], meta['loss_torch_f32'])
    for k, o in enumerate(outs):
        err, ref, _, _ = _compare(fx, f'out{k}', o)
        report.append((err, ref, f'out{k}'))
        assert err <= max(2e-3, 6 * ref), (f'out{k}', err, ref)
    params = dict(m.named_parameters())
    gscale = max(float(fx[k][1]) for k in fx.files if k.startswith('grad::') and k.endswith('::stat'))
    for k in meta['parameters_without_gradient']:
        assert params[k].grad is None or float(params[k].grad.abs().max()) == 0.0, k
    n = 0
    for k, p in params.items():
        if k in meta['parameters_without_gradient']:
            continue
        assert p.grad is not None, k
        err, ref, inf, amax = _compare(fx, 'grad::' + k, p.grad)
        if amax > ZERO_GRAD_FLOOR * gscale:
            report.append((err, ref, k))
        # a bias in front of a training-mode BatchNorm has a TRUE gradient of zero: both sides return rounding noise around it, so
        # such tensors are held to an absolute floor relative to the largest gradient of the step instead
        assert err <= max(5e-3, 8 * ref) or amax <= ZERO_GRAD_FLOOR * gscale, (k, err, ref, amax, inf, gscale)
        n += 1
    assert n == 527
    for k, v in m.named_buffers():
        if k.endswith(('running_mean', 'running_var')):
            err, ref, _, amax = _compare(fx, 'buf::' + k, v)
            assert err <= max(1e-3, 6 * ref) or amax <= 1e-6, (k, err, ref)
        if k.endswith('num_batches_tracked'):
            assert int(v) == 1, k
    return sorted(report, reverse=True)[:8]


def test_emulated_training_step_matches_the_reference():
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        worst = _check('cpu')
        print('largest relative errors (ours, torch fp32):', [(f'{e:.1e}', f'{r:.1e}', k) for e, r, k in worst])
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
def test_gpu_training_step_matches_the_reference():
    _check('cuda')


def _oracle_training_reference(sd, kw, x, xr, xp, cot, dtype=torch.float64):
    """An independent torch-autograd statement of the training step for ANY configuration: the (reference-pinned) oracle with its
    BatchNorm switched to batch statistics and its parameters as float64 autograd leaves."""
    import torch.nn.functional as F
    from oracle.achelous_oracle import AchelousOracle

    class TrainingOracle(AchelousOracle):
        def __init__(self, sd, **k):
            super().__init__(sd, **k)
            self.sd = {n: (v.detach().to(dtype).requires_grad_(True) if v.is_floating_point() and not n.endswith(('running_mean', 'running_var')) else v.detach())
                       for n, v in sd.items()}

        def bn(self, t, pfx, eps):
            return F.batch_norm(t, None, None, self.P(pfx + '.weight'), self.P(pfx + '.bias'), True, 0.1, eps)

        def conv(self, t, pfx, stride=1, pad=0, groups=1):               # (the positional table is built in float32)
            return super().conv(t.to(dtype), pfx, stride, pad, groups)

    o = TrainingOracle(sd, **kw)
    with torch.enable_grad():
        pc = o.pointnet(xp.to(dtype))
        se, lane, (q5, q4, q3) = o.ghost_dual_fpn(x.to(dtype)) if kw['neck'] == 'gdf' else o.csp_dual_fpn(x.to(dtype))
        r3, r4, r5 = o.rcnet(xr.to(dtype))
        det = o.head((o.fuse(q3, r3, 3), o.fuse(q4, r4, 4), o.fuse(q5, r5, 5)))
        outs = [*det, se, lane, pc]
        loss = sum((a * c.to(dtype)).sum() for a, c in zip(outs, cot))
        loss.backward()
    return [t.detach().double() for t in outs], {n: v.grad.double() for n, v in o.sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}


ORACLE_CASES = [('S2', True, 64, 'en_s2'), ('S0', False, 64, 'en_s0'), ('S2', True, 64, 'mv_s2'), ('S0', True, 64, 'en_s0_cdf'), ('S0', True, 320, 'en_s0')]
# The 320 px case is one whole step at the size training runs at, where api_train.cpp dispatches the sliced reductions, split-K and the four-per-thread kernels.  Batch 4, not 2:
# PointNet's STN normalises its fc layers over the batch, and at 2 samples torch's own float32 is 50 % off the float64 truth.  At this size the step is well enough
# conditioned to be held to the yardstick alone (`strict`): outputs and gradients within 6 x torch-float32's own error, no 6e-2 floor.  Measured under the emulation:
# outputs 6e-6 to 2e-5 (torch float32: 7e-6 to 1e-3), median gradient error 4e-3 (1.5e-2), worst ratio to the yardstick over the 527 gradients 2.6.
ORACLE_SETTINGS = {320: dict(batch=4, points=512, radar_cells=256, strict=True)}


def _check_against_oracle_autograd(dev, phi, spp, res, fixture, batch=2, points=32, radar_cells=12, strict=False):
    from golden_util import Golden, ctor_kwargs
    kw = dict(ctor_kwargs(Golden(fixture).meta), resolution=res, spp=spp)
    m = Achelous(**kw)
    sd = condition_state_dict(m.state_dict(), seed=0)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    x, xr, xp = make_inputs(batch, 13, resolution=res, num_points=points, pc_channels=kw['pc_channels'], radar_cells=radar_cells)
    det, se, lane, pc = m(x.to(dev), xr.to(dev), xp.to(dev))
    outs = [*det, se, lane, pc]
    g = torch.Generator().manual_seed(3)
    cot = [torch.randn(o.shape, generator=g) for o in outs]
    sum((a * c.to(dev)).sum() for a, c in zip(outs, cot)).backward()
    okw = {k: kw[k] for k in ('num_det', 'num_seg', 'phi', 'backbone', 'neck', 'pc_seg', 'pc_channels', 'pc_classes', 'nano_head', 'spp', 'resolution')}
    ref_outs, ref_grads = _oracle_training_reference(sd, okw, x, xr, xp, cot)
    f32_outs, f32_grads = _oracle_training_reference(sd, okw, x, xr, xp, cot, torch.float32)        # torch's own float32 evaluation: the yardstick
    for k, (a, b, c) in enumerate(zip(outs, ref_outs, f32_outs)):
        err, yard = ((a.detach().cpu().double() - b).norm() / b.norm()).item(), ((c - b).norm() / b.norm()).item()
        assert err < 5e-3, (f'output {k}', err)
        if strict:
            assert err <= 6 * yard, (f'output {k}', err, yard)
    gscale = max(float(v.abs().max()) for v in ref_grads.values())
    checked, worst = 0, (0.0, None)
    for k, p in m.named_parameters():
        if k not in ref_grads:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        ref, got = ref_grads[k], p.grad.detach().cpu().double()
        err = float((got - ref).norm() / (ref.norm() + 1e-300))
        yard = float((f32_grads[k] - ref).norm() / (ref.norm() + 1e-300))
        at_floor = float((got - ref).abs().max()) <= ZERO_GRAD_FLOOR * gscale
        if strict:
            assert err <= 6 * yard or at_floor, (k, err, yard)
            if not at_floor and err / (yard + 1e-300) > worst[0]:
                worst = (err / (yard + 1e-300), k)
        else:
            # a wiring check (a wrong graph is off by O(1)): BatchNorm over 2 frames of 2x2 maps and PointNet's max over 32 points make a
            # float32 step deviate from the float64 truth by several per cent on some tensors — torch's own float32 does the same
            assert err < max(6e-2, 6 * yard) or at_floor, (k, err, yard)
        checked += 1
    assert checked > 500
    if strict:
        print(f'{checked} gradients; the worst ratio to the yardstick: {worst[0]:.2f} ({worst[1]})')


@pytest.mark.parametrize('phi,spp,res,fixture', ORACLE_CASES)
def test_emulated_training_graph_matches_autograd_on_the_oracle(phi, spp, res, fixture):
    """Configurations the imported-reference fixture does not cover — EdgeNeXt-S2 (8 XCA heads, 3/3/9/3 blocks), the SPPF neck, the
    MobileViT-S2 backbone and the CSP-Dual-FPN neck — against torch autograd (float64) through the oracle in training mode: outputs and
    every parameter gradient."""
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        _check_against_oracle_autograd('cpu', phi, spp, res, fixture, **ORACLE_SETTINGS.get(res, {}))
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
@pytest.mark.parametrize('phi,spp,res,fixture', ORACLE_CASES)
def test_gpu_training_graph_matches_autograd_on_the_oracle(phi, spp, res, fixture):
    _check_against_oracle_autograd('cuda', phi, spp, res, fixture, **ORACLE_SETTINGS.get(res, {}))


@pytest.mark.gpu
def test_gpu_train_then_eval_uses_the_updated_weights_and_statistics():
    """utils/utils_fit.py alternates training steps and evaluation: after `.train()` steps (parameters changed by the optimizer, BatchNorm
    running statistics by the forward) `.eval()` must run the inference engine on the NEW weights — equal to a fresh module loaded from the
    trained state dict."""
    from golden_util import Golden, ctor_kwargs
    g = Golden('en_s0')
    kw = dict(ctor_kwargs(g.meta), resolution=96)
    m = Achelous(**kw)
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=0))
    m = m.cuda()
    x, xr, xp = (t.cuda() for t in make_inputs(2, 41, resolution=96, num_points=32, pc_channels=kw['pc_channels'], radar_cells=10))
    m.eval()
    with torch.no_grad():
        before = [t.clone() for t in (*m(x, xr, xp)[0], m(x, xr, xp)[1])]
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
        after = m(x, xr, xp)
        fresh = Achelous(**kw)
        fresh.load_state_dict(m.state_dict())
        ref = fresh.cuda().eval()(x, xr, xp)
    assert any(not torch.equal(a, b) for a, b in zip((*after[0], after[1]), before))            # the step changed something
    for a, b in zip((*after[0], after[1], after[2], after[3]), (*ref[0], ref[1], ref[2], ref[3])):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_gpu_training_step_under_the_reference_amp_loop():
    """The reference trains under `torch.cuda.amp.autocast()` + GradScaler by default (utils/utils_fit.py:120-166, train.py:37 --fp16 True): the
    forward is called with fp32 tensors inside the autocast region and the scaled loss is back-propagated.  The native training graph keeps its
    own fp32 kernels inside the region (autocast re-types torch ops, not ours), so that loop runs UNCHANGED and its gradients equal the plain
    loop's — a superset of the precision the reference's AMP mode asks for."""
    from golden_util import Golden, ctor_kwargs
    g = Golden('en_s0')
    kw = dict(ctor_kwargs(g.meta), resolution=96)
    x, xr, xp = (t.cuda() for t in make_inputs(2, 43, resolution=96, num_points=32, pc_channels=kw['pc_channels'], radar_cells=10))
    grads = []
    for amp in (False, True):
        m = Achelous(**kw)
        m.load_state_dict(condition_state_dict(m.state_dict(), seed=0))
        m = m.cuda().train()
        scaler = torch.amp.GradScaler('cuda', enabled=amp, init_scale=1024.0)
        with torch.autocast('cuda', dtype=torch.float16, enabled=amp):
            det, se, lane, pc = m(x, xr, xp)
            assert se.dtype == torch.float32
            loss = sum((o.float() ** 2).mean() for o in (*det, se, lane, pc))
        scaler.scale(loss).backward()
        inv = 1.0 / float(scaler.get_scale()) if amp else 1.0
        grads.append({n: p.grad.detach().double() * inv for n, p in m.named_parameters() if p.grad is not None})
    assert len(grads[0]) > 400 and grads[0].keys() == grads[1].keys()
    gmax = max(float(v.abs().max()) for v in grads[0].values())
    for n in grads[0]:
        a, b = grads[0][n], grads[1][n]
        assert torch.isfinite(b).all(), n
        # (a bias in front of a training-mode BatchNorm has a TRUE gradient of zero: both loops return rounding noise around it, at the scale of the step's gradients — and not the
        #  same noise twice: the deformable conv's input gradient is summed with atomics, in an order that differs from run to run.  Measured over repeated runs: up to 2.5e-6 of the
        #  step's largest gradient on `rc_blocks.0.weight_conv1.bias`; the floor is 5e-6)
        assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max()) + ZERO_GRAD_FLOOR * gmax, n


def _bf16_step_errors(batch=8, resolution=160, points=128):
    """One training step of EN-GDF-PN-S0 with fp32 and with bf16 GEMM operands (`Achelous.train_precision`) on the GPU, against the float64 truth (the oracle in
    training mode through torch autograd, CPU) — and, as the yardstick for a 16-bit step, torch's own `autocast(bfloat16)` evaluation of the same float32 graph.
    -> {step: {'outputs': [relative L2 error per output], 'grads': {parameter: relative L2 error}}}"""
    from golden_util import Golden, ctor_kwargs
    kw = dict(ctor_kwargs(Golden('en_s0').meta), resolution=resolution)
    x, xr, xp = make_inputs(batch, 13, resolution=resolution, num_points=points, pc_channels=kw['pc_channels'], radar_cells=40)
    sd, cot, res = None, None, {}
    for prec in ('fp32', 'bf16'):
        m = Achelous(**kw)
        if sd is None:
            sd = condition_state_dict(m.state_dict(), seed=0)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().train()
        m.train_precision = prec
        det, se, lane, pc = m(x.cuda(), xr.cuda(), xp.cuda())
        outs = [*det, se, lane, pc]
        if cot is None:
            g = torch.Generator().manual_seed(3)
            cot = [torch.randn(o.shape, generator=g) / o.numel() ** 0.5 for o in outs]
        sum((o * c.cuda()).sum() for o, c in zip(outs, cot)).backward()
        res[prec] = ([o.detach().cpu().double() for o in outs], {k: p.grad.detach().cpu().double() for k, p in m.named_parameters() if p.grad is not None})
        assert train_ops.set_gemm_precision(x.cuda(), 0) == (1 if prec == 'bf16' else 0)          # the forward set the library's switch; leave it at fp32
    okw = {k: kw[k] for k in ('num_det', 'num_seg', 'phi', 'backbone', 'neck', 'pc_seg', 'pc_channels', 'pc_classes', 'nano_head', 'spp', 'resolution')}
    truth = _oracle_training_reference(sd, okw, x, xr, xp, cot)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        res['torch autocast(bf16)'] = _oracle_training_reference(sd, okw, x, xr, xp, cot, torch.float32)
    rel = lambda got, ref: float((got.double() - ref).norm() / (ref.norm() + 1e-300))
    gscale = max(float(v.abs().max()) for v in truth[1].values())
    return {name: {'outputs': [rel(o, t) for o, t in zip(outs, truth[0])],
                   'grads': {k: rel(grads[k], truth[1][k]) for k in truth[1] if k in grads and float(truth[1][k].abs().max()) > 1e-5 * gscale}}
            for name, (outs, grads) in res.items()}


@pytest.mark.gpu
def test_gpu_bf16_operand_training_step_is_no_worse_than_torch_autocast():
    """`train_precision = 'bf16'` (k_train.h: GEMM operands rounded to bf16 while staged, everything else fp32).  A 16-bit step cannot be held to the fp32 bounds
    above — BatchNorm on batch statistics amplifies the operands' 2^-8 roundings, in torch's own autocast(bfloat16) as much as here — so it is held to (a) absolute
    bounds on the outputs and (b) torch's autocast evaluation of the same graph as the yardstick, tensor by tensor.  Measured (profiles/r05_train_bf16_error.txt):
    outputs 1.3 - 4.1e-2 (autocast 3.9 - 6.1e-2, fp32 1e-5); median gradient error 0.39 (autocast 0.55, fp32 2.7e-3)."""
    e = _bf16_step_errors()
    ours, yard, f32 = e['bf16'], e['torch autocast(bf16)'], e['fp32']
    assert max(f32['outputs']) < 1e-3 and float(np.median(list(f32['grads'].values()))) < 1e-2          # the fp32 step of the same harness: the harness is sound
    assert max(ours['outputs'][:3]) < 3e-2 and max(ours['outputs'][3:]) < 8e-2, ours['outputs']
    for a, b in zip(ours['outputs'], yard['outputs']):
        assert a <= 1.25 * b + 5e-3, (ours['outputs'], yard['outputs'])
    go, gy = np.array([ours['grads'][k] for k in ours['grads']]), np.array([yard['grads'][k] for k in ours['grads']])
    assert len(go) > 450
    assert np.median(go) <= np.median(gy) and np.percentile(go, 90) <= np.percentile(gy, 90), (np.median(go), np.median(gy))
    assert (go <= 2.0 * gy + 5e-2).mean() >= 0.97, float((go <= 2.0 * gy + 5e-2).mean())                   # tensor by tensor (both are noisy: 97 % of the tensors)


@pytest.mark.gpu
def test_gpu_graphed_training_step_equals_the_eager_step():
    """`train_graph.GraphedTrainStep` (round 6): forward + loss + backward + SGD step captured once into a HIP graph and replayed.  Three replayed steps on three different batches
    against three eager steps of a twin model from the same state: the losses and every parameter / BatchNorm statistic agree to the run-to-run noise of the eager step itself
    (the deformable conv's input gradient is summed with atomics), and building the step leaves the model and the optimizer exactly as they were."""
    from achelous_amd.train_graph import GraphedTrainStep
    kw = dict(num_det=7, num_seg=9, phi='S0', resolution=96, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
    sd = condition_state_dict(Achelous(**kw).state_dict(), seed=0)
    batches = [tuple(t.cuda() for t in make_inputs(2, 30 + i, resolution=96, num_points=64, pc_channels=5, radar_cells=12)) for i in range(3)]

    def make():
        m = Achelous(**kw)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().train()
        return m, torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)

    def loss_fn(outs, tgt):
        det, se, lane, pc = outs
        return sum((o ** 2).mean() for o in (*det, se, lane)) + ((pc - tgt) ** 2).mean()
    tgt = [torch.randn(2, 64, 8, generator=torch.Generator().manual_seed(9 + i)).cuda() for i in range(3)]
    m1, o1 = make()
    eager = []
    for (x, xr, xp), t in zip(batches, tgt):
        o1.zero_grad(set_to_none=True)
        loss = loss_fn(m1(x, xr, xp), t)
        loss.backward()
        o1.step()
        eager.append(float(loss.detach()))
    m2, o2 = make()
    before = {k: v.clone() for k, v in m2.state_dict().items()}
    step = GraphedTrainStep(m2, o2, loss_fn, batches[0], (tgt[0],))
    for k, v in m2.state_dict().items():
        assert torch.equal(v, before[k]), k                               # the warm-up steps were undone
    graphed = [float(step(*b, t)) for b, t in zip(batches, tgt)]
    torch.cuda.synchronize()
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 1e-4 * abs(a) + 1e-7, (eager, graphed)
    s1, s2 = m1.state_dict(), m2.state_dict()
    for k in s1:
        if s1[k].is_floating_point():
            d = float((s1[k].double() - s2[k].double()).abs().max())
            assert d <= 1e-4 * float(s1[k].double().abs().max()) + 1e-6, (k, d)
        else:
            assert torch.equal(s1[k], s2[k]), k                           # num_batches_tracked: three steps each
    with pytest.raises(ValueError):
        step(batches[0][0][:1], batches[0][1][:1], batches[0][2][:1], tgt[0][:1])
