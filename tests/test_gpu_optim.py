"""achelous_amd.optim.FusedOptimizer in the training loop on the MI355X: eager steps with a real backward, then `eval()` on the model and on `opt.ema_model`; and a whole
step captured by train_graph.GraphedTrainStep — the learning rate read on replay, the warm-up undone for momentum, EMA and counters, graph against eager.
EN-GDF-PN-S0 at resolution 64, batch 2.  (The arithmetic itself is held to the reference in tests/test_optim.py, on both devices.)"""
import pytest
import torch

from achelous_amd import Achelous
from achelous_amd.optim import H_LR, H_UPDATES, FusedOptimizer
from achelous_amd.synth import condition_state_dict, make_inputs

pytestmark = pytest.mark.gpu
KW = dict(num_det=7, num_seg=9, phi='S0', resolution=64, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
LR = 1e-3


def _make(sd):
    m = Achelous(**KW)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    return m, FusedOptimizer(m, 'sgd', lr=LR, momentum=0.9, weight_decay=5e-4, ema_updates=3000)


def _batches(n):
    return [tuple(t.cuda() for t in make_inputs(2, 30 + i, resolution=64, num_points=64, pc_channels=5, radar_cells=12)) for i in range(n)]


def _loss_fn(outs, tgt):
    det, se, lane, pc = outs
    return sum((o ** 2).mean() for o in (*det, se, lane)) + ((pc - tgt) ** 2).mean()


def _flat(outs):
    return (*outs[0], outs[1], outs[2], outs[3])


def _serves_its_own_state(module, x, xr, xp, before):
    """module.eval()(x) equals a fresh module loaded from module.state_dict(), bit for bit, and differs from `before`"""
    module.eval()
    with torch.no_grad():
        after = _flat(module(x, xr, xp))
        fresh = Achelous(**KW)
        fresh.load_state_dict(module.state_dict())
        ref = _flat(fresh.cuda().eval()(x, xr, xp))
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    for a, b in zip(after, ref):
        assert torch.equal(a, b)


def test_train_then_eval_serves_the_updated_weights_and_the_ema():
    sd = condition_state_dict(Achelous(**KW).state_dict(), seed=0)
    m, opt = _make(sd)
    (x, xr, xp), = _batches(1)
    tgt = torch.randn(2, 64, 8, generator=torch.Generator().manual_seed(9)).cuda()
    m.eval()
    with torch.no_grad():
        before = [t.clone() for t in _flat(m(x, xr, xp))]
        before_ema = [t.clone() for t in _flat(opt.ema_model(x, xr, xp))]
    m.train()
    for _ in range(2):
        loss = _loss_fn(m(x, xr, xp), tgt)
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert float(opt.hyper[H_UPDATES]) == 3002.0
    _serves_its_own_state(m, x, xr, xp, before)
    _serves_its_own_state(opt.ema_model, x, xr, xp, before_ema)


class _Tiny(torch.nn.Module):
    """three inputs, as GraphedTrainStep calls its model; torch ops only"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.weight = torch.nn.Parameter(torch.randn(300, 7, generator=g))
        self.bias = torch.nn.Parameter(torch.randn(300, generator=g))
        self.register_buffer('seen', torch.zeros(7))

    def forward(self, x, xr, xp):
        with torch.no_grad():
            self.seen.add_(x.mean(0))
        return x @ self.weight.t() + self.bias + xr.sum() + xp.sum()


def test_graphed_adam_step_restores_counts_and_moments():
    """the per-parameter step counts `t`, both moments, the EMA and `hyper` are what they were after the capture's warm-up steps; a replay then counts one step"""
    from achelous_amd.train_graph import GraphedTrainStep
    m = _Tiny().cuda().train()
    opt = FusedOptimizer(m, 'adam', lr=1e-2, groups=[{'params': [m.weight], 'weight_decay': 5e-4}, {'params': [m.bias], 'weight_decay': 0.0}], ema_updates=10)
    x, xr, xp = torch.randn(4, 7).cuda(), torch.randn(3).cuda(), torch.randn(2).cuda()
    for s in range(2):                                                       # two steps on drawn gradients first (no autograd graph): the restored state is not the zero state
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=torch.Generator().manual_seed(s)).cuda()
        opt.step()
    opt.zero_grad()
    before = [t.clone() for t in (*m.state_dict().values(), *opt.graph_state())]
    assert set(opt.t.tolist()) == {2} and any(t is opt.t for t in opt.graph_state())
    step = GraphedTrainStep(m, opt, lambda out: out.square().mean(), (x, xr, xp))
    for a, b in zip(before, (*m.state_dict().values(), *opt.graph_state())):
        assert torch.equal(a, b)
    step(x, xr, xp)
    torch.cuda.synchronize()
    assert set(opt.t.tolist()) == {3} and float(opt.hyper[H_UPDATES]) == 13.0 and not torch.equal(m.weight.detach(), before[0])


def test_graphed_step_reads_the_learning_rate_and_equals_the_eager_step():
    from achelous_amd.train_graph import GraphedTrainStep
    sd = condition_state_dict(Achelous(**KW).state_dict(), seed=0)
    batches = _batches(3)
    tgt = [torch.randn(2, 64, 8, generator=torch.Generator().manual_seed(9 + i)).cuda() for i in range(3)]
    m1, o1 = _make(sd)
    for (x, xr, xp), t in zip(batches, tgt):                                 # the eager twin: three steps from the same start
        o1.zero_grad(set_to_none=True)
        loss = _loss_fn(m1(x, xr, xp), t)
        loss.backward()
        o1.step()
    del loss
    m2, o2 = _make(sd)
    snap = lambda: {**{'model.' + k: v.clone() for k, v in m2.state_dict().items()},          # noqa: E731
                    **{k: t.clone() for k, t in (('m1', o2.m1), ('ema', o2.ema_arena), ('hyper', o2.hyper), ('flags', o2.flags))}}
    before = snap()
    m2.eval()
    with torch.no_grad():
        served_before = [t.clone() for t in _flat(m2(*batches[0]))]
        served_before_ema = [t.clone() for t in _flat(o2.ema_model(*batches[0]))]
    m2.train()
    step = GraphedTrainStep(m2, o2, _loss_fn, batches[0], (tgt[0],))
    # 8a: building the step leaves everything as it was (hyper holds lr, updates and d; sgd has no t)
    now = snap()
    for k in before:
        if k != 'flags':
            assert torch.equal(before[k], now[k]), k
    assert len(o2.state) == 0 and o2.t is None
    optimised = [p for g in o2.param_groups for p in g['params']]
    # 8b: learning rate 0 -> a replay moves no optimised parameter, the EMA still ticks and moves (the BatchNorm statistics it averages moved)
    params0, ema0 = [p.detach().clone() for p in optimised], o2.ema_arena.clone()
    o2.set_lr(0.0)
    step(*batches[0], tgt[0])
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), q) for p, q in zip(optimised, params0))
    assert float(o2.hyper[H_UPDATES]) == 3001.0 and float(o2.hyper[H_LR]) == 0.0 and not torch.equal(o2.ema_arena, ema0)
    # 8c: the learning rate back -> parameters change, no new capture
    o2.set_lr(LR)
    step(*batches[0], tgt[0])
    torch.cuda.synchronize()
    assert sum(not torch.equal(p.detach(), q) for p, q in zip(optimised, params0)) > len(optimised) // 2
    # 8d: three replays against three eager steps from the same start (state restored in place: an in-place load keeps the aliasing)
    with torch.no_grad():
        m2.load_state_dict({k[6:]: v for k, v in before.items() if k.startswith('model.')})
        for t, k in ((o2.m1, 'm1'), (o2.ema_arena, 'ema'), (o2.hyper, 'hyper')):
            t.copy_(before[k])
    for b, t in zip(batches, tgt):
        step(*b, t)
    torch.cuda.synchronize()
    assert torch.equal(o1.hyper, o2.hyper)
    pairs = list(zip(m1.state_dict().items(), m2.state_dict().values())) + list(zip(o1.ema_model.state_dict().items(), o2.ema_model.state_dict().values()))
    for (k, a), b in pairs:
        if a.is_floating_point():                                            # tests/test_train_graph.py's graph-against-eager bound (the deformable conv's backward sums with atomics)
            d = float((a.double() - b.double()).abs().max())
            assert d <= 1e-4 * float(a.double().abs().max()) + 1e-6, (k, d)
    assert all(torch.equal(a, b) for (k, a), b in pairs[:len(m1.state_dict())] if not a.is_floating_point())         # num_batches_tracked
    # 8e: eval() after the replays serves the new weights
    _serves_its_own_state(m2, *batches[0], served_before)
    _serves_its_own_state(o2.ema_model, *batches[0], served_before_ema)
