"""What the optimizer step and the weight EMA cost in a training step of EN-GDF-PN-S0 (320 x 320), three contenders:
  (a) torch.optim.SGD (Nesterov, the reference's three groups) + the reference's per-tensor EMA loop (loss/detection_loss.py:449-459: two small kernels per float entry)
  (b) the same optimizer + the EMA as torch._foreach_mul_ / _foreach_add_ over all float entries — the best torch offers
  (c) achelous_amd.optim.FusedOptimizer (two launches)
Per batch: the whole step eager and under train_graph.GraphedTrainStep, and the optimizer-and-EMA part alone (gradients in place, host-issued), ms, median of fenced
repeats (device events around synchronised work, the contenders alternated).  Then the step kernel alone: time per launch and bytes per second against the HBM peak.
The loss is the sum of squares of the outputs (tests/test_train_graph.py's): the step's forward and backward do not depend on the contender.
usage: python profiles/scripts/optim_timing.py [--batches 8 32] [--rounds 3] [--contenders abc] [--out profiles/optim_timing.txt]
       python profiles/scripts/optim_timing.py --kernels-only a|b|c --iters 20        (the optimizer part alone, for a launch count under rocprofv3 --kernel-trace --stats)"""
import argparse
import math
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO]
from achelous_amd import Achelous, _native as N                                        # noqa: E402
from achelous_amd.optim import CHUNK, KINDS, FusedOptimizer, reference_param_groups      # noqa: E402
from achelous_amd.synth import condition_state_dict, make_inputs                       # noqa: E402
from achelous_amd.train_graph import GraphedTrainStep                                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batches', type=int, nargs='*', default=[8, 32])
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--contenders', default='abc')            # e.g. 'c': one contender alone in the process
ap.add_argument('--resolution', type=int, default=320)
ap.add_argument('--kernels-only', default='')
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--out', default='')
a = ap.parse_args()
R, LR, HBM_PEAK = a.resolution, 1e-4, 8.0e12
KW = dict(num_det=7, num_seg=9, phi='S0', resolution=R, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


class TorchSgdEma:
    """contenders (a) and (b): torch.optim.SGD over the reference's groups, then ModelEMA.update restated — per tensor, or with torch's multi-tensor ops; `state`,
    `param_groups` and `zero_grad` are the optimizer's, so GraphedTrainStep treats it as one"""

    def __init__(self, model, foreach):
        named = dict(model.named_parameters())
        pg0, pg1, pg2, _ = reference_param_groups(model)
        self.opt = torch.optim.SGD([named[k] for k in pg0], LR, momentum=0.937, nesterov=True)
        self.opt.add_param_group({'params': [named[k] for k in pg1], 'weight_decay': 5e-4})
        self.opt.add_param_group({'params': [named[k] for k in pg2]})
        self.state, self.param_groups, self.zero_grad = self.opt.state, self.opt.param_groups, self.opt.zero_grad
        self.foreach, self.updates = foreach, 3000
        self.src = [v for v in model.state_dict().values() if v.is_floating_point()]
        self.ema = [v.detach().clone() for v in self.src]

    @torch.no_grad()
    def step(self):
        self.opt.step()
        self.updates += 1
        d = 0.9999 * (1 - math.exp(-self.updates / 2000))
        if self.foreach:
            torch._foreach_mul_(self.ema, d)
            torch._foreach_add_(self.ema, self.src, alpha=1 - d)
        else:
            for v, x in zip(self.ema, self.src):
                v *= d
                v += (1 - d) * x


def make(which, batch):
    m = Achelous(**KW)
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=0))
    m = m.cuda().train()
    opt = FusedOptimizer(m, 'sgd', lr=LR, ema_updates=3000) if which == 'c' else TorchSgdEma(m, foreach=which == 'b')
    return m, opt, tuple(t.cuda() for t in make_inputs(batch, 3, resolution=R, pc_channels=5))


def loss_fn(outs):
    det, se, lane, pc = outs
    return sum((o ** 2).mean() for o in (*det, se, lane, pc))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


NAMES = {'a': '(a) torch SGD + per-tensor EMA loop ', 'b': '(b) torch SGD + _foreach_ EMA       ', 'c': '(c) FusedOptimizer                  '}

if a.kernels_only:
    m, opt, (x, xr, xp) = make(a.kernels_only, 2)
    loss_fn(m(x, xr, xp)).backward()
    torch.cuda.synchronize()
    for _ in range(a.iters):
        opt.step()
    torch.cuda.synchronize()
    print(f'{a.kernels_only}: {a.iters} optimizer-and-EMA parts issued')
    sys.exit(0)

say(f'optimizer step + weight EMA in a training step of EN-GDF-PN-S0 at {R} x {R}, fp32; ms, median of {a.rounds} fenced rounds (min .. max); contenders alternated')
for batch in a.batches:
    say(f'batch {batch}')
    legs = {}
    for which in a.contenders:
        m, opt, (x, xr, xp) = make(which, batch)

        def step(m=m, opt=opt, x=x, xr=xr, xp=xp):
            opt.zero_grad(set_to_none=True)
            loss_fn(m(x, xr, xp)).backward()
            opt.step()
        for _ in range(3):
            step()
        legs[which] = dict(m=m, opt=opt, step=step, eager=[], part=[], graph=[])
    iters = max(3, int(600.0 / a.rounds / timed(legs[a.contenders[-1]]['step'], 2)) + 1)
    for _ in range(a.rounds):
        for which in a.contenders:
            legs[which]['eager'].append(timed(legs[which]['step'], iters))
    for which in a.contenders:                                           # the step's kernels are not all data-independent: a model that went non-finite runs FASTER
        with torch.no_grad():
            bad = sum(int((~torch.isfinite(p)).sum()) for p in legs[which]['m'].parameters())
        if bad:
            say(f'  {NAMES[which]} {bad} non-finite parameter elements after the eager rounds: its eager times are void')
    # the part alone LAST, behind every eager round: torch's multi-tensor SGD adds the momentum term into .grad in place (Nesterov), so repeating step() on the gradients of
    # one backward compounds them and the weights overflow within 20 repeats — harmless for the time of elementwise kernels, fatal for any step timed afterwards
    for _ in range(a.rounds):
        for which in a.contenders:
            legs[which]['part'].append(timed(legs[which]['opt'].step, 20))
    for leg in legs.values():                                            # the graphed legs run on fresh models: a capture wants no eager autograd history
        leg['m'] = leg['opt'] = leg['step'] = None
    torch.cuda.empty_cache()
    for which in a.contenders:
        m, opt, (x, xr, xp) = make(which, batch)
        g = GraphedTrainStep(m, opt, loss_fn, (x, xr, xp))
        g(x, xr, xp)
        legs[which]['graph'] = [timed(lambda: g(x, xr, xp), iters) for _ in range(a.rounds)]
        del g
        if which == 'c':
            fused = opt
    for which in a.contenders:
        leg = legs[which]
        e, p, gr = med(leg['eager']), med(leg['part']), med(leg['graph'])
        say(f'  {NAMES[which]} eager step {e[0]:7.2f} ({e[1]:.2f} .. {e[2]:.2f})   optimizer + EMA alone {p[0]:7.3f} ({p[1]:.3f} .. {p[2]:.3f})   graphed step {gr[0]:7.2f} ({gr[1]:.2f} .. {gr[2]:.2f})')
    if batch == a.batches[-1] and 'c' in a.contenders:
        opt = fused
        L, s = opt._lib.lib, N.stream(opt.state_arena)

        def kernel():
            L.ach_optim_step(N.ptr(opt.state_arena), N.ptr(opt.ema_arena), N.ptr(opt.grad_arena), N.ptr(opt.m1), N.ptr(opt.m2), N.ptr(opt.flags), N.ptr(opt.t), N.ptr(opt.hyper),
                             opt.chunks, opt.param_chunks, KINDS['sgd'], 1, opt.momentum, 0.9, 0.999, 1e-8, s)
        timed(kernel, 50)
        k = med([timed(kernel, 500) for _ in range(a.rounds)])
        # per element: state read + write, gradient read, momentum read + write, EMA read + write = 28 bytes over the parameter part; state read, EMA read + write = 12 over the buffers
        nbytes = 28 * opt.param_chunks * CHUNK + 12 * (opt.chunks - opt.param_chunks) * CHUNK
        say(f'ach_optim_step alone (SGD + Nesterov + EMA, {opt.chunks} chunks = {opt.chunks * CHUNK} elements, {nbytes / 1e6:.1f} MB of traffic), 500 back-to-back launches: '
            f'{1e3 * k[0]:.1f} us ({1e3 * k[1]:.1f} .. {1e3 * k[2]:.1f}) = {nbytes / (k[0] * 1e-3) / 1e12:.2f} TB/s, {100 * nbytes / (k[0] * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak '
            f'(the arenas, {4 * 5 * opt.chunks * CHUNK / 1e6:.0f} MB in all, fit the 256 MB last-level cache: back-to-back launches re-read them from there)')
    del legs
    torch.cuda.empty_cache()
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
