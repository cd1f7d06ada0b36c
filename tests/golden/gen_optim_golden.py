#!/usr/bin/env python3
"""Generate tests/golden/optim_traj.npz / optim_traj.meta.json by IMPORTING the reference (read-only): its model, `ModelEMA`, `get_lr_scheduler` and
`set_optimizer_lr`, with the group construction of train.py:499-518 restated on the imported model.

Recorded:
  * group membership — the parameter names of pg0 / pg1 / pg2 / ungrouped for EN-S0 gdf, EN-S0 cdf, MV-S0 and RV-S0 (tests/optim_cases.py GROUP_CONFIGS);
  * trajectories — five steps of every variant of tests/optim_cases.py VARIANTS on EN-GDF-PN-S0 (resolution 64, weights from condition_state_dict(seed 0)), no forward
    pass: seeded gradients, seeded drift of the float buffers, a learning rate that differs every step (`set_optimizer_lr` on the 'cos' schedule).  Per variant: lr and d
    per step; 24 seeded samples per tensor of the DISPLACEMENT from the initial state of every parameter, EMA parameter and EMA float buffer in float64 (the truth) —
    displacement, because a parameter's value is right to 1e-7 whether or not its update is; and per class (parameters, EMA parameters, EMA float buffers) the largest displacement and torch
    float32's own deviation from the truth, max-abs and L2 (the yardstick).  One table in gen_train_rv_golden.py's format.
  * mutation checks, asserted here: float64 runs with the decay dropped, Nesterov dropped and one extra EMA tick (a second `ema.update` after the first step) must each
    move the compared quantity by at least 20 x the bound tests/test_optim.py derives from the yardstick — a fixture that cannot tell them apart is worthless.  (A
    counter that is merely off by one moves the EMA by only ~10 x the bound; it is held by `d_per_step`, which the test compares to 1e-12.)

Usage:  python tests/golden/gen_optim_golden.py
"""
import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path[:0] = [os.path.join(REPO, 'tests', 'oracle_shims'), os.path.join(REPO, 'tests'), REPO, REF]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn, optim  # noqa: E402

import optim_cases as OC  # noqa: E402
from achelous_amd.synth import condition_state_dict  # noqa: E402


def reference_model(ctor):
    from nets.Achelous import Achelous            # the reference (never copied)
    torch.manual_seed(0)
    return Achelous(**ctor)


def reference_groups(model, backbone):
    """train.py:499-518 on the imported model: (pg0, pg1, pg2) as parameter lists, or one list for 'rv'"""
    if backbone == 'rv':
        return [list(model.parameters())]
    pg0, pg1, pg2 = [], [], []
    for k, v in model.named_modules():
        if hasattr(v, 'bias') and isinstance(v.bias, nn.Parameter):
            pg2.append(v.bias)
        if isinstance(v, nn.BatchNorm2d) or 'bn' in k:
            pg0.append(v.weight)
        elif hasattr(v, 'weight') and isinstance(v.weight, nn.Parameter):
            pg1.append(v.weight)
    return [pg0, pg1, pg2]


def membership(model, backbone):
    names = {id(p): k for k, p in model.named_parameters()}
    groups = [[names[id(p)] for p in g] for g in reference_groups(model, backbone)]
    groups += [[] for _ in range(3 - len(groups))]
    taken = {k for g in groups for k in g}
    return groups + [[k for k in names.values() if k not in taken]]


def build_optimizer(model, v, drop_decay=False, drop_nesterov=False):
    wd = 0.0 if drop_decay else v['weight_decay']
    if v['groups'] == 'one':                      # train.py:514-518
        if v['kind'] == 'sgd':
            return optim.SGD(model.parameters(), weight_decay=wd, lr=v['lr'], foreach=False)
        return optim.AdamW(model.parameters(), weight_decay=wd, lr=v['lr'], foreach=False)
    pg0, pg1, pg2 = reference_groups(model, 'en')
    if v['kind'] == 'adam':
        opt = optim.Adam(pg0, v['lr'], betas=v['betas'], foreach=False)
    else:
        opt = optim.SGD(pg0, v['lr'], momentum=v['momentum'], nesterov=v['nesterov'] and not drop_nesterov, foreach=False)
    opt.add_param_group({'params': pg1, 'weight_decay': wd})
    opt.add_param_group({'params': pg2})
    return opt


def run(v, dtype, base, sd, extra_tick=False, **mut):
    """one trajectory -> (lr per step, d per step, displacement of every parameter, of every EMA parameter / float buffer), float64 tensors"""
    from loss.detection_loss import ModelEMA, get_lr_scheduler, set_optimizer_lr
    model = copy.deepcopy(base)
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).train()
    opt = build_optimizer(model, v, **mut)
    ema = ModelEMA(model, updates=v['u0']) if v['u0'] is not None else None
    p0 = {k: p.detach().double().clone() for k, p in model.named_parameters()}
    e0 = {k: t.detach().double().clone() for k, t in ema.ema.state_dict().items() if t.dtype.is_floating_point} if ema else {}
    sched = get_lr_scheduler('cos', v['lr'], OC.MIN_LR, OC.STEPS)
    lrs, ds = [], []

    def after():
        if ema is not None:
            ema.update(model)
            if extra_tick and not ds:              # the mutation: the EMA ticks twice after the first step
                ema.update(model)
            ds.append(ema.decay(ema.updates))

    def set_lr(s):
        set_optimizer_lr(opt, sched, s)
        lrs.append(opt.param_groups[0]['lr'])
    OC.drive(model, opt, set_lr, after)
    dp = {k: p.detach().double() - p0[k] for k, p in model.named_parameters()}
    de = {k: t.detach().double() - e0[k] for k, t in ema.ema.state_dict().items() if k in e0} if ema else {}
    return lrs, ds, dp, de


def cat(d):
    return torch.cat([t.reshape(-1) for t in d.values()]) if d else torch.zeros(0, dtype=torch.float64)


def class_stat(truth, other):
    """[largest displacement, max-abs deviation of `other`, L2 of the displacement, L2 of the deviation] over all tensors of a class"""
    a, b = cat(truth), cat(other)
    return [float(a.abs().max()), float((a - b).abs().max()), float(a.norm()), float((a - b).norm())] if len(a) else [0.0] * 4


def split(truth, other, pnames, params):
    """the EMA's parameters (params) or its float buffers (not params) out of two state-dict-keyed tables"""
    return tuple({k: t for k, t in d.items() if (k in pnames) == params} for d in (truth, other))


def bound(stat):
    return min(2e-4, max(2.0 ** -20, 8 * stat[1] / stat[0]))


def main():
    meta = {'ctor': OC.CTOR, 'steps': OC.STEPS, 'weight_seed': OC.WEIGHT_SEED, 'groups': {}, 'variants': {}}
    for name, ctor in OC.GROUP_CONFIGS.items():
        meta['groups'][name] = membership(reference_model(ctor), ctor['backbone'])
        print(name, [len(g) for g in meta['groups'][name]])
    base = reference_model(OC.CTOR)
    sd = condition_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in base.state_dict().items()}, seed=OC.WEIGHT_SEED)
    meta['param_names'] = [k for k, _ in base.named_parameters()]                   # the order the seeds of tests/optim_cases.py index
    meta['buffer_names'] = [k for k, _ in OC.float_buffers(base)]
    rng = np.random.default_rng(11)
    shapes = {k: p.numel() for k, p in base.named_parameters()}
    shapes.update({'ema::' + k: t.numel() for k, t in base.state_dict().items() if t.dtype.is_floating_point})
    idx = {k: np.sort(rng.choice(n, size=min(OC.NS, n), replace=False)).astype(np.int32) for k, n in shapes.items()}
    names = list(idx)
    store = {'names::json': np.frombuffer(json.dumps(names, separators=(',', ':')).encode(), dtype=np.uint8), 'count': np.array([len(idx[k]) for k in names], dtype=np.int32),
             'idx': np.zeros((len(names), OC.NS), dtype=np.int32)}
    for r, k in enumerate(names):
        store['idx'][r, :len(idx[k])] = idx[k]
    runs, pnames = {}, set(shapes) - {k for k in shapes if k.startswith('ema::')}
    for vname, v in OC.VARIANTS.items():
        lrs, ds, dp, de = runs[vname] = run(v, torch.float64, base, sd)
        _, ds32, dp32, de32 = run(v, torch.float32, base, sd)
        rows = {**dp, **{'ema::' + k: t for k, t in de.items()}}
        val = np.zeros((len(names), OC.NS))
        for r, k in enumerate(names):
            if k in rows:
                val[r, :len(idx[k])] = rows[k].reshape(-1).numpy()[idx[k]]
        store[vname + '/val'] = val if de else val[:len(dp)]
        meta['variants'][vname] = dict(v, lr_per_step=lrs, d_per_step=ds, param_stat=class_stat(dp, dp32), ema_param_stat=class_stat(*split(de, de32, pnames, True)),
                                       ema_buffer_stat=class_stat(*split(de, de32, pnames, False)))
        print(vname, 'lr', lrs, 'd', ds, *[(c, meta['variants'][vname][c]) for c in ('param_stat', 'ema_param_stat', 'ema_buffer_stat')])

    # ---- mutation checks (float64): each must move the compared quantity by >= 20 x the test's bound
    def moved(truth, other, stat):
        return float((cat(truth) - cat(other)).abs().max()) / stat[0]
    mv = {}
    for vname in ('sgd_wd5e-2',):
        v, st = OC.VARIANTS[vname], meta['variants'][vname]
        _, _, dp, de = runs[vname]
        mv['decay dropped'] = (moved(dp, run(v, torch.float64, base, sd, drop_decay=True)[2], st['param_stat']), bound(st['param_stat']))
        mv['nesterov dropped'] = (moved(dp, run(v, torch.float64, base, sd, drop_nesterov=True)[2], st['param_stat']), bound(st['param_stat']))
    # the tick is told apart on the EMA's PARAMETERS and on its BUFFERS, each against its own largest displacement, in both EMA regimes (updates from 0 and from 3000)
    for vname in ('sgd_wd5e-4', 'sgd_wd5e-2'):
        v, st = OC.VARIANTS[vname], meta['variants'][vname]
        de, dm = runs[vname][3], run(v, torch.float64, base, sd, extra_tick=True)[3]
        for cls, params in (('ema_param_stat', True), ('ema_buffer_stat', False)):
            mv[f'one extra EMA tick ({vname}, {cls})'] = (moved(*split(de, dm, pnames, params), st[cls]), bound(st[cls]))
    tick = {k: m / b for k, (m, b) in mv.items() if 'tick' in k}
    print('one extra EMA tick, moved / bound:', tick)
    best = max(tick, key=tick.get)
    mv = {k: x for k, x in mv.items() if 'tick' not in k or k == best}
    for what, (m, b) in mv.items():
        print(f'mutation: {what}: moves the displacement {m:.2e} relative, bound {b:.2e} ({m / b:.0f} x)')
        assert m >= 20 * b, (what, m, b)
    meta['mutations'] = {k: {'moved': m, 'bound': b} for k, (m, b) in mv.items()}
    np.savez_compressed(os.path.join(HERE, 'optim_traj.npz'), **store)
    size = os.path.getsize(os.path.join(HERE, 'optim_traj.npz'))
    print('optim_traj.npz', size, 'bytes')
    assert size < 1 << 20
    json.dump(meta, open(os.path.join(HERE, 'optim_traj.meta.json'), 'w'), indent=1)


if __name__ == '__main__':
    main()
