"""What tests/golden/gen_optim_golden.py (the reference's optimizers and ModelEMA, float64 and float32) and tests/test_optim.py (achelous_amd.optim.FusedOptimizer)
share: the configurations whose group membership is recorded, the trajectory variants, and the seeded inputs of a trajectory — no forward pass: gradients and the
BatchNorm-like drift of the float buffers are drawn per (step, tensor)."""
import math

import torch

CTOR = dict(num_det=7, num_seg=9, phi='S0', resolution=64, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
GROUP_CONFIGS = {'en_s0_gdf': dict(CTOR), 'en_s0_cdf': dict(CTOR, neck='cdf'), 'mv_s0': dict(CTOR, backbone='mv'), 'rv_s0': dict(CTOR, backbone='rv')}
STEPS, WEIGHT_SEED, NS, MIN_LR = 5, 0, 24, 1e-4

# `groups`: 'reference' = train.py:499-513's pg0 / pg1 / pg2 on the EN-S0 model, 'one' = the 'rv' form (train.py:514-518: all parameters, one group) on the same model.
# `lr` is 1e-2 for every variant, Adam's too: what is compared is the displacement over five steps, and float32 resolves it only where it is large against one ulp of
# the weights themselves (~1.2e-7 at |w| ~ 1).  At Adam's usual 1e-3 the displacement is ~2e-3 and torch's OWN float32 run is 1e-4 .. 2.6e-4 of it from the float64
# truth — above the 2e-4 cap of the bound, a case no float32 implementation can pass; at 1e-2 it is ~1e-5.
# `u0`: ModelEMA(model, updates=u0) — at 0 d is ~5e-4 and the EMA nearly a copy, at 3000 d is ~0.78; None: no EMA.
VARIANTS = {
    'sgd_wd5e-4': dict(kind='sgd', groups='reference', lr=1e-2, momentum=0.937, nesterov=True, weight_decay=5e-4, u0=0),
    'sgd_wd5e-2': dict(kind='sgd', groups='reference', lr=1e-2, momentum=0.937, nesterov=True, weight_decay=5e-2, u0=3000),
    'adam': dict(kind='adam', groups='reference', lr=1e-2, betas=(0.937, 0.999), weight_decay=5e-4, u0=3000),
    'rv_sgd': dict(kind='sgd', groups='one', lr=1e-2, momentum=0.0, nesterov=False, weight_decay=5e-4, u0=None),
    'rv_adamw': dict(kind='adamw', groups='one', lr=1e-2, betas=(0.9, 0.999), weight_decay=5e-4, u0=0),
}


def cos_lr(lr, min_lr, total, it):
    """the 'cos' schedule of the reference's get_lr_scheduler (loss/detection_loss.py:488-514) at its default ratios, restated; the fixture holds the reference's values"""
    warm = min(max(0.05 * total, 1), 3)
    start = max(0.1 * lr, 1e-6)
    no_aug = min(max(0.05 * total, 1), 15)
    if it <= warm:
        return (lr - start) * pow(it / float(warm), 2) + start
    if it >= total - no_aug:
        return min_lr
    return min_lr + 0.5 * (lr - min_lr) * (1.0 + math.cos(math.pi * (it - warm) / (total - warm - no_aug)))


def has_grad(i, s):
    """parameter i at step s: i % 50 == 7 never gets a gradient, i % 50 == 9 gets one from step 2 on"""
    return i % 50 != 7 and (i % 50 != 9 or s >= 2)


def grad_of(i, s, shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(1000 * s + i))


def drift_of(i, s, shape):
    return 0.01 * torch.randn(tuple(shape), generator=torch.Generator().manual_seed(777000 + 1000 * s + i))


def float_buffers(model):
    return [(k, b) for k, b in model.named_buffers() if b.is_floating_point()]


def drive(model, optimizer, set_lr, after_step=None, steps=STEPS):
    """`steps` steps on `model`: set_lr(s), the seeded gradients and buffer drift in the model's dtype and device, optimizer.step(), after_step() (the reference's ema.update)"""
    params, bufs = list(model.named_parameters()), float_buffers(model)
    for s in range(steps):
        set_lr(s)
        with torch.no_grad():
            for i, (_, p) in enumerate(params):
                p.grad = grad_of(i, s, p.shape).to(device=p.device, dtype=p.dtype) if has_grad(i, s) else None
            for i, (_, b) in enumerate(bufs):
                b.add_(drift_of(i, s, b.shape).to(device=b.device, dtype=b.dtype))
        optimizer.step()
        if after_step is not None:
            after_step()


class Standin(torch.nn.Module):
    """The smallest shapes that walk slot tails (1, 3, 255, 257, 1023, 4097), exact fits (256) and multi-chunk tensors, spread over the three groups, plus one parameter
    in no group, one whose gradient is always None (`never`), one that gains a gradient at step 2 (`late`), a float buffer of 5 elements and an int64 buffer."""
    SIZES = (1, 3, 255, 256, 257, 1023, 4097)

    def __init__(self, seed=3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for i, n in enumerate(self.SIZES):
            self.register_parameter(f'p{i}', torch.nn.Parameter(torch.randn(n, generator=g)))
        self.never = torch.nn.Parameter(torch.randn(300, generator=g))
        self.late = torch.nn.Parameter(torch.randn(7, 37, generator=g))
        self.loose = torch.nn.Parameter(torch.randn(513, generator=g))            # in no group
        self.register_buffer('stat', torch.randn(5, generator=g))
        self.register_buffer('count', torch.tensor(11, dtype=torch.int64))

    def groups(self, weight_decay):
        """three torch-style groups: (p0, p3, p6, never) without decay, (p1, p4, late) with, (p2, p5) without"""
        return [{'params': [self.p0, self.p3, self.p6, self.never], 'weight_decay': 0.0}, {'params': [self.p1, self.p4, self.late], 'weight_decay': weight_decay},
                {'params': [self.p2, self.p5], 'weight_decay': 0.0}]

    def standin_grads(self, s):
        """step s: a seeded gradient for every grouped parameter but `never`, `late` from step 2 on, none for `loose` (it is in no group)"""
        for i, (k, p) in enumerate(self.named_parameters()):
            on = k not in ('never', 'loose') and (k != 'late' or s >= 2)
            p.grad = grad_of(i, s, p.shape).to(device=p.device, dtype=p.dtype) if on else None
        with torch.no_grad():
            self.stat.add_(drift_of(0, s, self.stat.shape).to(device=self.stat.device, dtype=self.stat.dtype))
