"""What the two RepViT test files share (tests/test_repvit_host.py on the CPU emulation library, tests/test_gpu_repvit.py on the MI355X): the
fixtures' weights and inputs, and the bounds.  The yardstick is the imported reference itself through the rv_* fixtures (tests/golden/gen_rv_golden.py);
tests/repvit_ref.py is the truth for shapes that have no fixture."""
import hashlib
import json

import torch

from achelous_amd.synth import condition_state_dict, make_inputs
from golden_util import Golden, ctor_kwargs

FIXTURES = ('rv_s0', 'rv_s2', 'rv_s1_r96', 'rv_s0_r64', 'rv_s2_cdf_r64')
OUTPUTS = ('det0', 'det1', 'det2', 'se_seg', 'lane_seg', 'pc_seg')
F32_TOL = 1e-3                   # the project's fp32 contract against the reference (tests/test_gpu_parity.py)
H16_TOL = {'det0': 1e-2, 'det1': 1e-2, 'det2': 1e-2, 'pc_seg': 1e-2, 'se_seg': 2e-2, 'lane_seg': 3e-2}      # the 16-bit engines' output bounds (tests/test_gpu_parity.py)
NUM_POINTS = 512


def h16_bound(g, tap):
    """The 16-bit engines against the reference's fp32 fixture, measured against the reference's own drift under bf16 autocast (the fixture's
    `bf16_autocast_reference_err`): outputs max(H16_TOL, 2 x that figure), internal taps max(2e-2, 3 x that figure)."""
    ref = g.meta['bf16_autocast_reference_err'].get(tap, 0.0)
    return max(H16_TOL[tap], 2.0 * ref) if tap in OUTPUTS else max(2e-2, 3.0 * ref)


def fixture_keys(g):
    """The reference's state-dict key list [[key, shape, dtype], ...] of a rv_* fixture: JSON text inside the .npz, its sha256 in the .keys.json."""
    text = g.npz[g.meta['keys_entry']].tobytes()
    assert hashlib.sha256(text).hexdigest() == g.meta['keys_sha256']
    keys = json.loads(text)
    assert len(keys) == g.meta['n_keys']
    return keys


def fixture_case(name):
    """(fixture, constructor keywords, state dict with the fixture's calibration, (image, radar, points))"""
    g = Golden(name)
    kw = ctor_kwargs(g.meta)
    blank = {k: torch.zeros(s, dtype=getattr(torch, dt)) for k, s, dt in fixture_keys(g)}
    sd = g.calibrate(condition_state_dict(blank, seed=g.meta['weight_seed']))
    inputs = make_inputs(g.meta['batch'], g.meta['input_seed'], resolution=kw['resolution'], num_points=NUM_POINTS, pc_channels=kw['pc_channels'])
    return g, kw, sd, inputs


def fixture_errors(g, outs, read_tap, tap_names, check_sums=True):
    """rel err of every tensor the fixture stores (except `decoded`); a stored tap the engine does not have is an error"""
    named = dict(zip(OUTPUTS, outs))
    errs = {}
    for tap in g.taps:
        if tap == 'decoded':
            continue
        assert tap in named or tap in tap_names, f'the engine has no tap {tap}'
        t = named[tap].float() if tap in named else read_tap(tap)
        errs[tap] = g.rel_err(tap, t, check_sums=check_sums)
    return errs


# ---------------------------------------------------------------------------------------------------- the training step (tests/golden/gen_train_rv_golden.py)
ZERO_GRAD_FLOOR = 5e-6           # tests/test_train_graph.py: a gradient that is zero in exact arithmetic is held to this fraction of the step's largest gradient


def train_fixture():
    """(meta, {name: (idx, val, stat)}) of train_rv_s0; stat = |truth|_2, |truth|_inf, torch-fp32 deviation as L2 and as max-abs"""
    import os
    import numpy as np
    from golden_util import GOLDEN_DIR
    meta = json.load(open(os.path.join(GOLDEN_DIR, 'train_rv_s0.meta.json')))
    fx = np.load(os.path.join(GOLDEN_DIR, 'train_rv_s0.npz'))
    names = json.loads(fx['names::json'].tobytes())
    return meta, {n: (fx['idx'][r, :c], fx['val'][r, :c], fx['stat'][r]) for r, (n, c) in enumerate(zip(names, fx['count']))}


def train_check(dev):
    """One training step of Achelous(backbone='rv') on `dev` against the reference's float64 step, with tests/test_train_graph.py's rules: loss, outputs
    max(2e-3, 6 x torch-fp32's own deviation), gradients max(5e-3, 8 x), running statistics max(1e-3, 6 x).  The absolute clause for gradients dominated by
    cancellation: max-abs error <= max(ZERO_GRAD_FLOOR x the step's largest gradient, 8 x torch-fp32's stored max-abs deviation of that tensor).  The parameters
    without gradient are exactly the fixture's list (the block behind the last map), whose running statistics are compared like every other."""
    import numpy as np
    from achelous_amd import Achelous
    meta, fx = train_fixture()
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
    loss = float(loss.detach())

    def compare(name, t):
        idx, val, stat = fx[name]
        ours = t.detach().double().cpu().reshape(-1).numpy()[idx]
        return np.linalg.norm(ours - val) / (np.linalg.norm(val) + 1e-300), stat[2] / (stat[0] + 1e-300), np.abs(ours - val).max(), stat[3]

    report = []
    assert abs(loss - meta['loss']) <= 5 * abs(meta['loss_torch_f32'] - meta['loss']) + 1e-4 * abs(meta['loss']), (loss, meta['loss'], meta['loss_torch_f32'])
    for k, o in enumerate(outs):
        err, ref, _, _ = compare(f'out{k}', o)
        report.append((err, ref, f'out{k}'))
        assert err <= max(2e-3, 6 * ref), (f'out{k}', err, ref)
    params = dict(m.named_parameters())
    gscale = max(float(s[1]) for n, (_, _, s) in fx.items() if n.startswith('grad::'))
    assert sorted(k for k, p in params.items() if p.grad is None) == sorted(meta['parameters_without_gradient'])
    n = 0
    for k, p in params.items():
        if p.grad is None:
            continue
        err, ref, amax, tmax = compare('grad::' + k, p.grad)
        absolute = amax <= max(ZERO_GRAD_FLOOR * gscale, 8 * tmax)
        if not absolute:
            report.append((err, ref, k))
        assert err <= max(5e-3, 8 * ref) or absolute, (k, err, ref, amax, tmax, gscale)
        n += 1
    assert n == sum(1 for k in fx if k.startswith('grad::'))
    nbuf = 0
    for k, v in m.named_buffers():
        if k.endswith(('running_mean', 'running_var')):
            err, ref, amax, _ = compare('buf::' + k, v)
            assert err <= max(1e-3, 6 * ref) or amax <= 1e-6, (k, err, ref)
            nbuf += 1
        if k.endswith('num_batches_tracked'):
            assert int(v) == 1, k
    assert nbuf == sum(1 for k in fx if k.startswith('buf::'))
    return sorted(report, reverse=True)[:8]
