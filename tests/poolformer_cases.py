"""What the two PoolFormer test files share (tests/test_poolformer_host.py on the CPU emulation library, tests/test_gpu_poolformer.py on the MI355X): the
fixtures' weights and inputs, and the bounds.  The yardstick is the imported reference itself through the pf_* fixtures (tests/golden/gen_pf_golden.py);
tests/poolformer_ref.py is the truth for shapes that have no fixture."""
import hashlib
import json

import torch

from achelous_amd.synth import condition_state_dict, make_inputs
from golden_util import Golden, ctor_kwargs

FIXTURES = ('pf_s0', 'pf_s2', 'pf_s1_r96', 'pf_s0_r64', 'pf_s0_cdf_r64')
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
    """The reference's state-dict key list [[key, shape, dtype], ...] of a pf_* fixture: JSON text inside the .npz, its sha256 in the .keys.json."""
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
