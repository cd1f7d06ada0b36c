"""Per-tensor relative errors of the three engines (fp32, fp16 storage, bf16 storage; the 16-bit engines behind bf16 tensors) on the rv_* fixtures of the imported
reference, with the 16-bit bound of tests/repvit_cases.h16_bound: writes profiles/rv_parity_table.txt.
usage: python profiles/scripts/rv_parity_table.py [--out profiles/rv_parity_table.txt]"""
import argparse
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [os.path.join(REPO, 'tests'), REPO]
from achelous_amd import Achelous                                                      # noqa: E402
from repvit_cases import FIXTURES, fixture_case, fixture_errors, h16_bound             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), 'rv_parity_table.py measures on the GPU'
lines = ['RepViT backbone on the MI355X: relative error (max|a-b| / max|b| over the stored elements) of every tensor of the rv_* fixtures of the imported reference,',
         'per engine: fp32 / fp16 storage / bf16 storage (the 16-bit engines behind bf16 tensors), and the 16-bit bound of tests/repvit_cases.h16_bound in brackets',
         '(max(H16_TOL, 2 x the reference\'s drift under bf16 autocast) for the six outputs, max(2e-2, 3 x that figure) for internal taps; the fp32 bound is 1e-3).', '']
for name in FIXTURES:
    g, kw, sd, (x, xr, xp) = fixture_case(name)
    errs = {}
    for tag, dt, storage in (('f32', torch.float32, 'f16'), ('f16', torch.bfloat16, 'f16'), ('bf16', torch.bfloat16, 'bf16')):
        m = Achelous(**kw).eval()
        m.debug_taps, m.bf16_storage, m.f16_guard = True, storage, 'off'
        m.load_state_dict(sd, strict=True)
        m = m.cuda()
        with torch.no_grad():
            det, se, lane, pc = m(x.cuda().to(dt), xr.cuda().to(dt), xp.cuda().to(dt))
        torch.cuda.synchronize()
        e = m.native_engine(dt)
        errs[tag] = fixture_errors(g, (*det, se, lane, pc), e.read_tap, e.tap_names(), check_sums=False)
    worst = {t: max(v.values()) for t, v in errs.items()}
    lines.append(f'{name}: {len(errs["f32"])} tensors; worst fp32 {worst["f32"]:.2e}, fp16 storage {worst["f16"]:.2e}, bf16 storage {worst["bf16"]:.2e}')
    for k in errs['f32']:
        lines.append(f'  {k:18s} {errs["f32"][k]:.1e} / {errs["f16"][k]:.1e} / {errs["bf16"][k]:.1e}  ({h16_bound(g, k):.1e})')
    lines.append('')
print('\n'.join(lines))
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines))
