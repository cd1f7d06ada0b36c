"""SHA-256 of the bits of every output and every tap (full_taps = 1) of the golden-fixture cases that run the register-chained MLP kernels (mlp_kernel, ffn2_kernel,
pf_mlp_kernel, rv_mlp_kernel), for ONE engine library given by path: the CPU emulation library (tests/hostemu/libachelous_emu.so, host tensors) or the HIP library
(achelous_amd/libachelous_hip.so, tensors on cuda:0).  Run it on two builds of the library and compare the lists: a change that only moves code must leave every
digest as it was.
usage: python profiles/scripts/mlp_core_bits.py LIBRARY [--device cpu|cuda] [--only SUBSTRING] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
from achelous_amd.engine import DTYPE_BF16, DTYPE_F16, DTYPE_F32, NativeLibrary      # noqa: E402
from achelous_amd.synth import condition_state_dict, make_inputs                     # noqa: E402
from emu_util import alloc_outputs, make_engine                                      # noqa: E402
from golden_util import GOLDEN_DIR                                                   # noqa: E402
import poolformer_cases                                                              # noqa: E402
import repvit_cases                                                                  # noqa: E402

STORAGE = {'f32': (DTYPE_F32, torch.float32), 'bf16': (DTYPE_BF16, torch.bfloat16), 'f16': (DTYPE_F16, torch.float16)}
OUTPUTS = ('det0', 'det1', 'det2', 'se_seg', 'lane_seg', 'pc_seg')
# (fixture, resolution, batch, storage): the EdgeNeXt / MobileViT cases of tests/test_emulated_engine.py (seeded weights at a small resolution; mv_s2 bf16 at 128
# reaches ffn2_kernel) ...
SEEDED = [('en_s0', 64, 2, 'f32'), ('en_s0', 96, 1, 'bf16'), ('en_s0', 96, 1, 'f16'), ('en_s2', 64, 1, 'f32'), ('en_s2', 96, 1, 'f16'), ('mv_s2', 128, 1, 'bf16')]
# ... and the PoolFormer / RepViT fixtures with their own calibration, inputs and batch: (cases module, fixture, storage)
FIXTURES = ([(poolformer_cases, 'pf_s1_r96', 'f32'), (poolformer_cases, 'pf_s1_r96', 'bf16')] + [(repvit_cases, n, 'f32') for n in repvit_cases.FIXTURES] +
            [(repvit_cases, 'rv_s1_r96', 'bf16')])


def seeded_case(name, res, batch):
    meta = json.load(open(os.path.join(GOLDEN_DIR, name + '.keys.json')))
    kw = dict(meta['ctor'], resolution=res)
    sd = condition_state_dict({k: torch.zeros(s, dtype=getattr(torch, dt)) for k, s, dt in meta['keys']}, seed=0)
    return kw, sd, make_inputs(batch, 7, resolution=res, num_points=48, pc_channels=kw['pc_channels'], radar_cells=40), 48


def digest(t):
    t = t.detach().cpu().contiguous()
    raw = t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()
    return hashlib.sha256(np.ascontiguousarray(raw).tobytes()).hexdigest()


def run(lib, dev, tag, kw, sd, inputs, npts, storage):
    dtype, td = STORAGE[storage]
    batch = inputs[0].shape[0]
    eng = make_engine(lib, kw, batch, sd, npts, dtype, full_taps=True)
    outs = alloc_outputs(kw, batch, npts, td, dev)
    eng.forward(*(t.to(td).to(dev) for t in inputs), outs)
    if dev != 'cpu':
        torch.cuda.synchronize()
    rows = [(f'{tag} out {k}', digest(o)) for k, o in zip(OUTPUTS, outs)]
    rows += [(f'{tag} tap {t}', digest(eng.read_tap(t))) for t in eng.tap_names()]       # (taps come back as fp32 copies of the stored values: exact)
    return rows


ap = argparse.ArgumentParser()
ap.add_argument('library')
ap.add_argument('--device', default='cpu', choices=('cpu', 'cuda'))
ap.add_argument('--only', default='')
ap.add_argument('--out', default=None)
a = ap.parse_args()
lib = NativeLibrary(os.path.abspath(a.library))
rows = []
with torch.no_grad():
    for name, res, batch, storage in SEEDED:
        tag = f'{name}/{res}/b{batch}/{storage}'
        if a.only in tag:
            rows += run(lib, a.device, tag, *seeded_case(name, res, batch), storage)
            print(tag, len(rows), flush=True)
    for cases, name, storage in FIXTURES:
        tag = f'{name}/{storage}'
        if a.only in tag:
            g, kw, sd, inputs = cases.fixture_case(name)
            rows += run(lib, a.device, tag, kw, sd, inputs, cases.NUM_POINTS, storage)
            print(tag, len(rows), flush=True)
text = ''.join(f'{d}  {k}\n' for k, d in rows)
text += f'{len(rows)} tensors; digest of the list: {hashlib.sha256(text.encode()).hexdigest()}\n'
if a.out:
    with open(a.out, 'w') as f:
        f.write(text)
print(text.splitlines()[-1])
