"""The cases of tests/test_ln_gemm_rows_once.py and of its fixture generator tests/golden/gen_ln_gemm_parent.py: production plans of the 16-bit engines on the CPU
emulation, the taps behind the LayerNorm-prologue GEMMs (k_lngemm.h) and the six network outputs, as the exact bits of the storage type.

Shapes: the smallest at which the row-tile-resident kernel can go wrong.
  en_s0 / 96 / batch 1   maps 24 / 12 / 6 / 3: the last patchify conv has 9 rows (one partial tile), a qkv group 36 and 9 tokens (the tile tail inside a group),
                         N = 176 and 528 end in partial chunks, N = 48 is a single partial chunk;
  en_s0 / 160 / batch 3  maps 40 / 20 / 10 / 5: 75 rows in the last patchify conv, qkv groups of 100 and 25 tokens, several workgroups per launch;
  en_s2 / 64 / batch 1   widths that are not instantiated: the launches stay on gemm_body."""
import hashlib
import json
import os

import numpy as np
import torch

from achelous_amd.engine import DTYPE_BF16, DTYPE_F16
from achelous_amd.synth import condition_state_dict, make_inputs
from emu_util import alloc_outputs, make_engine
from golden_util import GOLDEN_DIR

CASES = [('en_s0', 96, 1), ('en_s0', 160, 3), ('en_s2', 64, 1)]
STORAGE = {'f16': (DTYPE_F16, torch.float16), 'bf16': (DTYPE_BF16, torch.bfloat16)}
TAPS = ('backbone.ds1', 'backbone.ds2', 'backbone.ds3', 'map3', 'map4', 'map5')
OUTPUTS = ('det0', 'det1', 'det2', 'se_seg', 'lane_seg', 'pc_seg')
NPTS = 16
FULL_ELEMS = 32768                     # tensors up to this size are stored whole (torch.equal); every tensor is stored as the SHA-256 of its bits
FIXTURE_JSON = os.path.join(GOLDEN_DIR, 'ln_gemm_parent.json')
FIXTURE_NPZ = os.path.join(GOLDEN_DIR, 'ln_gemm_parent.npz')


def case_id(name, res, batch, storage):
    return f'{name}/{res}/b{batch}/{storage}'


def setup(name, res, batch):
    meta = json.load(open(os.path.join(GOLDEN_DIR, name + '.keys.json')))
    kw = dict(meta['ctor'])
    kw['resolution'] = res
    blank = {k: torch.zeros(s, dtype=getattr(torch, dt)) for k, s, dt in meta['keys']}
    sd = condition_state_dict(blank, seed=0)
    return kw, sd, make_inputs(batch, 7, resolution=res, num_points=NPTS, pc_channels=kw['pc_channels'], radar_cells=40)


def bits(t, td):
    """a tensor of values of the storage type -> its 16-bit patterns (int16, contiguous)"""
    return t.to(td).contiguous().view(torch.int16)


def digest(b):
    return hashlib.sha256(np.ascontiguousarray(b.numpy()).tobytes()).hexdigest()


def run(lib, name, res, batch, storage, options=None):
    """One forward of the production plan (full_taps = 0) -> ({tap or output: int16 bit patterns}, launch names)."""
    dtype, td = STORAGE[storage]
    kw, sd, (x, xr, xp) = setup(name, res, batch)
    from achelous_amd.engine import NativeEngine
    eng = NativeEngine(lib, num_det=kw['num_det'], num_seg=kw['num_seg'], phi=kw['phi'], backbone=kw['backbone'], resolution=res, pc_channels=kw['pc_channels'],
                       pc_classes=kw['pc_classes'], num_points=NPTS, nano_head=kw['nano_head'], spp=kw['spp'], dtype=dtype)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    eng.load_state_dict(sd)
    eng.plan(batch)
    outs = alloc_outputs(kw, batch, NPTS, td, 'cpu')
    eng.forward(x.to(td), xr.to(td), xp.to(td), outs)
    got = {t: bits(eng.read_tap(t), td) for t in TAPS}
    got.update({k: bits(o, td) for k, o in zip(OUTPUTS, outs)})
    return got, [n for n, _, _ in eng.op_table()]
