#!/usr/bin/env python3
"""Generate tests/golden/train_rv_s0.npz by IMPORTING the reference (read-only) in TRAINING mode: gen_train_golden.py's recipe with
backbone='rv' (RepViT-GDF-PN-S0, 96 x 96, batch 2).

One training step's worth of arithmetic: forward in `.train()` (BatchNorm on batch statistics), a fixed linear functional of all six
outputs as the loss, `backward()` through ATen autograd.  Stored as there — the six outputs, the loss, for EVERY parameter that gets a
gradient its L2 norm, largest magnitude and 24 seeded samples, for every BatchNorm the running statistics after the step — in float64
(the truth), plus per tensor torch's own float32 deviation from that truth: its L2 norm and, in addition, its MAX-ABS.

Specific to RepViT:
  * the reference runs the blocks behind the last out-slice in training mode too (features[26] of repvit_m1): their running statistics
    move and are stored like every other, their parameters get no gradient (`parameters_without_gradient`);
  * two families of gradients are zero in exact arithmetic — `token_mixer.0.conv1.c.weight` (a per-channel scale in front of a
    training-mode BatchNorm: zero up to the BatchNorm's eps, which shows in the channels whose drawn scale is tiny) and the stride-2
    `token_mixer.0.bn.bias` (a constant in front of a 1x1 conv + BatchNorm): what every evaluation returns there is dominated by
    cancellation, which is why the max-abs deviation of torch's float32 run is stored (the tests' absolute clause);
  * the per-tensor records are one table (`names::json`, `count`, `idx`, `val`, `stat`), not three zip members per tensor.

Usage:  python tests/golden/gen_train_rv_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path[:0] = [os.path.join(REPO, 'tests', 'oracle_shims'), REPO, REF]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from achelous_amd.synth import condition_state_dict, make_inputs  # noqa: E402

CTOR = dict(num_det=7, num_seg=9, phi='S0', resolution=96, backbone='rv', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
BATCH, NPTS, INPUT_SEED, COT_SEED, WEIGHT_SEED, NS = 2, 32, 77, 78, 0, 24


def cotangents(outs, dtype):
    g = torch.Generator().manual_seed(COT_SEED)
    return [torch.randn(o.shape, generator=g, dtype=torch.float64).to(dtype) for o in outs]


def run(dtype):
    from nets.Achelous import Achelous            # the reference (never copied)
    torch.set_default_dtype(dtype)                # the reference builds its positional-encoding tables in the default dtype
    torch.manual_seed(0)
    model = Achelous(**CTOR)
    sd = condition_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in model.state_dict().items()}, seed=WEIGHT_SEED)
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).train()
    torch.set_default_dtype(torch.float32)
    x, xr, xp = make_inputs(BATCH, INPUT_SEED, resolution=CTOR['resolution'], num_points=NPTS, pc_channels=CTOR['pc_channels'], radar_cells=20)
    torch.set_default_dtype(dtype)
    det, se, lane, pc = model(x.to(dtype), xr.to(dtype), xp.to(dtype))
    outs = [*det, se, lane, pc]
    loss = sum((o * c).sum() for o, c in zip(outs, cotangents(outs, dtype)))
    loss.backward()
    grads = {k: p.grad.detach().double() for k, p in model.named_parameters() if p.grad is not None}
    unused = [k for k, p in model.named_parameters() if p.grad is None]
    bufs = {k: v.detach().double() for k, v in model.named_buffers() if k.endswith(('running_mean', 'running_var'))}
    return [o.detach().double() for o in outs], float(loss), grads, bufs, unused


def main():
    outs64, loss64, g64, b64, unused = run(torch.float64)
    outs32, loss32, g32, b32, _ = run(torch.float32)
    torch.set_default_dtype(torch.float32)
    rng = np.random.default_rng(5)
    names, rows, meta = [], [], {'ctor': CTOR, 'batch': BATCH, 'num_points': NPTS, 'input_seed': INPUT_SEED, 'cotangent_seed': COT_SEED,
                       'weight_seed': WEIGHT_SEED, 'radar_cells': 20, 'loss': loss64, 'loss_torch_f32': loss32,
                       'parameters_without_gradient': unused}

    def put(name, t64, t32):
        flat, f32 = t64.reshape(-1).numpy(), t32.reshape(-1).numpy()
        idx = np.sort(rng.choice(flat.size, size=min(NS, flat.size), replace=False)).astype(np.int64)
        names.append(name)
        rows.append((idx, flat[idx], np.array([np.linalg.norm(flat), np.abs(flat).max(), np.linalg.norm(f32 - flat), np.abs(f32 - flat).max()])))     # |t|_2, |t|_inf, torch-fp32 deviation (L2, max-abs)

    for k, (a, b) in enumerate(zip(outs64, outs32)):
        put(f'out{k}', a, b)
    for k in g64:
        put('grad::' + k, g64[k], g32[k])
    for k in b64:
        put('buf::' + k, b64[k], b32[k])
    # one table instead of three zip members per tensor (1100 tensors: the members' headers alone would pass the size limit of a committed file):
    # row r belongs to names[r]; `count[r]` of its NS slots are used
    store = {'names::json': np.frombuffer(json.dumps(names, separators=(',', ':')).encode(), dtype=np.uint8), 'count': np.array([len(r[0]) for r in rows], dtype=np.int32),
             'idx': np.zeros((len(rows), NS), dtype=np.int64), 'val': np.zeros((len(rows), NS)), 'stat': np.stack([r[2] for r in rows])}
    for r, (idx, val, _) in enumerate(rows):
        store['idx'][r, :len(idx)], store['val'][r, :len(idx)] = idx, val
    np.savez_compressed(os.path.join(HERE, 'train_rv_s0.npz'), **store)
    assert os.path.getsize(os.path.join(HERE, 'train_rv_s0.npz')) < 1 << 20
    stat = {n: r[2] for n, r in zip(names, rows)}
    json.dump(meta, open(os.path.join(HERE, 'train_rv_s0.meta.json'), 'w'), indent=1)
    dev = sorted(((stat['grad::' + k][2] / (stat['grad::' + k][0] + 1e-30), k) for k in g64), reverse=True)
    print(f"loss {loss64:.6f} (torch fp32 {loss32:.6f}); {len(g64)} parameter gradients, {len(b64)} running statistics")
    print("largest torch-fp32 relative deviations:", [(f'{d:.2e}', k) for d, k in dev[:6]])
    print("parameters the forward never touches:", unused)
    zero = [k for k in g64 if k.endswith('token_mixer.0.conv1.c.weight') or (k.endswith('token_mixer.0.bn.bias'))]
    gmax = max(float(g64[k].abs().max()) for k in g64)
    print(f"largest gradient {gmax:.3e}; the {len(zero)} gradients that are zero in exact arithmetic (up to the BatchNorm eps): float64 max-abs "
          f"{min(float(g64[k].abs().max()) for k in zero):.1e} .. {max(float(g64[k].abs().max()) for k in zero):.1e}, torch fp32 max-abs deviation "
          f"{min(float(stat['grad::' + k][3]) for k in zero):.1e} .. {max(float(stat['grad::' + k][3]) for k in zero):.1e}")


if __name__ == '__main__':
    main()
