"""Step time of the RepViT configurations against EdgeNeXt-S0 and PoolFormer-S0 in the same run: the pipelined submit_detect / wait serving loop of bench.py's
headline (bf16 tensors, fp16 storage, batch 64, 320 x 320, conf 0.35 / iou 0.35 / 100 detections), RV-GDF-PN-S0, EN-GDF-PN-S0 and PF-GDF-PN-S0 alternated in one
process on the same card, then RV-S1 and RV-S2: >= 5 rounds of >= 0.5 s of fenced work each, median and spread of the rounds.  bench.py itself does not cover these
configurations.  Then, for RV-S0, every launch of one forward bracketed by device events (ach_forward_profiled: isolated times, no overlap between streams), summed
per kernel of the backbone and per map size — which launches carry the backbone.
usage: python profiles/scripts/rv_timing.py [--batch 64] [--rounds 5] [--seconds 0.5] [--out profiles/rv_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO]
from achelous_amd import Achelous                                           # noqa: E402
from achelous_amd.spec import repvit_rows                                   # noqa: E402
from achelous_amd.synth import condition_state_dict, make_inputs            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--seconds', type=float, default=0.5)
ap.add_argument('--out', default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), 'rv_timing.py measures on the GPU: there is no CPU path'
B, R, DT = a.batch, 320, torch.bfloat16
COMMON = dict(num_det=7, num_seg=9, resolution=R, neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def runner(backbone, phi):
    m = Achelous(**dict(COMMON, backbone=backbone, phi=phi)).eval()
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=0))
    m = m.cuda()
    m.static_weights = True
    x, xr, xp = (t.cuda().to(DT) for t in make_inputs(B, 1236, resolution=R, pc_channels=5))
    state = {'inflight': None}

    def step():
        nxt = m.submit_detect(x, xr, xp, 0.35, 0.35, 100)
        if state['inflight'] is not None:
            state['inflight'].wait()
        state['inflight'] = nxt

    def fence():
        if state['inflight'] is not None:
            state['inflight'].wait()
            state['inflight'] = None
        torch.cuda.synchronize()

    def block(steps):
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        fence()
        return (time.perf_counter() - t0) / steps
    with torch.no_grad():
        block(10)                                   # warm-up: plan, code objects
        per = block(20)
    return m, block, max(20, int(a.seconds / per) + 1), (x, xr, xp)


def measure(legs):
    """legs: {tag: (block, steps)} alternated round by round -> {tag: [s per step per round]}"""
    ts = {k: [] for k in legs}
    with torch.no_grad():
        for _ in range(a.rounds):
            for k, (block, steps) in legs.items():
                ts[k].append(block(steps))
    return ts


def report(tag, t):
    med = statistics.median(t)
    say(f'  {tag:14s} {med * 1e3:7.3f} ms / step   {B / med:9.0f} frames/s   rounds {min(t) * 1e3:.3f} .. {max(t) * 1e3:.3f} ms   ({len(t)} rounds)')
    return med


say(f'pipelined submit_detect / wait loop, bf16 tensors (fp16 storage), batch {B}, {R} x {R}; {torch.cuda.get_device_name(0)}')
models = {}
legs = {}
for tag, bb, phi in (('RV-GDF-PN-S0', 'rv', 'S0'), ('EN-GDF-PN-S0', 'en', 'S0'), ('PF-GDF-PN-S0', 'pf', 'S0')):
    m, block, steps, inp = runner(bb, phi)
    models[tag] = (m, inp)
    legs[tag] = (block, steps)
ts = measure(legs)
say('RV-S0, EN-S0 and PF-S0 alternated round by round:')
med = {k: report(k, v) for k, v in ts.items()}
ratios = [e / r for r, e in zip(ts['RV-GDF-PN-S0'], ts['EN-GDF-PN-S0'])]
say(f'  RV-S0 / EN-S0 frames/s: {med["EN-GDF-PN-S0"] / med["RV-GDF-PN-S0"]:.3f}   (round by round {min(ratios):.3f} .. {max(ratios):.3f});   '
    f'RV-S0 / PF-S0: {med["PF-GDF-PN-S0"] / med["RV-GDF-PN-S0"]:.3f}')
for tag, phi in (('RV-GDF-PN-S1', 'S1'), ('RV-GDF-PN-S2', 'S2')):
    m, block, steps, inp = runner('rv', phi)
    t = measure({tag: (block, steps)})[tag]
    report(tag, t)
    del m, block

# ---- per-launch device-event times of one RV-S0 forward (isolated launches)
m, (x, xr, xp) = models['RV-GDF-PN-S0']
with torch.no_grad():
    outs = m(x, xr, xp)
    torch.cuda.synchronize()
    e = m.native_engine(DT)
    flat = (outs[0][0], outs[0][1], outs[0][2], outs[1], outs[2], outs[3])
    reps = [e.forward_profiled(x, xr, xp, flat) for _ in range(5)]
    torch.cuda.synchronize()
names = [o[0] for o in e.op_table()]
ms = [statistics.median(r[i] for r in reps) for i in range(len(names))]
pfx = 'image_radar_encoder.fpn.backbone.'
total = sum(ms)
bb = [(n[len(pfx):], t) for n, t in zip(names, ms) if n.startswith(pfx)]
say()
say(f'RV-S0, one forward with every launch bracketed by device events (median of 5): {len(names)} launches, {total:.3f} ms in all; backbone {len(bb)} launches, {sum(t for _, t in bb):.3f} ms')
kinds, totals = {}, {}
STRIDE2 = {i for i, row in enumerate(repvit_rows('S0'), 1) if row[2] == 2}
size = R // 4                                  # side of the map the launch works on: the stem and features[1..3] at R / 4, halved by every stride-2 block
for n, t in bb:
    leaf = n.rsplit('.', 1)[-1]
    stem = n.startswith('features.0.')
    kind = 'stem' if stem else {'dw': 'dw', 'gate': 'gate', 'mlp': 'mlp', 'pw': 'pw (stride-2 1x1)'}[leaf]
    if not stem and leaf == 'dw' and int(n.split('.')[1]) in STRIDE2:
        size //= 2                             # (the depthwise launch of a stride-2 block writes the smaller map)
    key = kind if stem else f'{kind} {size:3d} x {size:<3d}'
    c, s_ = kinds.get(key, (0, 0.0))
    kinds[key] = (c + 1, s_ + t)
    c, s_ = totals.get(kind, (0, 0.0))
    totals[kind] = (c + 1, s_ + t)
for key in sorted(kinds):
    c, s = kinds[key]
    say(f'  {key:18s} {c:3d} launches  {s * 1e3:8.1f} us  ({s / c * 1e3:6.1f} us each)')
say('totals:')
for key in sorted(totals):
    c, s = totals[key]
    say(f'  {key:18s} {c:3d} launches  {s * 1e3:8.1f} us  ({100.0 * s / sum(t for _, t in bb):4.1f} % of the backbone)')
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
