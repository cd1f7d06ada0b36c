"""Time of the validation metrics (achelous_amd/metrics.py) on the GPU against what the package offered before for the same result:
  confusion matrix   A `SegConfusion.update`   B torch on the device: argmax + `torch.bincount` (it reads the maximum back: a synchronisation per call)
                     C copy of the logits to the host + numpy argmax + the reference's `fast_hist` formula (np.bincount)
  matching           A `DetectionAP.update`    C copy of rows to the host + the reference's per-detection loop (tests/metrics_cases.py::host_match)
Device events around synchronised work for A and B, a host clock around work that ends synchronised for C; warm-up; >= 0.5 s of timed work per fast leg; legs
alternated in one process; median and spread over the rounds.  Every leg's result is checked against A's before anything is timed.
usage: python profiles/scripts/metrics_timing.py [--batch 64] [--rounds 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
import metrics_cases as MC                               # noqa: E402
from achelous_amd import metrics as M                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--resolution', type=int, default=320)
ap.add_argument('--out', default=None)
a = ap.parse_args()
dev, B, R, C = 'cuda', a.batch, a.resolution, 9
g = torch.Generator().manual_seed(0)
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def realistic_labels():
    """mostly water (class 0), a shore band, a few rectangular objects per frame, 2 % ignored (class 9): what a USV frame looks like to the histogram"""
    lab = torch.zeros(B, R, R, dtype=torch.int64)
    lab[:, :R // 5] = 1
    for b in range(B):
        for _ in range(4):
            y, x = [int(v) for v in torch.randint(R // 5, R - 40, (2,), generator=g)]
            h, w = [int(v) for v in torch.randint(8, 40, (2,), generator=g)]
            lab[b, y:y + h, x:x + w] = int(torch.randint(2, C, (1,), generator=g))
    lab[torch.rand(B, R, R, generator=g) < 0.02] = C
    return lab


def logits_for(lab, noise):
    x = torch.randn(B, C, R, R, generator=g) * noise
    x.scatter_add_(1, lab.clamp(max=C - 1).unsqueeze(1), torch.full((B, 1, R, R), 3.0))
    return x.to(torch.bfloat16)


def timed_events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def timed_host(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def iters_for(fn, timer, target_ms=500.0, cap=20000):
    fn()
    one = timer(fn, 3)
    return max(1, min(cap, int(target_ms / max(one, 1e-3))))


def report(name, legs):
    """legs: [(label, fn, timer)], alternated over the rounds"""
    n = [iters_for(fn, timer) for _, fn, timer in legs]
    t = [[] for _ in legs]
    for _ in range(a.rounds):
        for i, (_, fn, timer) in enumerate(legs):
            t[i].append(timer(fn, n[i]))
    say(f'  {name}')
    med = []
    for i, (label, _, _) in enumerate(legs):
        med.append(statistics.median(t[i]))
        say(f'    {label:<66s}: {med[i]:9.3f}  ({min(t[i]):.3f} .. {max(t[i]):.3f}; {n[i]} calls per round)')
    for i in range(1, len(legs)):
        say(f'    {legs[i][0][0]} / A = {med[i] / med[0]:.2f}')
    return med


say(f'profiles/scripts/metrics_timing.py on one MI355X (device events / a host clock around synchronised work, warm-up, >= 0.5 s of timed work per leg and round, legs '
    f'alternated in one process; ms per call, median of {a.rounds} rounds, min .. max)')
say()
say(f'confusion matrix, batch {B} at {R} x {R}, {C} classes, bf16 logits [B, C, H, W] ({B * C * R * R * 2 / 1e6:.1f} MB), int64 labels ({B * R * R * 8 / 1e6:.1f} MB)')
for title, lab, noise in (('realistic label map (mostly water, 2 % ignored), noisy logits', realistic_labels(), 0.7),
                          ('every pixel in one bin', torch.zeros(B, R, R, dtype=torch.int64), 0.0)):
    x, lab = logits_for(lab, noise).to(dev), lab.to(dev)
    acc = M.SegConfusion(C, dev)

    def native():
        acc.update(x, lab)

    def torch_dev():
        pred = x.argmax(1)
        k = (lab >= 0) & (lab < C)
        return torch.bincount(C * lab[k] + pred[k], minlength=C * C).reshape(C, C)

    def host():
        xs, ls = x.float().cpu().numpy(), lab.cpu().numpy().reshape(-1)
        pred = xs.argmax(1).reshape(-1)
        k = (ls >= 0) & (ls < C)
        return np.bincount(C * ls[k].astype(int) + pred[k], minlength=C ** 2).reshape(C, C)
    native()
    ref = acc.hist.cpu().numpy().copy()
    assert np.array_equal(torch_dev().cpu().numpy(), ref) and np.array_equal(host(), ref), 'the legs disagree'
    say(f'  (largest bin holds {ref.max() / max(ref.sum(), 1) * 100:.1f} % of the {int(ref.sum())} counted pixels; all three legs give the same matrix)')
    med = report(title, [('A SegConfusion.update (one launch, no host read)', native, timed_events),
                         ('B torch on the device: argmax + mask + torch.bincount (synchronises)', torch_dev, timed_events),
                         ('C logits to the host + numpy argmax + np.bincount (fast_hist)', host, timed_host)])
    mb = (B * C * R * R * 2 + B * R * R * 8) / 1e6
    say(f'    A reads {mb:.1f} MB per call: {mb / med[0] / 1e3:.2f} TB/s by call time (launch overhead included), {mb / med[0] / 1e3 / 8 * 100:.0f} % of the 8 TB/s HBM peak')
    del x, lab

say()
rows, counts, gt, gt_counts, difficult = [np.concatenate([v] * (B // 8)) for v in MC.make_det_case()]
say(f'detection matching, batch {B}: rows [{B}, {MC.MAX_DET}, 7] with {int(counts.sum())} detections, {int(gt_counts.sum())} boxes (G = {MC.MAX_GT}), '
    f'{len(MC.THRESHOLDS)} IoU thresholds in one launch')
d_rows, d_counts, d_gt, d_gtc, d_diff = [torch.from_numpy(v).to(dev) for v in (rows, counts, gt, gt_counts, difficult)]
det = M.DetectionAP(MC.NUM_DET, MC.THRESHOLDS, MC.MAX_DET, capacity_images=B, device=dev)


def native_match():
    det.images = 0
    det.update(d_rows, d_counts, d_gt, d_gtc, d_diff)


def host_match():
    return MC.host_match(d_rows.cpu().numpy(), d_counts.cpu().numpy(), gt, gt_counts, difficult, MC.THRESHOLDS, truncate=True)


native_match()
h = host_match()
assert np.array_equal(det.flags.cpu().numpy(), h[0]) and np.array_equal(det.iou.cpu().numpy(), h[2]), 'the legs disagree'
report('DetectionAP.update', [('A DetectionAP.update (one launch + two slab copies, no host read)', native_match, timed_events),
                              ('C rows to the host + the reference\'s loop per detection and box (Python)', host_match, timed_host)])
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
