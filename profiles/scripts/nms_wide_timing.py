"""Time of decode + NMS above 416 x 416 (csrc/k_nmswide.h: nms_wide_filter_kernel + nms_wide_kernel) beside the unchanged single-launch nms_kernel at 416 and
beside the forward of the same batch.
Workload per resolution R in 416 (the yardstick: nms_kernel), 448, 640, 864 and batch B in 1, 64 (32 at 864, where one plan takes 44 frames: activations below 2 GiB): seeded bf16 head maps [B, 12, R/s, R/s], s = 8, 16, 32 (7 classes).  300
anchors per image carry objectness and class logits of +3 (score about 0.9), all the others -3 (score about 0.002); x / y logits N(0, 0.5), w / h logits N(0.5, 0.5)
(boxes of about 1.6 cells).  The same maps serve both regimes: conf 0.35 -> 300 candidates per image, conf 0 -> every anchor is a candidate (above 5000 the per-class
rule).  nms_thres 0.45, max_det 100 (the serving setting; `all, max_det = A` repeats the conf 0 leg with every slot open, the evaluation-time worst case).
  decode     ach_decode alone
  nms 300    ach_nms alone, conf 0.35
  nms all    ach_nms alone, conf 0
  forward    Achelous EN-S0 (gdf, pn), bf16 tensors, the plain forward of the same batch
  detect     forward_detect of the same batch at conf 0.35 (decode + NMS ride the detection-branch stream)
Buffers are allocated once; device events around `iters` back-to-back calls, warm-up, >= 0.15 s of timed work per leg and round, legs alternated in one process, median
and spread of the rounds (measuring-on-mi355x).  Before anything is timed each NMS result is compared with the oracle on the first image.
usage: python profiles/scripts/nms_wide_timing.py [--rounds 5] [--out FILE] [--no-forward]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO]
from achelous_amd import Achelous                                   # noqa: E402
from achelous_amd._native import stateless_handle                   # noqa: E402
from achelous_amd.synth import condition_state_dict, make_inputs    # noqa: E402
from oracle.achelous_oracle import non_max_suppression as o_nms    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--no-forward', action='store_true')
ap.add_argument('--res', type=int, nargs='*', default=[416, 448, 640, 864])
ap.add_argument('--batch', type=int, nargs='*', default=[1, 64])
a = ap.parse_args()
C, IOU, MAX_DET, HOT = 7, 0.45, 100, 300
lines = []


def batches(R):
    return [min(B, 32) if R > 640 else B for B in a.batch]


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def timed_events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def iters_for(fn, target_ms=150.0, cap=2000):
    fn()
    one = timed_events(fn, 2)
    return max(1, min(cap, int(target_ms / max(one, 1e-3))))


def head_maps(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = [R // s for s in (8, 16, 32)]
    A = sum(n * n for n in sizes)
    flat = torch.empty(B, 5 + C, A)
    flat[:, 0:2] = torch.randn(B, 2, A, generator=g) * 0.5
    flat[:, 2:4] = torch.randn(B, 2, A, generator=g) * 0.5 + 0.5
    flat[:, 4:] = -3.0
    for b in range(B):
        hot = torch.randperm(A, generator=g)[:HOT]
        flat[b, 4:, hot] = 3.0
    maps, at = [], 0
    for n in sizes:
        maps.append(flat[:, :, at:at + n * n].reshape(B, 5 + C, n, n).contiguous().to(torch.bfloat16).cuda())
        at += n * n
    return maps, A


assert torch.cuda.is_available(), 'this script measures on the GPU'
say(f'device {torch.cuda.get_device_name(0)}; {C} classes, nms_thres {IOU}, max_det {MAX_DET}, {HOT} hot anchors per image; bf16 head maps; ms per call, '
    f'median [min .. max] of {a.rounds} rounds')
kw = dict(num_det=C, num_seg=9, phi='S0', backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
stream = None
table = {}
for R in a.res:
    model = None
    if not a.no_forward:
        model = Achelous(resolution=R, **kw).eval()
        model.load_state_dict(condition_state_dict(model.state_dict(), seed=0))
        model = model.cuda()
    for B in batches(R):
        maps, A = head_maps(B, R, 100 + R + B)
        h = stateless_handle(C, R, torch.bfloat16)
        hn = stateless_handle(C, R, torch.float32)
        st = torch.cuda.current_stream().cuda_stream
        dec = torch.empty(B, A, 5 + C, dtype=torch.float32, device='cuda')
        ws = torch.empty(hn.nms_workspace_bytes(B), dtype=torch.uint8, device='cuda')

        def outs(md):
            return (torch.empty(B, md, 7, dtype=torch.float32, device='cuda'), torch.empty(B, md, dtype=torch.int32, device='cuda'),
                    torch.empty(B, dtype=torch.int32, device='cuda'))
        o100, oA = outs(MAX_DET), outs(A)
        legs = {'decode': lambda: h.decode(B, maps[0], maps[1], maps[2], dec, st),
                'nms 300': lambda: hn.nms(B, dec, 0.35, IOU, MAX_DET, *o100, ws, st),
                'nms all': lambda: hn.nms(B, dec, 0.0, IOU, MAX_DET, *o100, ws, st),
                'nms all, max_det = A': lambda: hn.nms(B, dec, 0.0, IOU, A, *oA, ws, st)}
        # the results first: the kernels against the oracle on the first image
        legs['decode']()
        host = dec[:1].cpu()
        for name, conf, o in (('nms 300', 0.35, o100), ('nms all, max_det = A', 0.0, oA)):
            legs[name]()
            torch.cuda.synchronize()
            want = o_nms(host, C, conf, IOU)[0][1][:o[1].shape[1]]
            kept = int(o[2][0])
            assert kept == len(want) and np.array_equal(o[1][0, :kept].cpu().numpy(), want), (R, B, name)
            if name == 'nms 300':
                cand = int((host[0, :, 4] * host[0, :, 5:].max(1).values >= 0.35).sum())
        if model is not None:
            x, xr, xp = (t.cuda().to(torch.bfloat16) for t in make_inputs(B, 9, resolution=R, pc_channels=5))
            with torch.no_grad():
                model(x, xr, xp)
                model.forward_detect(x, xr, xp, 0.35, IOU, MAX_DET)

            def fwd():
                with torch.no_grad():
                    model(x, xr, xp)

            def det():
                with torch.no_grad():
                    model.forward_detect(x, xr, xp, 0.35, IOU, MAX_DET)
            legs['forward'], legs['detect'] = fwd, det
        iters = {k: iters_for(fn) for k, fn in legs.items()}
        res = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                res[k].append(timed_events(fn, iters[k]))
        say(f'\nR = {R} ({A} anchors, {"nms_kernel, one launch" if A <= 4096 else "wide path, two launches"}), B = {B}: {cand} candidates at conf 0.35, {A} at conf 0, '
            f'{kept} kept of all')
        for k, v in res.items():
            table[(R, B, k)] = v
            say(f'  {k:<22} {statistics.median(v):9.4f}  [{min(v):9.4f} .. {max(v):9.4f}]')
    del model
    torch.cuda.empty_cache()

if 416 in a.res and 448 in a.res:
    say('\nwide path at 448 against nms_kernel at 416 (anchor ratio 4116 / 3549 = 1.160):')
    for B in a.batch:
        for k in ('nms 300', 'nms all'):
            w, y = table[(448, B, k)], table[(416, B, k)]
            say(f'  B = {B:<3} {k:<8} {statistics.median(w) / statistics.median(y):6.3f} x   (ratios of the rounds: {min(p / q for p, q in zip(w, y)):.3f} .. {max(p / q for p, q in zip(w, y)):.3f})')
if not a.no_forward:
    say('\ndecode + NMS (300 candidates) as a share of the forward of the same batch:')
    for R in a.res:
        for B in batches(R):
            d, n, f = (statistics.median(table[(R, B, k)]) for k in ('decode', 'nms 300', 'forward'))
            say(f'  R = {R}, B = {B:<3} {(d + n):8.4f} ms of {f:8.4f} ms = {100 * (d + n) / f:5.1f} %')

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
