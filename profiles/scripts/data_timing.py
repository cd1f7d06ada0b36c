"""Time of assembling one training batch on the GPU (achelous_amd/data.py) against the other ways to the same tensors.
Workload: B seeded 1080 x 1920 frames with both label maps to R = 320, bf16 images, uint8 label maps.
  A0  the three launches alone (arenas and tables already on the device)      A1  + building and uploading the frame / coefficient / index tables (one small copy)
  A2  the whole `TrainBatcher` call from host arrays: packing into pinned memory, three uploads, launches (host clock, ends synchronised)
  a   what the package offered before, frames already on the device: `prepost.resize_image` + `preprocess_input` per frame, labels by torch indexing per frame
  b   the host path: PIL per frame, single process (tests/data_cases.py::pil_frame), without any upload
  c   the pinned upload of the raw frames and label maps alone (the price of resizing on the device: the host path would upload ~10 MB instead)
Device events around synchronised work (host clock for A2, b), warm-up, >= 0.5 s of timed work per leg and round, legs alternated in one process, median and spread of
the rounds.  Before anything is timed the bytes of A, a and b are compared.  `--profile`: only leg A0, a few times, for `rocprofv3 --kernel-trace --stats`.
usage: python profiles/scripts/data_timing.py [--batch 32] [--rounds 5] [--out FILE] [--profile]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
import data_cases as DC                                  # noqa: E402
from achelous_amd import data as D                       # noqa: E402
from achelous_amd import prepost                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--profile', action='store_true')
a = ap.parse_args()
B, R, H, W, NSEG = a.batch, 320, 1080, 1920, 9
lines = []


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


def timed_host(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def iters_for(fn, timer, target_ms=500.0, cap=5000):
    fn()
    one = timer(fn, 2)
    return max(1, min(cap, int(target_ms / max(one, 1e-3))))


rng = np.random.default_rng(0)
images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
png = [rng.integers(0, NSEG + 3, (H, W)).astype(np.uint8) for _ in range(B)]
png_w = [rng.integers(0, 4, (H, W)).astype(np.uint8) for _ in range(B)]
frames = [dict(image=i, png=p, png_w=w, boxes=[(100, 100, 400, 300, 1)]) for i, p, w in zip(images, png, png_w)]
place = [D.default_placement(W, H, R)] * B
nw, nh, dx, dy = place[0]

arena = D.pack_arena(images, 3, 'cuda', 'images')
la, law = D._pack_label_arena(png, png_w, 'cuda')
meta = D._Meta(arena.data.device, 'timing')
iref, mid_bytes = D._plan_images(meta, arena, place, R)
lref = D._plan_labels(meta, la, law, place, R)
lut = meta.add(D.value_table())
meta.commit()


def leg_a0():
    return D._launch_images(meta, arena, iref, mid_bytes, lut, R, torch.bfloat16), D._launch_labels(meta, la.data, lref, B, R, NSEG, torch.uint8)


def leg_a0_images():
    return D._launch_images(meta, arena, iref, mid_bytes, lut, R, torch.bfloat16)


def leg_a0_labels():
    return D._launch_labels(meta, la.data, lref, B, R, NSEG, torch.uint8)


if a.profile:
    for _ in range(20):
        leg_a0()
    torch.cuda.synchronize()
    sys.exit(0)


def leg_a1():
    return D.letterbox_batch(arena, R, place, torch.bfloat16), D.labels_batch(la, law, R, NSEG, place)


batcher = D.TrainBatcher(R, NSEG, dtype=torch.bfloat16, device='cuda')


def leg_a2():
    out = batcher(frames)
    torch.cuda.synchronize()                             # one batch at a time: the pinned buffers are reused, not multiplied
    return out


dev_images = [arena.data[o:o + h * p].view(h, w, 3) for o, h, w, p in arena.frames]
dev_png = [la.data[o:o + h * p].view(h, w) for o, h, w, p in la.frames]
dev_png_w = [law.data[o:o + h * p].view(h, w) for o, h, w, p in law.frames]
yi = torch.from_numpy(DC.nearest_index(H, nh)).cuda()
xi = torch.from_numpy(DC.nearest_index(W, nw)).cuda()


def leg_a_images():
    return prepost.preprocess_input(torch.stack([prepost.resize_image(im, (R, R)) for im in dev_images]), torch.bfloat16)


def leg_a_labels():
    out = torch.zeros(2, B, R, R, dtype=torch.uint8, device='cuda')
    for b in range(B):
        out[0, b, dy:dy + nh, dx:dx + nw] = dev_png[b][yi][:, xi].clamp(max=NSEG)
        out[1, b, dy:dy + nh, dx:dx + nw] = dev_png_w[b][yi][:, xi].clamp(max=2)
    return out


def leg_a():
    return leg_a_images(), leg_a_labels()


have_pil = True
try:
    import PIL  # noqa: F401
except ImportError:
    have_pil = False


def leg_b():
    return [DC.pil_frame(i, p, w, R, NSEG) for i, p, w in zip(images, png, png_w)]


def leg_c():
    D.pack_arena(images, 3, 'cuda', 'images')
    D._pack_label_arena(png, png_w, 'cuda')
    torch.cuda.synchronize()


pin_img = torch.empty(arena.data.numel(), dtype=torch.uint8, pin_memory=True)
pin_lab = torch.empty(la.data.numel(), dtype=torch.uint8, pin_memory=True)
dst_img, dst_lab = torch.empty_like(arena.data), torch.empty_like(la.data)


def leg_c_copy():
    dst_img.copy_(pin_img, non_blocking=True)
    dst_lab.copy_(pin_lab, non_blocking=True)


# ---- every leg computes the same bytes
u8 = D.letterbox_batch(arena, R, place, torch.uint8)
old = torch.stack([prepost.resize_image(im, (R, R)) for im in dev_images])
assert torch.equal(u8, old), 'batched bytes differ from prepost.resize_image'
(img0, (p0, w0)) = leg_a0()
(img1, (p1, w1)) = leg_a1()
out2 = leg_a2()
assert torch.equal(img0, img1) and torch.equal(img0, out2.images) and torch.equal(p0, p1) and torch.equal(p0, out2.png) and torch.equal(w0, w1) and torch.equal(w0, out2.png_w)
lab_old = leg_a_labels()
assert torch.equal(lab_old[0], p0) and torch.equal(lab_old[1], w0), 'labels differ from the torch composite'
if have_pil:
    host = leg_b()
    assert all(np.array_equal(u8[b].cpu().numpy(), host[b][0]) for b in range(B)), 'batched bytes differ from PIL'
    assert all(np.array_equal(p0[b].cpu().numpy(), host[b][2]) and np.array_equal(w0[b].cpu().numpy(), host[b][3]) for b in range(B))
    lutf = torch.from_numpy(np.stack([h[1] for h in host])).to(torch.bfloat16).cuda()
    assert torch.equal(lutf, img0), 'bf16 images differ from the PIL path rounded once'

legs = [('A0 three launches, everything resident', leg_a0, timed_events),
        ('A0i  of which the two image launches', leg_a0_images, timed_events),
        ('A0l  of which the label launch', leg_a0_labels, timed_events),
        ('A1 + tables built and uploaded per call', leg_a1, timed_events),
        ('A2 TrainBatcher from host arrays (pack + 3 uploads + launches)', leg_a2, timed_host),
        ('a  per-image resize_image + preprocess_input, torch labels', leg_a, timed_events),
        ('ai  of which images', leg_a_images, timed_events),
        ('al  of which labels', leg_a_labels, timed_events),
        ('c  pack into pinned memory + upload of frames and label maps', leg_c, timed_host),
        ('cc  of which the two pinned copies alone', leg_c_copy, timed_events)]
if have_pil:
    legs.append(('b  PIL on the host, single process, no upload', leg_b, timed_host))
its = {name: iters_for(fn, timer) for name, fn, timer in legs}
res = {name: [] for name, _, _ in legs}
for _ in range(a.rounds):
    for name, fn, timer in legs:
        res[name].append(timer(fn, its[name]))
raw_mb = (arena.data.numel() + la.data.numel()) / 1e6
say(f'profiles/scripts/data_timing.py on one MI355X (device events / a host clock around synchronised work, warm-up, >= 0.5 s of timed work per leg and round, legs alternated in one '
    f'process; ms per batch, median of {a.rounds} rounds, min .. max)')
say()
say(f'batch {B}: 1080 x 1920 frames with both label maps ({raw_mb:.1f} MB of source bytes) to R = {R}, bf16 images [B, 3, R, R], uint8 label maps; placement {place[0]}')
say('(A, a and b give the same bytes: uint8 canvases, label maps, and the bf16 images are the PIL path rounded once)' if have_pil else
    '(A and a give the same bytes; PIL is missing on this machine: leg b skipped)')
med = {}
for name, _, _ in legs:
    v = res[name]
    med[name] = statistics.median(v)
    say(f'  {name:<66}: {med[name]:9.3f}  ({min(v):.3f} .. {max(v):.3f}; {its[name]} calls per round)')
k = [n for n, _, _ in legs]
say()
say(f'  a / A0 = {med[k[5]] / med[k[0]]:.2f}   a / A1 = {med[k[5]] / med[k[3]]:.2f}   images ai / A0i = {med[k[6]] / med[k[1]]:.2f}   labels al / A0l = {med[k[7]] / med[k[2]]:.2f}')
if have_pil:
    say(f'  b / A2 = {med[k[10]] / med[k[4]]:.2f} (host path without its upload against the whole device path with its uploads)')
say(f'  upload: {raw_mb:.1f} MB in {med[k[9]]:.3f} ms = {raw_mb / med[k[9]]:.1f} GB/s pinned copy; with the host-side packing {med[k[8]]:.3f} ms')
img_bytes = B * (H * W * 3 + 2 * H * 3 * R + 3 * R * R * 2) / 1e6
say(f'  image launches move {img_bytes:.1f} MB compulsory (source + intermediate written and read + output): {img_bytes / med[k[1]] / 1e3:.2f} TB/s by call time, '
    f'{img_bytes / med[k[1]] / 1e3 / 8 * 100:.0f} % of the 8 TB/s HBM peak')
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
