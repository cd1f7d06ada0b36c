"""Time of the serving path's post-processing for a batch (achelous_amd/prepost.py seg_maps_frames, csrc/k_serve.h) against the other ways to the same bytes.
Workload: B seeded 1080 x 1920 frames, R = 320, 9 semantic classes, bf16 network outputs (seeded normal logits).
  a   the new launch, class maps only (two softmax launches + ONE launch for all frames and both heads; tables resident)
  b   the new launch, class maps + overlay image
  a1  `seg_maps_frames` as a caller uses it: a + building and uploading the frame table per call
  c   the shipped path for the same class maps: `ach_seg_resize_argmax` per head (all frames share a shape here, so two calls: softmax + one thread per output pixel)
  d   c + the palette / blend / brightness arithmetic as torch ops: the overlay a user would write today
  e   for scale: forward + decode + NMS of the same batch (`forward_detect`, bf16)
and a mixed batch, 16 frames each of 1080 x 1920 and 720 x 1280: the new path (class maps + boxes: one launch each behind the softmax) against a Python loop of
`detect_frame`'s post-processing (per frame `correct_boxes_device` and `seg_class_map_original` twice).
Device events around the calls, warm-up, >= 0.5 s of timed work per leg and round, legs alternated in one process, median and spread of the rounds.  Before anything is
timed the bytes of the legs are compared.  `--profile`: only legs a and b, a few times, for `rocprofv3 --kernel-trace --stats`.
usage: python profiles/scripts/serve_timing.py [--batch 32] [--rounds 5] [--out FILE] [--profile] [--no-forward]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO]
from achelous_amd import data as D                       # noqa: E402
from achelous_amd import prepost as P                    # noqa: E402
from achelous_amd.postprocess import _handle, correct_boxes_device   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--profile', action='store_true')
ap.add_argument('--no-forward', action='store_true')
a = ap.parse_args()
B, R, H, W, C = a.batch, 320, 1080, 1920, 9
DT = torch.bfloat16
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


def iters_for(fn, target_ms=500.0, cap=5000):
    fn()
    one = timed_events(fn, 2)
    return max(1, min(cap, int(target_ms / max(one, 1e-3))))


assert torch.cuda.is_available(), 'serve_timing.py measures on the GPU; there is nothing to fall back to'
gen = torch.Generator().manual_seed(0)
se = torch.randn(B, C, R, R, generator=gen).to(DT).cuda()
lane = torch.randn(B, 2, R, R, generator=gen).to(DT).cuda()
rng = np.random.default_rng(0)
one = rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
images = [one[b % 4] for b in range(B)]
shapes = [(H, W)] * B
arena = D.pack_arena(images, 3, 'cuda', 'images')
run_a = P._seg_maps_plan(se, lane, shapes, None, meta_name='timing_a')
run_b = P._seg_maps_plan(se, lane, shapes, arena, meta_name='timing_b')
hnd = _handle(1, R, DT)
ws = torch.empty(B * C * R * R, dtype=torch.float32, device='cuda')
c_sem = torch.empty(B, H, W, dtype=torch.uint8, device='cuda')
c_line = torch.empty(B, H, W, dtype=torch.uint8, device='cuda')
stream = torch.cuda.current_stream().cuda_stream


def leg_a():
    return run_a()


def leg_b():
    return run_b()


def leg_a1():
    return P.seg_maps_frames(se, lane, shapes, None)


def leg_c():
    hnd.seg_resize_argmax(B, C, se, H, W, ws, c_sem, stream)
    hnd.seg_resize_argmax(B, 2, lane, H, W, ws, c_line, stream)
    return c_sem, c_line


pal_se = torch.tensor(P.PALETTE_SEG, dtype=torch.float32, device='cuda')
pal_line = torch.tensor(P.PALETTE_LINE, dtype=torch.float32, device='cuda')
lut = torch.from_numpy(P.brightness_table(1.3)).cuda()
dev_images = torch.stack([arena.data[o:o + h * p].view(h, w, 3) for o, h, w, p in arena.frames])


def leg_d():
    sem, line = leg_c()
    img = dev_images.float()
    o1 = (img + 0.45 * (pal_se[sem.long()] - img)).trunc()
    o2 = (o1 + 0.3 * (pal_line[line.long()] - o1)).trunc()
    return lut[o2.long()]


if a.profile:
    for _ in range(10):
        leg_a()
        leg_b()
    torch.cuda.synchronize()
    sys.exit(0)

# ---- every leg computes the same bytes
ra, rb = leg_a(), leg_b()
sem_c, line_c = leg_c()
for b in range(B):
    assert torch.equal(ra['semantic'][b], sem_c[b]) and torch.equal(ra['waterline'][b], line_c[b]), 'class maps differ from ach_seg_resize_argmax'
    assert torch.equal(rb['semantic'][b], sem_c[b]) and torch.equal(rb['waterline'][b], line_c[b])
ovl_d = leg_d()
ovl_diff = sum(int((rb['overlay'][b] != ovl_d[b]).sum()) for b in range(B))
del ovl_d
try:
    from PIL import Image, ImageEnhance
    img0 = Image.fromarray(images[0])
    s_img = Image.fromarray(np.array(P.PALETTE_SEG, np.uint8)[sem_c[0].cpu().numpy()])
    l_img = Image.fromarray(np.array(P.PALETTE_LINE, np.uint8)[line_c[0].cpu().numpy()])
    pil = np.array(ImageEnhance.Brightness(Image.blend(Image.blend(img0, s_img, 0.45), l_img, 0.3)).enhance(1.3))
    pil_note = f"frame 0 of the overlay against PIL Image.blend / ImageEnhance.Brightness: {int((rb['overlay'][0].cpu().numpy() != pil).sum())} differing bytes"
except ImportError:
    pil_note = 'PIL is missing on this machine: the overlay is compared with the torch-op statement only'

legs = [('a  new launch, class maps only (tables resident)', leg_a), ('b  new launch, class maps + overlay', leg_b),
        ('a1 seg_maps_frames as called: a + table built and uploaded', leg_a1), ('c  shipped: ach_seg_resize_argmax per head (two calls)', leg_c),
        ('d  c + palette / blend / brightness as torch ops', leg_d)]
if not a.no_forward:
    from achelous_amd import Achelous
    from achelous_amd.synth import condition_state_dict, make_inputs
    kw = dict(num_det=7, num_seg=C, phi='S0', resolution=R, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
    net = Achelous(**kw).eval()
    net.load_state_dict(condition_state_dict(net.state_dict(), seed=0))
    net = net.cuda()
    x, xr, xp = (t.to(DT).cuda() for t in make_inputs(B, 1234, resolution=R, pc_channels=5))

    def leg_e():
        return net.forward_detect(x, xr, xp, 0.35, 0.35, 100)
    legs.append(('e  for scale: forward + decode + NMS of the batch (bf16)', leg_e))

# ---- the mixed batch: 16 x 1080p + 16 x 720p
mshapes = [(1080, 1920)] * 16 + [(720, 1280)] * 16
mse, mlane = se[:32] if B >= 32 else se.repeat(32 // B + 1, 1, 1, 1)[:32], lane[:32] if B >= 32 else lane.repeat(32 // B + 1, 1, 1, 1)[:32]
mrows = torch.rand(32, 100, 7, generator=gen).cuda()
mrows[..., 2:4] = mrows[..., 0:2] + 0.1
mcnt = torch.full((32,), 60, dtype=torch.int32, device='cuda')


def leg_mixed_new():
    return P.seg_maps_frames(mse, mlane, mshapes, None), P.correct_boxes_frames(mrows, mcnt, (R, R), mshapes, True)


def leg_mixed_loop():
    out = []
    for b, sh in enumerate(mshapes):
        out.append((correct_boxes_device(mrows[b:b + 1], mcnt[b:b + 1], (R, R), sh, True), P.seg_class_map_original(mse[b:b + 1], sh), P.seg_class_map_original(mlane[b:b + 1], sh)))
    return out


(mm, mb), ml = leg_mixed_new(), leg_mixed_loop()
for b in range(32):
    assert torch.equal(mb[b:b + 1], ml[b][0]) and torch.equal(mm['semantic'][b], ml[b][1][0]) and torch.equal(mm['waterline'][b], ml[b][2][0]), 'mixed batch differs from the loop'
del mm, mb, ml
legs += [('m  mixed batch (16 x 1080p + 16 x 720p): class maps + boxes, new path', leg_mixed_new), ('ml mixed batch: Python loop of the per-frame path', leg_mixed_loop)]

its = {name: iters_for(fn) for name, fn in legs}
res = {name: [] for name, _ in legs}
for _ in range(a.rounds):
    for name, fn in legs:
        res[name].append(timed_events(fn, its[name]))
say(f'profiles/scripts/serve_timing.py on one MI355X (device events, warm-up, >= 0.5 s of timed work per leg and round, legs alternated in one process; ms per batch, median of '
    f'{a.rounds} rounds, min .. max)')
say()
say(f'batch {B}: {H} x {W} frames, R = {R}, {C} semantic + 2 water-line classes, bf16 network outputs; every leg includes the softmax launches')
say(f'(a, b and c give the same class maps, asserted; overlay of b against the torch-op statement d: {ovl_diff} differing bytes; {pil_note})')
med = {}
for name, _ in legs:
    v = res[name]
    med[name] = statistics.median(v)
    say(f'  {name:<72}: {med[name]:9.3f}  ({min(v):.3f} .. {max(v):.3f}; {its[name]} calls per round)')
k = [n for n, _ in legs]
spread = max((max(res[n]) - min(res[n])) / med[n] for n in (k[0], k[3]))
say()
say(f'  c / a = {med[k[3]] / med[k[0]]:.2f}   d / b = {med[k[4]] / med[k[1]]:.2f}   run-to-run spread of a and c: {spread * 100:.1f} % of the median')
if not a.no_forward:
    say(f'  a / e = {med[k[0]] / med[k[5]]:.2f}   b / e = {med[k[1]] / med[k[5]]:.2f}   c / e = {med[k[3]] / med[k[5]]:.2f} (post-processing against the forward + decode + NMS it follows)')
say(f'  mixed batch: loop / new = {med[k[-1]] / med[k[-2]]:.2f}')
# compulsory bytes: outputs written, the image read; the probabilities (B * 11 * R * R * 4 bytes) stay in the caches and are counted once, as written and read
prob = B * (C + 2) * R * R * 4 * 2 + B * (C + 2) * R * R * 2
bytes_a = (2 * B * H * W + prob) / 1e6
bytes_b = (2 * B * H * W + 2 * 3 * B * H * W + prob) / 1e6
say(f'  compulsory bytes (outputs written + image read + logits read, probabilities written and read once): a {bytes_a:.1f} MB -> {bytes_a / med[k[0]] / 1e3:.2f} TB/s by call time, '
    f'{bytes_a / med[k[0]] / 1e3 / 8 * 100:.0f} % of the 8 TB/s HBM peak; b {bytes_b:.1f} MB -> {bytes_b / med[k[1]] / 1e3:.2f} TB/s, {bytes_b / med[k[1]] / 1e3 / 8 * 100:.0f} %')
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
