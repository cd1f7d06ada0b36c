"""Time of drawing the kept detections on a served batch (achelous_amd/prepost.py draw_detections_frames, csrc/k_draw.h) against the host way to the same bytes.
Workload: B seeded 1080 x 1920 overlays in one packed arena, N detections per frame for N in 0, 5, 100 (seeded boxes all over the frame, 7 class names, the
reference's thickness 9 and font size 32).
  a   the two new launches alone (`ach_draw_detections_frames`, tables resident)
  a1  `draw_detections_frames` as a caller uses it: a + building and uploading the frame table per call
  b   the same drawing with PIL on the host: download every overlay, ImageDraw per frame (tests/draw_cases.py draw_pil), upload again
  c   for scale: the overlay launch (`seg_maps_frames`, two softmax launches + one launch), whose code this change does not touch
Device events around the calls (b: a host clock around work that ends in a synchronise), warm-up, >= 0.3 s of timed work per leg and round, legs alternated in one
process, median and spread of the rounds.  Before anything is timed, leg a's bytes are compared with leg b's on the first frames.
`--lib PATH`: a library built with another tile shape (hipcc ... -DACH_DRAW_TX=16 | 32 | 64 on csrc/api_frames.cpp: 64 x 16, 128 x 8, 256 x 4 pixels; default 8: 32 x 32);
name the file after its tile, the name is the leg's label.
Needs PIL with FreeType.  usage: python profiles/scripts/draw_timing.py [--batch 64] [--rounds 5] [--out FILE] [--lib PATH ...]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
from achelous_amd import data as D                       # noqa: E402
from achelous_amd import prepost as P                    # noqa: E402
from achelous_amd.engine import NativeLibrary, hip_library   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--lib', action='append', default=[])
ap.add_argument('--host-frames', type=int, default=8, help='frames the PIL leg draws per round (its time is scaled to the batch)')
a = ap.parse_args()
B, R, H, W, NC = a.batch, 320, 1080, 1920, 7
NAMES = tuple(f'class{i}' for i in range(NC))
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


def iters_for(fn, target_ms=300.0, cap=2000):
    fn()
    one = timed_events(fn, 2)
    return max(1, min(cap, int(target_ms / max(one, 1e-3))))


def rows_for(n, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((B, max(n, 1), 7), np.float32)
    cy, cx = rng.uniform(0, H, (B, n)), rng.uniform(0, W, (B, n))
    hh, ww = rng.uniform(20, 400, (B, n)), rng.uniform(20, 500, (B, n))
    out[:, :n] = np.stack([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2, rng.uniform(0.3, 1, (B, n)), rng.uniform(0.3, 1, (B, n)),
                           rng.integers(0, NC, (B, n)).astype(np.float64)], axis=2)
    return out


assert torch.cuda.is_available(), 'this script measures on the GPU'
dev = torch.device('cuda')
style = P.DrawStyle(NAMES)
shapes = [(H, W)] * B
layout = P.frames_layout(shapes)
offs, pitches, nbytes = layout[3], layout[4], layout[5]
rng = np.random.default_rng(1)
clean = torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8)).to(dev)
arena = clean.clone()
thick, size = style.thickness_for(0, H, W, (R, R)), style.font_size_for(H)
say(f'{B} frames of {H} x {W}, thickness {thick}, font size {size}, {NC} classes; device {torch.cuda.get_device_name(0)}')


def raw_call(lib, boxes, count, max_det):
    """leg a: everything host-side done once, the call itself only enqueues the two launches"""
    labels_host, labels_dev, blob_dev, base, blob_bytes = P._device_atlases(style, (size,), dev)
    table = np.zeros((B, P.DRAW_TABLE_COLS), np.int64)
    for b in range(B):
        table[b, :6] = (offs[b], H, W, pitches[b], thick, base[size])
    tdev, sdev = torch.from_numpy(table).to(dev), torch.from_numpy(style.bytes).to(dev)
    recs = torch.empty(B * max_det * P.DRAW_REC, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        rc = lib.lib.ach_draw_detections_frames(arena.data_ptr(), arena.numel(), table.ctypes.data, tdev.data_ptr(), B, boxes.data_ptr(), count.data_ptr(), max_det, NC,
                                                labels_host.ctypes.data, labels_dev.data_ptr(), len(labels_host), blob_dev.data_ptr(), blob_bytes, sdev.data_ptr(),
                                                recs.data_ptr(), None, stream)
        assert rc == 0, lib.lib.ach_last_error(None)
    fn.keep = (tdev, sdev, recs, table)
    return fn


def pil_leg(rows, n, frames):
    import draw_cases as DC
    from PIL import ImageFont
    font = ImageFont.load_default(size)
    colors = [tuple(int(v) for v in c) for c in style.colors]
    views = [torch.as_strided(arena, (H, W, 3), (pitches[b], 3, 1), offs[b]) for b in range(frames)]

    def fn():
        for b, v in enumerate(views):
            img = v.cpu().numpy()
            v.copy_(torch.from_numpy(DC.draw_pil(img, rows[b, :n], font, thick, names=NAMES, colors=colors, skip_ids=())))
        torch.cuda.synchronize()
    return fn


def overlay_leg():
    g = torch.Generator().manual_seed(3)
    se = torch.randn(B, 9, R, R, generator=g).to(dev).to(torch.bfloat16)
    lane = torch.randn(B, 2, R, R, generator=g).to(dev).to(torch.bfloat16)
    images = D.Arena(clean, [(offs[b], H, W, pitches[b]) for b in range(B)])
    return P._seg_maps_plan(se, lane, shapes, images, want=('overlay',), meta_name='draw_timing')


libs = [('32 x 32 (shipped)', hip_library())] + [(os.path.basename(p), NativeLibrary(p)) for p in a.lib]
overlay = overlay_leg()
for n in (0, 5, 100):
    rows = rows_for(n, 10 + n)
    boxes, count = torch.from_numpy(rows).to(dev), torch.full((B,), n, dtype=torch.int32, device=dev)
    max_det = rows.shape[1]
    legs = {f'a  two launches, tile {name}': raw_call(lib, boxes, count, max_det) for name, lib in libs}
    legs['a1 draw_detections_frames (tables built and uploaded per call)'] = lambda: P.draw_detections_frames(arena, layout, boxes, count, shapes, style, (R, R))
    # the bytes first: the kernels against PIL on the first frames
    check = min(2, B)
    arena.copy_(clean)
    next(iter(legs.values()))()
    got = [torch.as_strided(arena, (H, W, 3), (pitches[b], 3, 1), offs[b]).cpu().numpy() for b in range(check)]
    arena.copy_(clean)
    pil_leg(rows, n, check)()
    same = all(np.array_equal(got[b], torch.as_strided(arena, (H, W, 3), (pitches[b], 3, 1), offs[b]).cpu().numpy()) for b in range(check))
    drawn = sum(int((got[b] != torch.as_strided(clean, (H, W, 3), (pitches[b], 3, 1), offs[b]).cpu().numpy()).any(axis=2).sum()) for b in range(check)) / check
    say(f'\n{n} detections per frame: kernels == PIL on the first {check} frames: {same}; {drawn:.0f} pixels drawn per frame')
    assert same
    host = pil_leg(rows, n, min(a.host_frames, B))
    iters = {k: iters_for(fn) for k, fn in legs.items()}
    it_c = iters_for(overlay)
    host()
    res = {k: [] for k in list(legs) + ['b', 'c']}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            res[k].append(timed_events(fn, iters[k]))
        t0 = time.perf_counter()
        host()
        res['b'].append((time.perf_counter() - t0) * 1e3 * B / min(a.host_frames, B))
        res['c'].append(timed_events(overlay, it_c))
    names = dict({k: k for k in legs}, b=f'b  PIL on the host, download + draw + upload ({min(a.host_frames, B)} frames timed, scaled to {B})',
                 c='c  for scale: seg_maps_frames overlay launch (2 softmax + 1 launch)')
    for k, v in res.items():
        say(f'  {names[k]:<78} median {statistics.median(v):9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}   ({a.rounds} rounds)')

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
