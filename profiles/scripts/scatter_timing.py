"""Time of painting the radar point classes on a served batch (achelous_amd/prepost.py scatter_points_frames, csrc/k_scatter.h) against the host way to the same bytes.
Workload: B seeded 1080 x 1920 overlays in one packed arena, one float32 cloud of 6000 rows per frame (u, v all over the frame, rcs in [0, 400): discs of up to 20
pixels across), N rows of it sampled with replacement for N in 512, 4096, 9 classes, the default style (viridis, alpha 0.98, size_scale 1, max_radius 64).
  a   the two new launches alone (`ach_scatter_points_frames`, tables resident)
  a1  `scatter_points_frames` as a caller uses it: a + building and uploading the frame table, the colours and the indices per call
  b   the same on the host: download every overlay, np.unique, per row the float64 coverage on the disc's bounding box and a PIL Image.blend under its mask (the oracle
      of tests/scatter_cases.py restricted to the box, which gives the same bytes), upload again
  c   for scale: the overlay launch (`seg_maps_frames`, two softmax launches + one launch), whose code this change does not touch
Device events around the calls (b: a host clock around work that ends in a synchronise), warm-up, >= 0.3 s of timed work per leg and round, legs alternated in one
process, median and spread of the rounds.  Before anything is timed, leg a's rows and bytes are compared with leg b's on the first frame.
  r   leg a on frames declared 1 x 1: one tile per frame, so in effect launch 1 (gather, sort, unique, records) alone
`--lib PATH`: a library built with another tile height (hipcc ... -DACH_SCATTER_RY=1 | 4 on csrc/api_frames.cpp: 64 x 16, 64 x 64 pixels; default 2: 64 x 32); name the
file after its tile, the name is the leg's label.
usage: python profiles/scripts/scatter_timing.py [--batch 64] [--rounds 5] [--out FILE] [--lib PATH ...]"""
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
import scatter_cases as SC                               # noqa: E402
from achelous_amd import data as D                       # noqa: E402
from achelous_amd import prepost as P                    # noqa: E402
from achelous_amd.engine import NativeLibrary, hip_library   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--lib', action='append', default=[])
ap.add_argument('--host-frames', type=int, default=1, help='frames the host leg paints per round (its time is scaled to the batch)')
a = ap.parse_args()
B, R, H, W, NC, ROWS = a.batch, 320, 1080, 1920, 9, 6000
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


assert torch.cuda.is_available(), 'this script measures on the GPU'
dev = torch.device('cuda')
style = P.ScatterStyle()
shapes = [(H, W)] * B
layout = P.frames_layout(shapes)
offs, pitches, nbytes = layout[3], layout[4], layout[5]
rng = np.random.default_rng(1)
clean = torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8)).to(dev)
arena = clean.clone()
clouds_host = []
for b in range(B):
    c = rng.uniform(0, 100, (ROWS, 5)).astype(np.float32)
    c[:, 2], c[:, 3], c[:, 4] = rng.integers(0, 1600, ROWS) / 4.0, rng.integers(0, 8 * W, ROWS) / 8.0, rng.integers(0, 8 * H, ROWS) / 8.0
    clouds_host.append(c)
clouds = D.pack_clouds(clouds_host, dev, 'scatter_timing')
say(f'{B} frames of {H} x {W}, {ROWS} cloud rows per frame, {NC} classes, alpha {style.alpha}, size_scale {style.size_scale}, max_radius {style.max_radius}; '
    f'device {torch.cuda.get_device_name(0)}')


def raw_call(lib, idx, cls, N, tiny=False):
    """leg a: everything host-side done once, the call itself only enqueues the two launches; tiny: the frames are declared 1 x 1"""
    table = np.zeros((B, P.SCATTER_TABLE_COLS), np.int64)
    for b, fr in enumerate(clouds.frames):
        table[b, :11] = (offs[b], 1 if tiny else H, 1 if tiny else W, pitches[b]) + tuple(fr) + (3, 4, 2)
    tdev, cdev, idev = torch.from_numpy(table).to(dev), torch.from_numpy(style.cmap.copy()).to(dev), torch.from_numpy(idx).to(dev)
    out = dict(rows=torch.empty(B, N, 4, dtype=torch.float64, device=dev), count=torch.empty(B, dtype=torch.int32, device=dev),
               range=torch.empty(B, 2, dtype=torch.int32, device=dev), discs=torch.empty(B * N * 4, dtype=torch.float64, device=dev),
               boxes=torch.empty(B * N * 4, dtype=torch.int32, device=dev))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        rc = lib.lib.ach_scatter_points_frames(arena.data_ptr(), arena.numel(), table.ctypes.data, tdev.data_ptr(), B, clouds.data.data_ptr(), clouds.data.numel(), 0,
                                               idev.data_ptr(), cls.data_ptr(), N, NC, cdev.data_ptr(), 0, 0, 0, style.alpha, style.k, style.max_radius,
                                               out['rows'].data_ptr(), out['count'].data_ptr(), out['range'].data_ptr(), out['discs'].data_ptr(), B * N * 32,
                                               out['boxes'].data_ptr(), B * N * 16, stream)
        assert rc == 0, lib.lib.ach_last_error(None)
    fn.keep, fn.out = (tdev, cdev, idev, table), out
    return fn


def host_paint(img, rows, colours):
    """the oracle of tests/scatter_cases.py on every disc's bounding box: the same coverage expression and the same PIL blend, so the same bytes"""
    from PIL import Image
    k, mr = style.k, float(style.max_radius)
    for (u, v, s, _), col in zip(rows, colours):
        if not s > 0:
            continue
        rad = int(np.sqrt(min(k * s, mr * mr))) + 2
        x0, x1, y0, y1 = max(0, int(np.floor(u)) - rad), min(W, int(np.floor(u)) + rad + 2), max(0, int(np.floor(v)) - rad), min(H, int(np.floor(v)) + rad + 2)
        if x1 <= x0 or y1 <= y0:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float64)
        dx, dy = xx - u, yy - v
        m = dx * dx + dy * dy <= min(k * s, mr * mr)
        if not m.any():
            continue
        crop = np.ascontiguousarray(img[y0:y1, x0:x1])
        blended = np.asarray(Image.blend(Image.fromarray(crop), Image.new('RGB', (x1 - x0, y1 - y0), tuple(int(c) for c in col)), style.alpha))
        crop[m] = blended[m]
        img[y0:y1, x0:x1] = crop
    return img


def host_leg(idx, cls_host, frames):
    views = [torch.as_strided(arena, (H, W, 3), (pitches[b], 3, 1), offs[b]) for b in range(frames)]
    kept = []

    def fn():
        kept.clear()
        for b, v in enumerate(views):
            img = v.cpu().numpy()
            rows = SC.unique_rows(SC.gather(clouds_host[b], idx[b], cls_host[b], NC, (2, 3, 4)))
            colours, _ = SC.row_colours(rows, style.cmap)
            v.copy_(torch.from_numpy(host_paint(img, rows, colours)))
            kept.append(rows)
        torch.cuda.synchronize()
    fn.rows = kept
    return fn


def overlay_leg():
    g = torch.Generator().manual_seed(3)
    se = torch.randn(B, 9, R, R, generator=g).to(dev).to(torch.bfloat16)
    lane = torch.randn(B, 2, R, R, generator=g).to(dev).to(torch.bfloat16)
    images = D.Arena(clean, [(offs[b], H, W, pitches[b]) for b in range(B)])
    return P._seg_maps_plan(se, lane, shapes, images, want=('overlay',), meta_name='scatter_timing')


libs = [('64 x 32 (shipped)', hip_library())] + [(os.path.basename(p), NativeLibrary(p)) for p in a.lib]
overlay = overlay_leg()
for N in (512, 4096):
    idx = rng.integers(0, ROWS, (B, N)).astype(np.int64)
    cls_host = rng.integers(0, NC, (B, N)).astype(np.int64)
    cls = torch.from_numpy(cls_host).to(dev)
    legs = {f'a  two launches, tile {name}': raw_call(lib, idx, cls, N) for name, lib in libs}
    legs['r  launch 1 in effect: the shipped library on frames declared 1 x 1'] = raw_call(hip_library(), idx, cls, N, tiny=True)
    legs['a1 scatter_points_frames (table, colours and indices built and uploaded per call)'] = lambda: P.scatter_points_frames(arena, layout, shapes, clouds, cls, NC, style, idx)
    # the rows and the bytes first: the kernels against the host on the first frame
    first = next(iter(legs.values()))
    arena.copy_(clean)
    first()
    got = torch.as_strided(arena, (H, W, 3), (pitches[0], 3, 1), offs[0]).cpu().numpy()
    n0 = int(first.out['count'][0])
    got_rows = first.out['rows'][0, :n0].cpu().numpy()
    arena.copy_(clean)
    host = host_leg(idx, cls_host, 1)
    host()
    want = torch.as_strided(arena, (H, W, 3), (pitches[0], 3, 1), offs[0]).cpu().numpy()
    same = np.array_equal(got, want) and np.array_equal(got_rows, host.rows[0])
    painted = int((got != torch.as_strided(clean, (H, W, 3), (pitches[0], 3, 1), offs[0]).cpu().numpy()).any(axis=2).sum())
    say(f'\n{N} points per frame: kernels == host on the first frame (rows and bytes): {same}; {n0} unique rows, {painted} pixels painted')
    assert same
    host = host_leg(idx, cls_host, min(a.host_frames, B))
    iters = {k: iters_for(fn) for k, fn in legs.items()}
    it_c = iters_for(overlay)
    res = {k: [] for k in list(legs) + ['b', 'c']}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            res[k].append(timed_events(fn, iters[k]))
        t0 = time.perf_counter()
        host()
        res['b'].append((time.perf_counter() - t0) * 1e3 * B / min(a.host_frames, B))
        res['c'].append(timed_events(overlay, it_c))
    names = dict({k: k for k in legs}, b=f'b  numpy + PIL on the host, download + paint + upload ({min(a.host_frames, B)} frame timed, scaled to {B})',
                 c='c  for scale: seg_maps_frames overlay launch (2 softmax + 1 launch)')
    for k, v in res.items():
        say(f'  {names[k]:<86} median {statistics.median(v):9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}   ({a.rounds} rounds)')

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
