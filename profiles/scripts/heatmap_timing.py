"""Time of the heat-map mode on a served batch (achelous_amd/prepost.py heatmap_frames, csrc/k_heatmap.h) against the overlay launch on the same frames and against the
host way to the same bytes.  Workloads: 64 frames of 1080 x 1920, and a mixed batch of 16 x 1080p + 16 x 720p; seeded det maps at R = 320 with 7 classes (fp32), seeded
camera bytes in one packed arena, window 'full', alpha 0.5, an out arena of its own.
  a2  scores + mask + statistics (`ach_heatmap_frames` without colour outputs: two launches, tables resident)
  a3  all three launches (tables resident); a3 - a2 is the colour launch
  a   `heatmap_frames` as a caller uses it: a3 + building and uploading the frame table and allocating per call
  b   the host route the reference takes: download the det maps, numpy per frame (tests/heatmap_cases.py, the reference's arithmetic), upload the picture
  c   for scale: the overlay launch on the same frames (`seg_maps_frames`, two softmax launches + one launch), which also reads and writes 3 bytes per pixel
Device events around the calls (b: a host clock around work that ends in a synchronise), warm-up, >= 0.3 s of timed work per leg and round, legs alternated in one
process, median and spread of the rounds.  Before anything is timed, the kernels' mask, range and picture are compared with the restatement on the first frames.
The horizontal blends are NOT shared across output rows in k_heatmap.h (every pixel reads its four cells of each level from LDS); that variant was not tried.
The measurement runs in a child process under a time limit of its own.
usage: python profiles/scripts/heatmap_timing.py [--rounds 5] [--limit 540] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=None)
ap.add_argument('--limit', type=int, default=540, help='seconds the measuring child may take')
ap.add_argument('--host-frames', type=int, default=2, help='frames the host leg computes per round (its time is scaled to the batch)')
ap.add_argument('--child', action='store_true')
a = ap.parse_args()
if not a.child:
    cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', '--rounds', str(a.rounds), '--host-frames', str(a.host_frames)]
    sys.exit(subprocess.run(cmd + (['--out', a.out] if a.out else [])).returncode)

import numpy as np          # noqa: E402
import torch                # noqa: E402

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
import heatmap_cases as HC                               # noqa: E402
from achelous_amd import data as D                       # noqa: E402
from achelous_amd import prepost as P                    # noqa: E402
from achelous_amd.colormaps import JET                   # noqa: E402
from achelous_amd.engine import hip_library              # noqa: E402

R, ND = 320, 7
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
lib = hip_library()
say(f'device {torch.cuda.get_device_name(0)}; det maps R = {R}, {ND} classes, fp32; tile {64} rows x {128} columns per workgroup')

for label, shapes in (('64 frames of 1080 x 1920', [(1080, 1920)] * 64), ('16 frames of 1080 x 1920 + 16 of 720 x 1280, interleaved', [(1080, 1920), (720, 1280)] * 16)):
    B = len(shapes)
    g = torch.Generator().manual_seed(5)
    dets = [(torch.randn(B, 5 + ND, R // s, R // s, generator=g) * 3.0 - 2.0).to(dev) for s in (8, 16, 32)]
    pics = {sh: np.random.default_rng(sh[0]).integers(0, 256, (sh[0], sh[1], 3), dtype=np.uint8) for sh in set(shapes)}        # (one seeded picture per size)
    images = D.pack_arena([pics[sh] for sh in shapes], 3, dev, 'heat_timing')
    moff, mp, mbytes, ooff, op, obytes = P.frames_layout(shapes)
    A = sum(HC.cells(R))
    table = np.zeros((B, P.HEAT_TABLE_COLS), np.int64)
    for b, (h, w) in enumerate(shapes):
        table[b, :12] = (images.frames[b][0], h, w, images.frames[b][3], 0, 0, R, R, moff[b], mp[b], ooff[b], op[b])
    tdev, cdev = torch.from_numpy(table).to(dev), torch.from_numpy(JET.copy()).to(dev)
    scores, stats = torch.empty(B, A, device=dev), torch.empty(B, 2, dtype=torch.int32, device=dev)
    mask, out = torch.empty(mbytes, dtype=torch.uint8, device=dev), torch.empty(obytes, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(colour):
        def fn():
            rc = lib.lib.ach_heatmap_frames(0, R, ND, B, dets[0].data_ptr(), dets[1].data_ptr(), dets[2].data_ptr(), scores.data_ptr(), images.data.data_ptr(),
                                            images.data.numel(), table.ctypes.data, tdev.data_ptr(), cdev.data_ptr(), 0.5, mask.data_ptr(), mbytes, stats.data_ptr(),
                                            out.data_ptr() if colour else None, obytes, stream)
            assert rc == 0, lib.lib.ach_last_error(None)
        return fn

    def host(frames):
        def fn():
            d = [t[:frames].cpu().numpy() for t in dets]
            s = HC.scores(d)
            for b in range(frames):
                h, w = shapes[b]
                m = HC.mask_from_scores(s[b], R, h, w)
                img = torch.as_strided(images.data, (h, w, 3), (images.frames[b][3], 3, 1), images.frames[b][0]).cpu().numpy()
                pic = HC.colour(m, int(m.min()), int(m.max()), img, JET, 0.5)
                torch.as_strided(out, (h, w, 3), (op[b], 3, 1), ooff[b]).copy_(torch.from_numpy(pic))
            torch.cuda.synchronize()
        return fn

    # the bytes first: the three launches against the restatement on the first frames
    check = 2
    raw(True)()
    s_dev, rng_dev = scores.cpu().numpy(), torch.stack((255 - stats[:, 1], stats[:, 0]), 1).cpu().numpy()
    same = True
    for b in range(check):
        h, w = shapes[b]
        m = HC.mask_from_scores(s_dev[b], R, h, w)
        img = torch.as_strided(images.data, (h, w, 3), (images.frames[b][3], 3, 1), images.frames[b][0]).cpu().numpy()
        same = same and np.array_equal(torch.as_strided(mask, (h, w), (mp[b], 1), moff[b]).cpu().numpy(), m) and rng_dev[b].tolist() == [int(m.min()), int(m.max())]
        same = same and np.array_equal(torch.as_strided(out, (h, w, 3), (op[b], 3, 1), ooff[b]).cpu().numpy(), HC.colour(m, int(m.min()), int(m.max()), img, JET, 0.5))
    err = float(np.abs(s_dev[:check].astype(np.float64) - HC.scores([t[:check].cpu().numpy() for t in dets], np.float64)).max())
    px = sum(h * w for h, w in shapes)
    say(f'\n{label}: {px / 1e6:.1f} M pixels; mask, range and picture == restatement on the first {check} frames: {same}; max |score - float64| {err:.3g}; ranges {rng_dev[:check].tolist()}')
    assert same

    se = torch.randn(B, 9, R, R, generator=g).to(dev).to(torch.bfloat16)
    lane = torch.randn(B, 2, R, R, generator=g).to(dev).to(torch.bfloat16)
    legs = {'a2 scores + mask + statistics (2 launches, tables resident)': raw(False),
            'a3 scores + mask + colour (3 launches, tables resident)': raw(True),
            'a  heatmap_frames (tables built and uploaded, arenas allocated per call)': lambda: P.heatmap_frames(dets, shapes, images),
            'c  for scale: seg_maps_frames overlay launch (2 softmax + 1 launch)': P._seg_maps_plan(se, lane, shapes, images, want=('overlay',), meta_name='heat_timing')}
    hf = min(a.host_frames, B)
    host_fn = host(hf)
    iters = {k: iters_for(fn) for k, fn in legs.items()}
    host_fn()
    res = {k: [] for k in list(legs) + ['b']}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            res[k].append(timed_events(fn, iters[k]))
        t0 = time.perf_counter()
        host_fn()
        res['b'].append((time.perf_counter() - t0) * 1e3 * px / sum(h * w for h, w in shapes[:hf]))
    names = dict({k: k for k in legs}, b=f'b  host route: download, numpy, upload ({hf} frames timed, scaled to the batch by pixels)')
    for k, v in res.items():
        say(f'  {names[k]:<84} median {statistics.median(v):10.3f} ms   min {min(v):10.3f}   max {max(v):10.3f}   ({a.rounds} rounds)')
    col = statistics.median(res['a3 scores + mask + colour (3 launches, tables resident)']) - statistics.median(res['a2 scores + mask + statistics (2 launches, tables resident)'])
    say(f'  colour launch alone (a3 - a2): {col:.3f} ms; per pixel it reads 3 base bytes and 1 mask byte and writes 3: {7 * px / 1e6:.0f} MB, {7e-6 * px / max(col, 1e-6):.0f} GB/s')

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
