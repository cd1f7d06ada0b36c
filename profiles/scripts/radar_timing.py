"""Time of rasterising raw radar point clouds into the network's radar map (achelous_amd/data.py radar_maps_batch, csrc/k_radarmap.h) against the other ways to it.
Workload: B seeded clouds of 300 points (range, doppler, rcs, u in [0, 1920), v in [0, 1080)), float64, R = 320, cell (6, 3.375); B = 1 and 64.
  a   the raw map, one launch (clouds and table resident)
  a1  `radar_maps_batch` as a caller uses it: a + packing and uploading the clouds and the table per call
  b   the normalised map (bf16) in two launches: the raster pass also gives the extrema, then the scaling launch
  b0  a + the existing `prepost.preprocess_input_radar` (min / max launch + scaling launch): three launches
  c   for scale: the reference's loop on the host (the independent-walk restatement of tests/radar_cases.py, which does less Python work than the notebook's
      triple loop) + the upload of the dense maps; wall clock, one pass per round
Device events around the calls, warm-up, >= 0.5 s of timed work per leg and round, legs alternated in one process, median and spread of the rounds.  Before anything is
timed the results of the legs are compared.
usage: python profiles/scripts/radar_timing.py [--rounds 5] [--out FILE]"""
import argparse
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
import radar_cases as RC                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()
R, N, DT = 320, 300, torch.bfloat16
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


def timed_wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def iters_for(fn, target_ms=500.0, cap=50000):
    fn()
    one = timed_events(fn, 2)
    return max(1, min(cap, int(target_ms / max(one, 1e-3))))


assert torch.cuda.is_available(), 'radar_timing.py measures on the GPU; there is nothing to fall back to'
say(f'profiles/scripts/radar_timing.py on one MI355X (device events, warm-up, >= 0.5 s of timed work per leg and round, legs alternated in one process; ms per batch, median of '
    f'{a.rounds} rounds, min .. max; leg c: wall clock, one pass per round)')
for B in (1, 64):
    rng = np.random.default_rng(B)
    clouds = []
    for _ in range(B):
        p = np.zeros((N, 5))
        p[:, :3] = rng.normal(size=(N, 3)) * np.array([40.0, 3.0, 12.0])
        p[:, 3], p[:, 4] = rng.uniform(0, 1920, N), rng.uniform(0, 1080, N)
        clouds.append(p)
    packed = D.pack_clouds(clouds, 'cuda', f'timing_clouds{B}')
    meta = D._Meta(packed.data.device, f'timing_radar{B}')
    ref = D._plan_clouds(meta, packed, D.MAP_COLUMNS)
    meta.commit()

    def leg_a():
        return D._launch_radar_maps(meta, packed, ref, R, D.CELL, False, torch.float32)

    def leg_a1():
        return D.radar_maps_batch(clouds, R)

    def leg_b():
        return D._launch_radar_maps(meta, packed, ref, R, D.CELL, True, DT)

    def leg_b0():
        return P.preprocess_input_radar(leg_a(), DT)

    def leg_c():
        return torch.from_numpy(RC.rasterise_batch(clouds, R).astype(np.float32)).cuda()

    # ---- every leg computes the same map
    raw, host = leg_a(), leg_c()
    assert torch.equal(raw, host) and torch.equal(raw, leg_a1()), 'the raw map differs from the host restatement'
    assert torch.equal(leg_b().view(torch.int16), leg_b0().view(torch.int16)), 'the normalised map differs from preprocess_input_radar'
    del host
    legs = [('a  raw map, one launch (clouds and table resident)', leg_a), ('a1 radar_maps_batch as called: a + clouds and table packed and uploaded', leg_a1),
            ('b  normalised bf16 map, extrema from the raster pass (two launches)', leg_b), ('b0 a + existing preprocess_input_radar (three launches)', leg_b0)]
    its = {name: iters_for(fn) for name, fn in legs}
    res = {name: [] for name, _ in legs}
    res_c = []
    for _ in range(a.rounds):
        for name, fn in legs:
            res[name].append(timed_events(fn, its[name]))
        res_c.append(timed_wall(leg_c, 1))
    say()
    say(f'batch {B}: {N} points per cloud (float64), R = {R}, cell {D.CELL} (a, a1 and c give the same raw map, b and b0 the same bf16 bits: asserted)')
    med = {}
    for name, _ in legs:
        v = res[name]
        med[name] = statistics.median(v)
        say(f'  {name:<76}: {med[name]:9.4f}  ({min(v):.4f} .. {max(v):.4f}; {its[name]} calls per round)')
    mc = statistics.median(res_c)
    say(f"  {'c  for scale: host loop (restatement) + upload of the dense maps, wall clock':<76}: {mc:9.3f}  ({min(res_c):.3f} .. {max(res_c):.3f}; 1 pass per round)")
    k = [n for n, _ in legs]
    say(f'  b0 / b = {med[k[3]] / med[k[2]]:.2f}   c / a1 = {mc / med[k[1]]:.0f}   run-to-run spread of b and b0: '
        f'{max((max(res[n]) - min(res[n])) / med[n] for n in (k[2], k[3])) * 100:.1f} % of the median')
    mb = B * 3 * R * R * 4 / 1e6
    say(f'  raw map written: {mb:.1f} MB -> {mb / med[k[0]] / 1e3:.3f} TB/s by call time of a, {mb / med[k[0]] / 1e3 / 8 * 100:.1f} % of the 8 TB/s HBM peak')
if a.out:
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
