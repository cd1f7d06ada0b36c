"""Time of the training losses (achelous_amd/losses.py) on the GPU, forward + backward, against the same losses as a torch-op composite (tests/loss_checker.py,
eager: the kinder stand-in for the reference's losses, without their per-box host reads), and their share of a whole training step.
Device events around synchronised work, warm-up, >= 1 s of timed work per leg, the two legs alternated in one process, spread reported.
usage: python profiles/scripts/losses_step_time.py [--batch 32] [--rounds 5] [--kernels-only N]     (--kernels-only: N plain iterations of the native losses, for rocprofv3)"""
import argparse
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
import loss_cases as LC                                  # noqa: E402
import loss_checker as CK                                # noqa: E402
from achelous_amd import Achelous, losses as L           # noqa: E402
from achelous_amd.synth import condition_state_dict, make_inputs       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--resolution', type=int, default=320)
ap.add_argument('--kernels-only', type=int, default=0)
ap.add_argument('--step-batches', type=int, nargs='*', default=[32, 8])
a = ap.parse_args()
dev = 'cuda'
B, R = a.batch, a.resolution
g = torch.Generator().manual_seed(0)


def targets(batch, points=1024):
    inputs, labels = LC.make_det_case(seed=7, B=batch, res=R, gmax=12)
    boxes, counts = L.pack_labels(labels, 12)
    return ([t.to(dev) for t in inputs], boxes.to(dev), counts.to(dev), torch.randint(0, 10, (batch, R, R), generator=g).to(dev),
            torch.randint(0, 3, (batch, R, R), generator=g).to(dev), torch.randint(0, 8, (batch, points), generator=g).to(dev))


raw, boxes, counts, png, png_w, _ = targets(B)
se = (2 * torch.randn(B, 9, R, R, generator=g)).to(dev)
lane = (2 * torch.randn(B, 2, R, R, generator=g)).to(dev)
w, w_wl = (torch.rand(9, generator=g) + 0.5).to(dev), (torch.rand(2, generator=g) + 0.5).to(dev)
det_loss, seg_loss, lane_loss = L.YOLOLoss(LC.NUM_DET), L.SegLoss(9, w).to(dev), L.SegLoss(2, w_wl).to(dev)


def leaves(ts):
    return [t.detach().requires_grad_(True) for t in ts]


def native_det():
    x = leaves(raw)
    det_loss(x, (boxes, counts)).backward()


def native_seg():
    x, y = leaves([se, lane])
    (seg_loss(x, png) + lane_loss(y, png_w)).backward()


def torch_det():
    x = leaves(raw)
    CK.detection_loss(x, boxes, counts, LC.NUM_DET)[0].backward()


def torch_seg():
    x, y = leaves([se, lane])
    (CK.seg_loss(x, png, w) + CK.seg_loss(y, png_w, w_wl)).backward()


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


if a.kernels_only:
    for _ in range(a.kernels_only):
        native_det()
        native_seg()
    torch.cuda.synchronize()
    sys.exit(0)

print(f'losses forward + backward, batch {B} at {R} x {R}, <= 12 boxes per image, fp32; ms per call (median of {a.rounds} alternated rounds, min .. max)')
res = {}
for name, fa, fb in (('detection', torch_det, native_det), ('segmentation (se 9 classes + lane 2 classes, focal + Dice)', torch_seg, native_seg)):
    for fn in (fa, fb, fa, fb):
        fn()                                                              # warm-up: allocator pools, code objects
    ia = max(3, int(1000.0 / a.rounds / max(timed(fa, 3), 1e-3)) + 1)      # >= 1 s of timed work per leg over the rounds
    ib = max(3, int(1000.0 / a.rounds / max(timed(fb, 3), 1e-3)) + 1)
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(fa, ia))
        tb.append(timed(fb, ib))
    ta.sort(); tb.sort()
    res[name] = (ta, tb)
    print(f'  {name}')
    print(f'    A torch composite (tests/loss_checker.py, eager): {ta[len(ta) // 2]:8.3f}  ({ta[0]:.3f} .. {ta[-1]:.3f}; {ia} calls per round)')
    print(f'    B achelous_amd.losses                           : {tb[len(tb) // 2]:8.3f}  ({tb[0]:.3f} .. {tb[-1]:.3f}; {ib} calls per round)')
    print(f'    A / B = {ta[len(ta) // 2] / tb[len(tb) // 2]:.2f}; A - B = {ta[len(ta) // 2] - tb[len(tb) // 2]:.3f} ms, spread of A = {ta[-1] - ta[0]:.3f} ms')
loss_ms = {B: sum(tb[len(tb) // 2] for _, tb in res.values())}
del se, lane

kw = dict(num_det=7, num_seg=9, phi='S0', resolution=R, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
print('whole training step (forward in .train() + MultiTaskLoss + backward + SGD), eager, same run')
for sb in a.step_batches:
    m = Achelous(**kw)
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=0))
    m = m.to(dev).train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-4, momentum=0.9)
    x, xr, xp = (t.to(dev) for t in make_inputs(sb, 3, resolution=R, pc_channels=5))
    _, bx, ct, pg, pgw, pcl = targets(sb, xp.shape[-1])
    mt = L.MultiTaskLoss(7, 9, w, w_wl).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        mt(m(x, xr, xp), bx, ct, pg, pgw, pcl).backward()
        opt.step()

    def step_losses():
        det, s, l, pc = outs
        xs = leaves([*det, s, l])
        (mt.det(xs[:3], (bx, ct)) + mt.seg(xs[3], pg) + mt.lane(xs[4], pgw)).backward()
    for _ in range(3):
        step()
    it = max(3, int(1200.0 / timed(step, 2)) + 1)
    ts = sorted(timed(step, max(2, it // 3)) for _ in range(3))
    outs = m(x, xr, xp)
    outs = ([t.detach() for t in outs[0]], outs[1].detach(), outs[2].detach(), outs[3].detach())
    for _ in range(3):
        step_losses()
    tl = sorted(timed(step_losses, 50) for _ in range(3))
    print(f'  batch {sb:2d}: step {ts[1]:7.2f} ms ({ts[0]:.2f} .. {ts[2]:.2f}); the three native losses forward + backward on its outputs {tl[1]:6.3f} ms ({tl[0]:.3f} .. {tl[2]:.3f}) '
          f'= {100.0 * tl[1] / ts[1]:.1f} % of the step')
    del m, opt, outs
    torch.cuda.empty_cache()
print('launches per forward + backward: detection 5 (assign, resolve, loss-and-gradient, reducer | cotangent scale); each SegLoss 3 (forward, reducer | backward)')
