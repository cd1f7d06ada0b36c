"""Seeded inputs of the loss tests, shared by tests/golden/gen_loss_golden.py (which runs the reference on them) and tests/test_losses.py (which regenerates them:
the raw tensors would not fit the size limit of a committed file; the fixtures hold a checksum of each, so a change of the generator's stream is detected, not
silently compared against).  CPU generators only."""
import torch

NUM_DET = 7

# detection: raw maps resembling an early-training head, boxes with centres inside the image and sides 12 - 132 px; image 1 of every batch has no boxes
DET_CASES = {
    'b4_320_s2': dict(seed=2, B=4, res=320, gmax=12),                 # contested anchors
    'b4_320_s4': dict(seed=4, B=4, res=320, gmax=12),                 # contested anchors
    'b4_160': dict(seed=3, B=4, res=160, gmax=12),
    'b2_320_g40': dict(seed=5, B=2, res=320, gmax=40, fixed=40),      # image 0: 40 boxes
}


def make_det_case(seed, B=4, res=320, gmax=12, fixed=None, C=NUM_DET):
    g = torch.Generator().manual_seed(seed)
    inputs = []
    for s in (8, 16, 32):
        h = res // s
        t = torch.randn(B, 5 + C, h, h, generator=g)
        t[:, 2:4] = t[:, 2:4] * 0.5 + 1.2
        t[:, 4:] = t[:, 4:] - 2.0
        inputs.append(t)
    labels = []
    for b in range(B):
        n = 0 if b == 1 else (int(fixed) if fixed else int(torch.randint(1, gmax + 1, (1,), generator=g)))
        cxy = torch.rand(n, 2, generator=g) * (res - 40) + 20
        wh = torch.rand(n, 2, generator=g) * 120 + 12
        cls = torch.randint(0, C, (n, 1), generator=g).float()
        labels.append(torch.cat([cxy, wh, cls], 1))
    return inputs, labels


# segmentation: logits ~ 2 N(0, 1), labels uniform over 0..C (C = ignored), random positive class weights
SEG_CASES = {
    'se9': dict(seed=11, C=9),
    'lane2': dict(seed=12, C=2),
    'se9_absent': dict(seed=13, C=9, absent=4),                       # class 4 never occurs
    'se9_ignored_image': dict(seed=14, C=9, ignored_image=1),          # image 1 is ignored as a whole
}


def make_seg_case(seed, C, absent=None, ignored_image=None, B=2, H=96, W=96):
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(B, C, H, W, generator=g)
    png = torch.randint(0, C + 1, (B, H, W), generator=g)
    weights = torch.rand(C, generator=g) + 0.5
    if absent is not None:
        png[png == absent] = (absent + 1) % C
    if ignored_image is not None:
        png[ignored_image] = C
    return logits, png, weights


def checksum(t):
    t = t.double()
    return [float(t.sum()), float(t.abs().sum())]
