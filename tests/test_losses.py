"""The training losses of achelous_amd/losses.py (csrc/k_loss.h): SimOTA detection loss and the segmentation losses, forward and gradient.

Truth is the reference itself: tests/golden/loss_det.npz / loss_seg.npz hold what `loss.detection_loss.YOLOLoss` and `loss.segmentation_loss.*` compute (float64 and
fp32) on the seeded inputs of tests/loss_cases.py (gen_loss_golden.py; the inputs are regenerated here and checked against a stored checksum).  Where the reference
is not available — the full-tensor gradient comparison and the training-size runs on the GPU — tests/loss_checker.py stands in, itself pinned to the fixtures by
`test_checker_matches_reference_fixtures`.  Every case runs once under the emulation library (`-m "not gpu"`) and once on the MI355X (`-m gpu`).

Bounds: assignment decisions are EXACT (the fixtures' inputs keep every decision >= 1e-3 away from a tie, asserted by the generator); values and gradients are held
to a max-normalised 2e-4, the bound tests/test_train_functional.py holds every native training primitive to (the reference's own fp32 run is ~1e-6 from its float64
run on these inputs: loss.meta.json).  The checker in float64 is held to 1e-9."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_checker as CK
from achelous_amd import train_ops

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
TOL = 2e-4
LOSS_SYMBOLS = ('ach_train_yolo_loss', 'ach_train_loss_scale', 'ach_train_seg_loss')
DEVICES = [pytest.param('cpu', id='emu'), pytest.param('cuda', id='gpu', marks=pytest.mark.gpu)]
SEG_KEYS = ('ce', 'focal', 'dice', 'ce_dice', 'focal_dice')


@pytest.fixture(params=DEVICES)
def dev(request):
    """'cpu': the kernels under the emulation library; 'cuda': the HIP kernels"""
    if request.param == 'cpu':
        from emu_util import emu_library
        train_ops._lib.test_library = emu_library()
        try:
            yield 'cpu'
        finally:
            train_ops._lib.test_library = None
    else:
        yield 'cuda'


def _fx(name):
    return np.load(os.path.join(HERE, 'golden', name))


def _pack(labels, G=None):
    G = G or max(1, max(len(l) for l in labels))
    boxes = torch.zeros(len(labels), G, 5)
    for b, l in enumerate(labels):
        boxes[b, :len(l)] = l
    return boxes, torch.tensor([len(l) for l in labels], dtype=torch.int32)


def _det_case(name):
    fx = _fx('loss_det.npz')
    inputs, labels = LC.make_det_case(**LC.DET_CASES[name])
    boxes, counts = _pack(labels)
    got = np.array([LC.checksum(t) for t in inputs] + [LC.checksum(boxes)])
    assert np.allclose(got, fx[f'{name}/checksum'], rtol=1e-12, atol=0), 'tests/loss_cases.py no longer generates the inputs the fixtures were recorded on'
    return fx, inputs, labels, boxes, counts


def _seg_case(name):
    fx = _fx('loss_seg.npz')
    logits, png, w = LC.make_seg_case(**LC.SEG_CASES[name])
    got = np.array([LC.checksum(logits), LC.checksum(png), LC.checksum(w)])
    assert np.allclose(got, fx[f'{name}/checksum'], rtol=1e-12, atol=0), 'tests/loss_cases.py no longer generates the inputs the fixtures were recorded on'
    return fx, logits, png, w


def _grad_err(fx, key, g):
    """max-normalised error over the stored samples, and the relative error of the norm (the whole tensor)"""
    idx, val, stat = fx[key + '_idx'], fx[key + '_val'], fx[key + '_stat']
    ours = g.detach().double().cpu().reshape(-1)
    return max(float(np.abs(ours.numpy()[idx] - val).max() / stat[1]), abs(float(ours.norm()) - stat[0]) / stat[0])


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _seg_fn(key, C, checker):
    """the loss `key` of the fixtures as a function (logits, png, weights) of our drop-ins / of the checker"""
    if checker:
        main = {'ce': CK.ce_loss, 'focal': CK.focal_loss}
        if key == 'dice':
            return lambda x, png, w: CK.dice_loss(x, png)
        if key in main:
            return main[key]
        return lambda x, png, w: main[key.split('_')[0]](x, png, w) + CK.dice_loss(x, png)
    from achelous_amd import losses as L

    def onehot(png):
        return torch.eye(C + 1, device=png.device)[png.reshape(-1)].reshape(*png.shape, C + 1)
    main = {'ce': lambda x, png, w: L.CE_Loss(x, png, w, C), 'focal': lambda x, png, w: L.Focal_Loss(x, png, w, C)}
    if key == 'dice':
        return lambda x, png, w: L.Dice_loss(x, onehot(png))
    if key in main:
        return main[key]
    return lambda x, png, w: main[key.split('_')[0]](x, png, w) + L.Dice_loss(x, onehot(png))


# ------------------------------------------------------------------------------------------------------------------ the checker's own pin
@pytest.mark.parametrize('name', list(LC.DET_CASES))
def test_checker_matches_reference_fixtures(name):
    fx, inputs, labels, boxes, counts = _det_case(name)
    for dtype, tol in ((torch.float64, 1e-9), (torch.float32, TOL)):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in inputs]
        loss, asg = CK.detection_loss(leaves, boxes.to(dtype), counts, LC.NUM_DET)
        loss.backward()
        assert np.array_equal(asg['matched'].numpy(), fx[f'{name}/matched'].astype(np.int32))
        assert np.array_equal(asg['num_fg'].numpy(), fx[f'{name}/num_fg'])
        assert float(np.abs(asg['pred_iou'].double().numpy() - fx[f'{name}/pred_iou']).max()) <= tol
        ref = float(fx[f'{name}/loss'][0])
        assert abs(float(loss.detach()) - ref) <= tol * abs(ref), (float(loss.detach()), ref)
        for k, t in enumerate(leaves):
            assert _grad_err(fx, f'{name}/g{k}', t.grad) <= tol, (k, _grad_err(fx, f'{name}/g{k}', t.grad))
        assert float(asg['margin'].min()) >= 1e-3


@pytest.mark.parametrize('name', list(LC.SEG_CASES))
def test_checker_matches_reference_seg_fixtures(name):
    fx, logits, png, w = _seg_case(name)
    C = logits.shape[1]
    for key in SEG_KEYS:
        for dtype, tol in ((torch.float64, 1e-9), (torch.float32, TOL)):
            x = logits.to(dtype).clone().requires_grad_(True)
            loss = _seg_fn(key, C, True)(x, png, w.to(dtype))
            loss.backward()
            ref = float(fx[f'{name}/{key}/loss'][0])
            assert abs(float(loss) - ref) <= tol * abs(ref), (key, float(loss), ref)
            assert _grad_err(fx, f'{name}/{key}/g', x.grad) <= tol, key


# ------------------------------------------------------------------------------------------------------------------ detection
def _native_det(dev, inputs, labels_or_packed):
    from achelous_amd.losses import YOLOLoss
    leaves = [t.clone().to(dev).requires_grad_(True) for t in inputs]
    if isinstance(labels_or_packed, tuple):
        lab = tuple(t.to(dev) for t in labels_or_packed)
    else:
        lab = [t.to(dev) for t in labels_or_packed]
    loss, matched, pred_iou, num_fg = YOLOLoss(LC.NUM_DET).forward_with_assignment(leaves, lab)
    loss.backward()
    return loss, matched, pred_iou, num_fg, leaves


@pytest.mark.parametrize('name', list(LC.DET_CASES))
def test_assignment_equals_the_reference(dev, name):
    """1: foreground mask, matched box, num_fg exactly; matched IoU within 2e-4."""
    fx, inputs, labels, boxes, counts = _det_case(name)
    _, matched, pred_iou, num_fg, _ = _native_det(dev, inputs, labels)
    assert np.array_equal(matched.cpu().numpy() >= 0, fx[f'{name}/fg'])
    assert np.array_equal(matched.cpu().numpy(), fx[f'{name}/matched'].astype(np.int32))
    assert np.array_equal(num_fg.cpu().numpy(), fx[f'{name}/num_fg'])
    d = float(np.abs(pred_iou.double().cpu().numpy() - fx[f'{name}/pred_iou']).max())
    print(f'{name} [{dev}] matched IoU: max abs distance {d:.2e}')
    assert d <= TOL


@pytest.mark.parametrize('name', list(LC.DET_CASES))
def test_detection_loss_and_gradients(dev, name):
    """2: the loss and its three gradients against the reference (fixtures: samples + norm) and against the checker (every element)."""
    fx, inputs, labels, boxes, counts = _det_case(name)
    loss, _, _, _, leaves = _native_det(dev, inputs, labels)
    ref = float(fx[f'{name}/loss'][0])
    e_loss = abs(float(loss) - ref) / abs(ref)
    e_fix = [_grad_err(fx, f'{name}/g{k}', t.grad) for k, t in enumerate(leaves)]
    cl = [t.double().clone().requires_grad_(True) for t in inputs]
    CK.detection_loss(cl, boxes.double(), counts, LC.NUM_DET)[0].backward()
    e_chk = [_rel(a.grad, b.grad) for a, b in zip(leaves, cl)]
    print(f'{name} [{dev}] detection: loss {e_loss:.2e} gradients vs reference samples {[f"{e:.2e}" for e in e_fix]} vs checker {[f"{e:.2e}" for e in e_chk]}')
    assert e_loss <= TOL and max(e_fix) <= TOL and max(e_chk) <= TOL


def test_label_forms_untouched_inputs_and_determinism(dev):
    """3: list and packed labels give identical bits; the head maps are not modified; the same call twice gives identical bits."""
    _, inputs, labels, boxes, counts = _det_case('b4_320_s2')
    before = [t.clone() for t in inputs]
    a = _native_det(dev, inputs, labels)
    for t, l in zip(before, a[4]):
        assert torch.equal(t, l.detach().cpu())                                  # the call left its inputs alone
    b = _native_det(dev, inputs, _pack(labels))
    c = _native_det(dev, inputs, _pack(labels, G=17))                              # a wider padding changes nothing either
    d = _native_det(dev, inputs, labels)
    for other in (b, c, d):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1]) and torch.equal(a[2], other[2]) and torch.equal(a[3], other[3])
        for x, y in zip(a[4], other[4]):
            assert torch.equal(x.grad, y.grad)


def test_detection_cotangent_and_boxes_without_candidates(dev):
    """the backward scales by the incoming cotangent; a box no anchor is a candidate for (the reference raises) matches nothing and does not fault."""
    from achelous_amd.losses import YOLOLoss
    _, inputs, labels, _, _ = _det_case('b4_160')
    l1, _, _, _, leaves = _native_det(dev, inputs, labels)
    x = [t.clone().to(dev).requires_grad_(True) for t in inputs]
    (YOLOLoss(LC.NUM_DET)(x, [t.to(dev) for t in labels]) * -2.5).backward()
    for a, b in zip(x, leaves):
        assert _rel(a.grad, -2.5 * b.grad) <= 1e-6
    far = [torch.tensor([[5000.0, 5000.0, 30.0, 30.0, 1.0]]) for _ in range(inputs[0].shape[0])]
    loss, matched, _, num_fg, leaves = _native_det(dev, inputs, far)
    assert int((matched >= 0).sum()) == 0 and int(num_fg.sum()) == 0 and bool(torch.isfinite(loss))
    ref = sum(torch.nn.functional.binary_cross_entropy_with_logits(t[:, 4], torch.zeros_like(t[:, 4]), reduction='sum') for t in inputs)
    assert abs(float(loss) - float(ref)) <= TOL * float(ref)                      # objectness over all anchors / max(num_fg, 1)


# ------------------------------------------------------------------------------------------------------------------ segmentation
@pytest.mark.parametrize('key', SEG_KEYS)
@pytest.mark.parametrize('name', list(LC.SEG_CASES))
def test_segmentation_loss_and_gradient(dev, name, key):
    """2: each drop-in loss (and the two sums the loop uses) and its gradient against the reference."""
    fx, logits, png, w = _seg_case(name)
    C = logits.shape[1]
    x = logits.clone().to(dev).requires_grad_(True)
    loss = _seg_fn(key, C, False)(x, png.to(dev), w.to(dev))
    loss.backward()
    ref = float(fx[f'{name}/{key}/loss'][0])
    e_loss, e_grad = abs(float(loss) - ref) / abs(ref), _grad_err(fx, f'{name}/{key}/g', x.grad)
    xc = logits.double().clone().requires_grad_(True)
    _seg_fn(key, C, True)(xc, png, w.double()).backward()
    e_chk = _rel(x.grad, xc.grad)
    print(f'{name}/{key} [{dev}] loss {e_loss:.2e} gradient vs reference samples {e_grad:.2e} vs checker {e_chk:.2e}')
    assert e_loss <= TOL and e_grad <= TOL and e_chk <= TOL


@pytest.mark.parametrize('label_dtype', [torch.int64, torch.int32, torch.uint8])
@pytest.mark.parametrize('focal', [True, False])
@pytest.mark.parametrize('name', ['se9', 'lane2', 'se9_ignored_image'])
def test_fused_segloss_equals_the_sum_of_the_dropins(dev, name, focal, label_dtype):
    from achelous_amd.losses import SegLoss
    fx, logits, png, w = _seg_case(name)
    C = logits.shape[1]
    key = 'focal_dice' if focal else 'ce_dice'
    x = logits.clone().to(dev).requires_grad_(True)
    loss = SegLoss(C, w, focal=focal).to(dev)(x, png.to(label_dtype).to(dev))
    loss.backward()
    y = logits.clone().to(dev).requires_grad_(True)
    parts = _seg_fn(key, C, False)(y, png.to(dev), w.to(dev))
    parts.backward()
    ref = float(fx[f'{name}/{key}/loss'][0])
    assert abs(float(loss) - float(parts)) <= TOL * abs(float(parts)) and abs(float(loss) - ref) <= TOL * abs(ref)
    assert _rel(x.grad, y.grad) <= TOL and _grad_err(fx, f'{name}/{key}/g', x.grad) <= TOL
    x2 = logits.clone().to(dev).requires_grad_(True)
    loss2 = SegLoss(C, w, focal=focal).to(dev)(x2, png.to(label_dtype).to(dev))
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(x.grad, x2.grad)                # determinism


def test_segmentation_sizes_that_are_not_a_multiple_of_four(dev):
    """the one-pixel-per-thread form of the kernels (H * W % 4 != 0)"""
    from achelous_amd.losses import SegLoss
    g = torch.Generator().manual_seed(5)
    logits, png, w = 2 * torch.randn(2, 5, 9, 7, generator=g), torch.randint(0, 6, (2, 9, 7), generator=g), torch.rand(5, generator=g) + 0.5
    for focal in (True, False):
        x = logits.clone().to(dev).requires_grad_(True)
        loss = SegLoss(5, w, focal=focal).to(dev)(x, png.to(dev))
        loss.backward()
        xc = logits.double().clone().requires_grad_(True)
        ref = CK.seg_loss(xc, png, w.double(), focal=focal)
        ref.backward()
        assert abs(float(loss) - float(ref)) <= TOL * abs(float(ref)) and _rel(x.grad, xc.grad) <= TOL


# ------------------------------------------------------------------------------------------------------------------ errors, exports
def test_errors(dev):
    """4: G above the cap, size mismatch of logits and labels, non-fp32 inputs outside autocast."""
    from achelous_amd import losses as L
    _, inputs, labels, boxes, counts = _det_case('b4_160')
    ins = [t.to(dev) for t in inputs]
    with pytest.raises(ValueError):
        L.pack_labels(labels, L.MAX_BOXES + 1)
    with pytest.raises(ValueError):
        L.pack_labels([torch.zeros(L.MAX_BOXES + 1, 5)])
    with pytest.raises(ValueError):
        L.YOLOLoss(LC.NUM_DET)(ins, (torch.zeros(4, L.MAX_BOXES + 1, 5, device=dev), counts.to(dev)))
    with pytest.raises(TypeError):
        L.YOLOLoss(LC.NUM_DET)([t.double() for t in ins], [t.to(dev) for t in labels])
    with pytest.raises(TypeError):
        L.YOLOLoss(LC.NUM_DET)(ins, (boxes.to(dev), counts.long().to(dev)))
    _, logits, png, w = _seg_case('lane2')
    logits, png, w = logits.to(dev), png.to(dev), w.to(dev)
    with pytest.raises(ValueError):
        L.CE_Loss(logits, png[:, :48, :48], w, 2)
    with pytest.raises(ValueError):
        L.Focal_Loss(logits[:, :, :48], png, w, 2)
    with pytest.raises(ValueError):
        L.Dice_loss(logits, torch.zeros(2, 48, 48, 3, device=dev))
    with pytest.raises(ValueError):
        L.SegLoss(2, w).to(dev)(logits, png[:, :48])
    with pytest.raises(TypeError):
        L.SegLoss(2, w).to(dev)(logits.half() if dev == 'cuda' else logits.double(), png)
    with pytest.raises(TypeError):
        L.SegLoss(2, w).to(dev)(logits, png.float())


def test_losses_need_the_gpu_library():
    """no CPU path: without the (test-only) emulation library CPU tensors are refused"""
    from achelous_amd.losses import SegLoss
    assert getattr(train_ops._lib, 'test_library', None) is None
    with pytest.raises(RuntimeError):
        SegLoss(2, torch.ones(2))(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_both_libraries_export_the_loss_entry_points():
    """7: every new ach_train_* symbol is exported by libachelous_hip.so built for gfx950 and by the emulation library."""
    from achelous_amd import engine as eng_mod
    from emu_util import emu_library, EMU_LIBRARY
    emu_library()
    if not os.path.exists(eng_mod.HIP_LIBRARY):
        import __graft_entry__
        __graft_entry__.build()
    for path in (eng_mod.HIP_LIBRARY, EMU_LIBRARY):
        lib = ctypes.CDLL(path)
        for s in LOSS_SYMBOLS:
            assert hasattr(lib, s), (path, s)
            assert s in eng_mod.NativeLibrary.SYMBOLS


# ------------------------------------------------------------------------------------------------------------------ GPU only
@pytest.mark.gpu
def test_gpu_losses_under_autocast():
    """Under torch.autocast the wrappers cast to fp32: half-precision head maps and logits are accepted there, and the result is that of the fp32 call on the same values."""
    from achelous_amd.losses import SegLoss, YOLOLoss
    _, inputs, labels, _, _ = _det_case('b4_160')
    _, logits, png, w = _seg_case('lane2')
    halves = [t.cuda().half() for t in inputs]
    with torch.autocast('cuda', dtype=torch.float16):
        a = YOLOLoss(LC.NUM_DET, fp16=True)(halves, [t.cuda() for t in labels])
        s = SegLoss(2, w).cuda()(logits.cuda().half(), png.cuda())
    b = YOLOLoss(LC.NUM_DET)([t.float() for t in halves], [t.cuda() for t in labels])
    t = SegLoss(2, w).cuda()(logits.cuda().half().float(), png.cuda())
    assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(s, t)


@pytest.mark.gpu
def test_gpu_assignment_at_training_size():
    """5: batch 32 at 320 x 320, up to 40 boxes per image, 8 seeded batches, against the checker on the same device.  Two fp32 evaluations may part on a near-tie, so
    images whose checker margins are below 1e-3 are left out of the decision comparison — at most 15 % of them (the reference alone leaves out 9.3 % at <= 40 boxes);
    on all others the decisions are exact and the loss recomputed over the compared images agrees to 2e-4."""
    from achelous_amd.losses import YOLOLoss
    total = left_out = 0
    crit = YOLOLoss(LC.NUM_DET)
    for seed in range(8):
        inputs, labels = LC.make_det_case(seed=100 + seed, B=32, res=320, gmax=40)
        boxes, counts = _pack(labels, 40)
        ins, boxes, counts = [t.cuda() for t in inputs], boxes.cuda(), counts.cuda()
        _, asg = CK.detection_loss(ins, boxes, counts, LC.NUM_DET)
        _, matched, pred_iou, num_fg = crit.forward_with_assignment(ins, (boxes, counts))
        keep = asg['margin'] >= 1e-3
        total += keep.numel()
        left_out += int((~keep).sum())
        assert torch.equal(matched[keep], asg['matched'][keep]) and torch.equal(num_fg[keep], asg['num_fg'][keep])
        assert float((pred_iou[keep] - asg['pred_iou'][keep]).abs().max()) <= TOL
        sub = [t[keep].contiguous() for t in ins]
        ours = crit(sub, (boxes[keep].contiguous(), counts[keep].contiguous()))
        ref, _ = CK.detection_loss(sub, boxes[keep], counts[keep], LC.NUM_DET)
        assert abs(float(ours) - float(ref)) <= TOL * abs(float(ref)), (seed, float(ours), float(ref))
    print(f'training-size assignment: {left_out} of {total} images left out of the decision comparison ({100.0 * left_out / total:.1f} %)')
    assert left_out <= 0.15 * total, (left_out, total)


def _step_targets(seed, counts, res=96, points=64, G=8):
    g = torch.Generator().manual_seed(seed)
    labels = []
    for n in counts:
        cxy = torch.rand(n, 2, generator=g) * (res - 20) + 10
        wh = torch.rand(n, 2, generator=g) * 48 + 12
        labels.append(torch.cat([cxy, wh, torch.randint(0, 7, (n, 1), generator=g).float()], 1))
    boxes, cnt = _pack(labels, G)
    return (boxes.cuda(), cnt.cuda(), torch.randint(0, 10, (len(counts), res, res), generator=g).cuda(), torch.randint(0, 3, (len(counts), res, res), generator=g).cuda(),
            torch.randint(0, 8, (len(counts), points), generator=g).cuda())


@pytest.mark.gpu
def test_gpu_graphed_training_step_with_the_real_losses():
    """6: `GraphedTrainStep` with `MultiTaskLoss` — SimOTA detection loss, focal + Dice on both segmentation heads, NLL on the points — captured once and replayed on three
    batches whose box counts differ (one with an empty image), against three eager steps of a twin model: the reason for the feature (the reference's detection loss reads
    the device dozens of times per step and cannot be captured).  Bounds as test_gpu_graphed_training_step_equals_the_eager_step."""
    from achelous_amd import Achelous
    from achelous_amd.losses import MultiTaskLoss
    from achelous_amd.synth import condition_state_dict, make_inputs
    from achelous_amd.train_graph import GraphedTrainStep
    kw = dict(num_det=7, num_seg=9, phi='S0', resolution=96, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
    sd = condition_state_dict(Achelous(**kw).state_dict(), seed=0)
    batches = [tuple(t.cuda() for t in make_inputs(2, 30 + i, resolution=96, num_points=64, pc_channels=5, radar_cells=12)) for i in range(3)]
    targets = [_step_targets(70 + i, c) for i, c in enumerate([(3, 5), (8, 0), (1, 2)])]
    g = torch.Generator().manual_seed(1)
    loss_fn = MultiTaskLoss(7, 9, torch.rand(9, generator=g) + 0.5, torch.rand(2, generator=g) + 0.5).cuda()

    def make():
        m = Achelous(**kw)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().train()
        return m, torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
    m1, o1 = make()
    eager = []
    for (x, xr, xp), t in zip(batches, targets):
        o1.zero_grad(set_to_none=True)
        loss = loss_fn(m1(x, xr, xp), *t)
        loss.backward()
        o1.step()
        eager.append(float(loss.detach()))
    del loss
    m2, o2 = make()
    step = GraphedTrainStep(m2, o2, loss_fn, batches[0], targets[0])
    graphed = [float(step(*b, *t)) for b, t in zip(batches, targets)]
    torch.cuda.synchronize()
    print('eager', eager, 'graphed', graphed)
    assert len(set(eager)) == 3 and all(np.isfinite(eager))
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 1e-4 * abs(a) + 1e-7, (eager, graphed)
    s1, s2 = m1.state_dict(), m2.state_dict()
    for k in s1:
        if s1[k].is_floating_point():
            d = float((s1[k].double() - s2[k].double()).abs().max())
            assert d <= 1e-4 * float(s1[k].double().abs().max()) + 1e-6, (k, d)
        else:
            assert torch.equal(s1[k], s2[k]), k
