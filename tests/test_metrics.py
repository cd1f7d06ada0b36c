"""The validation metrics of achelous_amd/metrics.py (csrc/k_metrics.h): fused arg-max + confusion matrix, detection-to-ground-truth matching, VOC AP.

Truth is the reference itself: tests/golden/metrics.npz holds what `utils_seg.utils_metrics.fast_hist` / `per_*`, `utils_seg_pc.utils_metrics.mean_iou` and
`utils.utils_map.get_map` compute on the inputs of tests/metrics_cases.py (gen_metrics_golden.py; the segmentation inputs are regenerated here and checked against
a stored checksum, the detection case is stored whole).  Every case runs once under the emulation library (`-m "not gpu"`) and once on the MI355X (`-m gpu`).

Bounds: everything the kernels produce is integer arithmetic or an ordering decision and is held EXACTLY — histograms, flags, matches, scores (one fp32 multiply)
and the float64 IoU (integer inputs, one correctly rounded division).  `rec` / `prec` are exact (integer counts, one float64 division each).  The derived ratios,
AP and mAP are the same float64 formulas on identical integers, only the order of a summation may differ: 1e-12."""
import os

import numpy as np
import pytest
import torch

import metrics_cases as MC
from achelous_amd import metrics as M
from achelous_amd import train_ops

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICES = [pytest.param('cpu', id='emu'), pytest.param('cuda', id='gpu', marks=pytest.mark.gpu)]
LABEL_KINDS = [torch.int64, torch.int32, torch.uint8]
RATIO_TOL = 1e-12
_FX = None


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


def _fx():
    global _FX
    if _FX is None:
        with np.load(os.path.join(HERE, 'golden', 'metrics.npz')) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def _conf_case(name):
    fx = _fx()
    logits, quant, labels = MC.make_conf_case(**MC.CONF_CASES[name])
    got = np.array([MC.checksum(logits), MC.checksum(quant), MC.checksum(labels)])
    assert np.allclose(got, fx[f'conf/{name}/checksum'], rtol=1e-12, atol=0), 'tests/metrics_cases.py no longer generates the inputs the fixtures were recorded on'
    return fx, logits, quant, labels


def _hist(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ confusion
@pytest.mark.parametrize('dkey', list(MC.DTYPES))
@pytest.mark.parametrize('name', list(MC.CONF_CASES))
def test_confusion_matches_reference(dev, name, dkey):
    """every case x logit type x label kind: the histogram is the reference's, exactly; the 16-bit inputs are full of ties, pinned to torch.argmax as well"""
    fx, logits, quant, labels = _conf_case(name)
    cfg = MC.CONF_CASES[name]
    x = MC.logits_of(logits, quant, dkey)
    ref = fx[f'conf/{name}/hist_{dkey}']
    # the fixture's arg-max is numpy's; torch's on the very tensor the kernel reads gives the same histogram (ties: lowest index)
    pred = torch.argmax(x.float(), dim=MC.class_axis(cfg['layout'])).reshape(-1).numpy()
    lab = labels.reshape(-1).numpy()
    k = (lab >= 0) & (lab < cfg['C'])
    assert np.array_equal(np.bincount(cfg['C'] * lab[k] + pred[k], minlength=cfg['C'] ** 2).reshape(cfg['C'], cfg['C']), ref)
    for kind in LABEL_KINDS:
        m = M.SegConfusion(cfg['C'], dev)
        m.update(x.to(dev), MC.labels_as(labels, kind).to(dev))
        got = _hist(m.hist)
        print(name, dkey, kind, 'counted', int(got.sum()), 'differing bins', int((got != ref).sum()))
        assert np.array_equal(got, ref), (name, dkey, kind)


@pytest.mark.parametrize('name', ['c9', 'c9_vec', 'pc8'])
def test_confusion_class_map_and_drop_in(dev, name):
    """a uint8 class map gives what the logits give; `fast_hist` takes the reference's arguments"""
    fx, logits, quant, labels = _conf_case(name)
    cfg = MC.CONF_CASES[name]
    ref = fx[f'conf/{name}/hist_f32']
    cmap = torch.argmax(logits, dim=MC.class_axis(cfg['layout'])).to(torch.uint8)
    for kind in LABEL_KINDS:
        m = M.SegConfusion(cfg['C'], dev)
        m.update(cmap.to(dev), MC.labels_as(labels, kind).to(dev))
        assert np.array_equal(_hist(m.hist), ref), kind
    got = M.fast_hist(labels.reshape(-1).to(dev), cmap.reshape(-1).to(torch.int64).to(dev), cfg['C'])
    assert got.dtype == torch.int64 and np.array_equal(_hist(got), ref)


def test_confusion_one_bin(dev):
    """every pixel in one bin: the case in which all lanes of a wave add to one address (2 x 37 x 41 and a vector-path size)"""
    ref = _fx()['conf/onebin/hist']
    m = M.SegConfusion(9, dev)
    m.update(torch.zeros(2, 37, 41, dtype=torch.uint8, device=dev), torch.zeros(2, 37, 41, dtype=torch.int64, device=dev))
    assert np.array_equal(_hist(m.hist), ref)
    x = torch.zeros(2, 9, 32, 40, dtype=torch.bfloat16, device=dev)              # all logits equal: class 0 wins every tie
    m = M.SegConfusion(9, dev)
    m.update(x, torch.full((2, 32, 40), 3, dtype=torch.uint8, device=dev))
    exp = np.zeros((9, 9), np.int64)
    exp[3, 0] = 2 * 32 * 40
    assert np.array_equal(_hist(m.hist), exp)


def test_confusion_accumulates_carries_and_repeats(dev):
    """three updates = one on the concatenation; the accumulator is 64-bit (a bin preset to 2**32 - 5 carries); two runs give the same bits; reset clears"""
    fx, logits, quant, labels = _conf_case('c9')
    ref = fx['conf/c9/hist_bf16']
    x = quant.to(torch.bfloat16)
    big = torch.cat([x, x.flip(0), x[:1]]).to(dev)
    lab = torch.cat([labels, labels.flip(0), labels[:1]]).to(dev)
    one = M.SegConfusion(9, dev)
    one.update(big, lab)
    three = M.SegConfusion(9, dev)
    three.update(big[:2], lab[:2])
    three.update(big[2:4], lab[2:4])
    three.update(big[4:], lab[4:])
    assert np.array_equal(_hist(one.hist), _hist(three.hist))
    again = M.SegConfusion(9, dev)
    again.update(big, lab)
    assert torch.equal(one.hist, again.hist)
    m = M.SegConfusion(9, dev)
    r, c = np.unravel_index(int(ref.argmax()), ref.shape)
    assert ref[r, c] > 5
    m.hist[r, c] = 2 ** 32 - 5
    m.update(x.to(dev), labels.to(dev))
    exp = ref.copy()
    exp[r, c] += 2 ** 32 - 5
    assert np.array_equal(_hist(m.hist), exp) and exp[r, c] > 2 ** 32
    m.reset()
    assert int(m.hist.abs().sum()) == 0


def test_confusion_rejects(dev):
    with pytest.raises(ValueError):
        M.SegConfusion(17, dev)
    hist = torch.zeros(17, 17, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        M._confusion(hist, torch.zeros(1, 17, 8, device=dev), torch.zeros(1, 8, dtype=torch.int64, device=dev), 17)
    lib = train_ops._lib(hist)                                                   # the C entry itself
    x, lab = torch.zeros(1, 17, 8, device=dev), torch.zeros(1, 8, dtype=torch.int64, device=dev)
    rc = lib.lib.ach_eval_confusion(train_ops._p(x), 0, 0, train_ops._p(lab), 0, 1, 17, 8, train_ops._p(hist), train_ops._stream(x))
    assert rc == -1 and int(hist.sum()) == 0                                     # ACH_ERR_INVALID
    m = M.SegConfusion(9, dev)
    with pytest.raises(ValueError):
        m.update(torch.zeros(2, 8, 4, 4, device=dev), torch.zeros(2, 4, 4, dtype=torch.int64, device=dev))
    with pytest.raises(TypeError):
        m.update(torch.zeros(2, 9, 4, 4, device=dev), torch.zeros(2, 4, 4, dtype=torch.int16, device=dev))


@pytest.mark.parametrize('name', ['c2', 'c9', 'c16', 'pc8'])
def test_derived_ratios(dev, name):
    fx, logits, quant, labels = _conf_case(name)
    cfg = MC.CONF_CASES[name]
    m = M.SegConfusion(cfg['C'], dev)
    m.update(logits.to(dev), labels.to(dev))
    r = m.compute()
    assert np.array_equal(r['hist'], fx[f'conf/{name}/hist_f32'])
    for key in ('iou', 'pa_recall', 'precision'):
        assert np.abs(r[key] - fx[f'conf/{name}/{key}']).max() <= RATIO_TOL, key
    assert abs(r['accuracy'] - fx[f'conf/{name}/accuracy'][0]) <= RATIO_TOL and abs(r['miou'] - fx[f'conf/{name}/miou'][0]) <= RATIO_TOL
    h = torch.from_numpy(fx[f'conf/{name}/hist_f32']).to(dev)                    # the drop-ins take tensors
    assert np.abs(M.per_class_iu(h) - fx[f'conf/{name}/iou']).max() <= RATIO_TOL
    assert np.abs(M.per_class_PA_Recall(h) - fx[f'conf/{name}/pa_recall']).max() <= RATIO_TOL
    assert np.abs(M.per_class_Precision(h) - fx[f'conf/{name}/precision']).max() <= RATIO_TOL
    assert abs(M.per_Accuracy(h) - fx[f'conf/{name}/accuracy'][0]) <= RATIO_TOL
    # the point-cloud formula on a matrix with an absent class: NaN for that class, nanmean over the rest
    m.hist.copy_(torch.from_numpy(fx[f'conf/{name}/pc_hist']))
    ious, miou = m.pc_mean_iou()
    ref = fx[f'conf/{name}/pc_ious']
    assert np.isnan(ious[-1]) and np.isnan(ref[-1]) and np.array_equal(np.isnan(ious), np.isnan(ref))
    assert np.nanmax(np.abs(ious - ref)) <= RATIO_TOL and abs(miou - fx[f'conf/{name}/pc_miou'][0]) <= RATIO_TOL


# ------------------------------------------------------------------------------------------------------------------ matching
def _det_inputs(dev, fx=None):
    fx = fx or _fx()
    return [torch.from_numpy(fx[f'det/{k}']).to(dev) for k in ('rows', 'counts', 'gt', 'gt_counts', 'difficult')]


def _assert_match_equal(got, fx_or_exp, counts):
    flags, match, iou, score, gtc = [t.cpu().numpy() for t in got]
    e_flags, e_match, e_iou, e_score, e_gtc = fx_or_exp
    assert np.array_equal(flags, e_flags), int((flags != e_flags).sum())
    assert np.array_equal(match, e_match)
    assert score.dtype == np.float32 and np.array_equal(score, e_score)
    assert iou.dtype == np.float64 and np.array_equal(iou, e_iou)
    assert np.array_equal(gtc, e_gtc)


@pytest.mark.parametrize('yx', [False, True], ids=['xyxy', 'yxyx'])
def test_match_matches_reference(dev, yx):
    """both thresholds in one launch, both column orders: flags, match, score and the float64 IoU are exactly the fixture's"""
    fx = _fx()
    rows, counts, gt, gt_counts, difficult = _det_inputs(dev)
    if yx:
        rows = rows[:, :, [1, 0, 3, 2, 4, 5, 6]].contiguous()
    got = M.match_detections(rows, counts, gt, gt_counts, difficult, MC.THRESHOLDS, MC.NUM_DET, truncate=True, yx_order=yx)
    exp = [fx[f'det/{k}'] for k in ('flags', 'match', 'iou', 'score', 'gt_per_class')]
    _assert_match_equal(got, exp, counts)
    f = got[0].cpu().numpy()
    for b in range(rows.shape[0]):                                               # a slot past the count is empty, and only those
        assert (f[:, b, int(counts[b]):] == M.FLAG_EMPTY).all() and (f[:, b, :int(counts[b])] != M.FLAG_EMPTY).all()
    none = M.match_detections(rows, counts, gt, gt_counts, None, MC.THRESHOLDS, MC.NUM_DET, truncate=True, yx_order=yx)     # no `difficult` array: nothing is ignored
    h = MC.host_match(fx['det/rows'], fx['det/counts'], fx['det/gt'], fx['det/gt_counts'], None, MC.THRESHOLDS)
    _assert_match_equal(none, h, counts)


def test_match_truncate(dev):
    """fractional (and negative) coordinates: `truncate` is int() applied on the host; without it the fractional boxes themselves are matched"""
    fx = _fx()
    rows, counts, gt, gt_counts, difficult = _det_inputs(dev)
    g = torch.Generator().manual_seed(5)
    frac = fx['det/rows'].copy()
    frac[..., :4] += (torch.rand(frac[..., :4].shape, generator=g).numpy() * 1.98 - 0.99).astype(np.float32)
    frac[0, 0, :4] = (-0.5, -1.5, 19.99, 19.01)
    host = frac.copy()
    host[..., :4] = np.array([[[float(int(v)) for v in r[:4]] for r in img] for img in frac], np.float32)
    assert (host[..., :4] != np.floor(frac[..., :4])).any()                      # int() is not floor
    a = M.match_detections(torch.from_numpy(frac).to(dev), counts, gt, gt_counts, difficult, MC.THRESHOLDS, MC.NUM_DET, truncate=True)
    b = M.match_detections(torch.from_numpy(host).to(dev), counts, gt, gt_counts, difficult, MC.THRESHOLDS, MC.NUM_DET, truncate=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    exp = MC.host_match(frac, fx['det/counts'], fx['det/gt'], fx['det/gt_counts'], fx['det/difficult'], MC.THRESHOLDS, truncate=True)
    _assert_match_equal(a, exp, counts)
    c = M.match_detections(torch.from_numpy(frac).to(dev), counts, gt, gt_counts, difficult, MC.THRESHOLDS, MC.NUM_DET, truncate=False)
    exp = MC.host_match(frac, fx['det/counts'], fx['det/gt'], fx['det/gt_counts'], fx['det/difficult'], MC.THRESHOLDS, truncate=False)
    _assert_match_equal(c, exp, counts)


def test_match_equal_scores_rank_by_slot(dev):
    """two detections with the same score on one box: the lower slot is ranked first"""
    rows = torch.zeros(1, 4, 7)
    rows[0, :3] = torch.tensor([[10, 10, 50, 50, 0.5, 1.0, 2], [11, 10, 50, 50, 1.0, 0.5, 2], [10, 10, 50, 49, 0.75, 1.0, 2]])
    gt = torch.tensor([[[10, 10, 50, 50, 2.0]]])
    flags = M.match_detections(rows.to(dev), torch.tensor([3], dtype=torch.int32).to(dev), gt.to(dev), torch.tensor([1], dtype=torch.int32).to(dev),
                               None, (0.5,), 3)[0]
    assert flags.cpu().reshape(-1).tolist() == [M.FLAG_FP, M.FLAG_FP, M.FLAG_TP, M.FLAG_EMPTY]
    rows[0, 2, 4] = 0.25
    flags = M.match_detections(rows.to(dev), torch.tensor([3], dtype=torch.int32).to(dev), gt.to(dev), torch.tensor([1], dtype=torch.int32).to(dev),
                               None, (0.5,), 3)[0]
    assert flags.cpu().reshape(-1).tolist() == [M.FLAG_TP, M.FLAG_FP, M.FLAG_FP, M.FLAG_EMPTY]


# ------------------------------------------------------------------------------------------------------------------ AP
def test_detection_ap(dev):
    """three updates of uneven size over the fixture's images: rec / prec per class exactly get_map's, AP and mAP within 1e-12; past the capacity: an error"""
    fx = _fx()
    rows, counts, gt, gt_counts, difficult = _det_inputs(dev)
    ap = M.DetectionAP(MC.NUM_DET, MC.THRESHOLDS, MC.MAX_DET, capacity_images=8, truncate=True, device=dev)
    for lo, hi in ((0, 3), (3, 4), (4, 8)):
        ap.update(rows[lo:hi], counts[lo:hi], gt[lo:hi], gt_counts[lo:hi], difficult[lo:hi])
    with pytest.raises(RuntimeError):
        ap.update(rows[:1], counts[:1], gt[:1], gt_counts[:1], difficult[:1])
    res = ap.compute(score_threshold=0.5)
    assert len(res) == len(MC.THRESHOLDS)
    gtc = fx['det/gt_per_class']
    for t, r in enumerate(res):
        for c in range(MC.NUM_DET):
            if gtc[c] == 0:                                                      # never labelled: left out, as get_map leaves it out
                assert np.isnan(r['ap'][c]) and c not in r['curves']
                continue
            assert np.array_equal(r['curves'][c]['rec'], fx[f'det/t{t}/c{c}/rec']), (t, c)
            assert np.array_equal(r['curves'][c]['prec'], fx[f'det/t{t}/c{c}/prec']), (t, c)
            assert np.array_equal(r['curves'][c]['fp'], fx[f'det/t{t}/c{c}/fp']), (t, c)
            e_ap, e_f1, e_rec, e_prec = fx[f'det/t{t}/c{c}/ap']
            assert abs(r['ap'][c] - e_ap) <= RATIO_TOL
            assert abs(r['f1'][c] - e_f1) <= RATIO_TOL and r['recall'][c] == e_rec and r['precision'][c] == e_prec
        print('threshold', r['iou_threshold'], 'mAP', r['map'], 'reference', fx[f'det/t{t}/map'][0])
        assert abs(r['map'] - fx[f'det/t{t}/map'][0]) <= RATIO_TOL
    ap.reset()
    ap.update(rows, counts, gt, gt_counts, difficult)                            # one update after a reset: the same epoch again
    again = ap.compute()
    assert again[0]['map'] == res[0]['map'] and again[1]['map'] == res[1]['map']


# ------------------------------------------------------------------------------------------------------------------ the whole evaluation
@pytest.mark.gpu
def test_evaluator_matches_host_formulas():
    """EN-GDF-PN-S0 fp32, batch 2 at 320: the four results of `Evaluator` equal the host-side formulas on the outputs of the same forward_detect, copied back.
    `update()` runs under torch's sync debug mode where this build supports it: no device-to-host copy, no synchronisation."""
    from achelous_amd import Achelous
    from achelous_amd.synth import condition_state_dict, make_inputs
    kw = dict(num_det=7, num_seg=9, phi='S0', resolution=320, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
    net = Achelous(**kw).eval()
    net.load_state_dict(condition_state_dict(net.state_dict(), seed=0))
    net = net.cuda()
    x, xr, xp = [t.cuda() for t in make_inputs(2, 1234, resolution=320, pc_channels=5)]
    B, R, D = 2, 320, 100
    # ground truth that the network's own detections overlap: a first pass (also the warm-up of the engine), its boxes jittered
    warm = M.Evaluator(net, 7, 9, 8, iou_thresholds=MC.THRESHOLDS, capacity_images=4)
    g = torch.Generator().manual_seed(3)
    seg_png = torch.randint(0, 10, (B, R, R), generator=g).cuda()
    lane_png = torch.randint(0, 3, (B, R, R), generator=g).to(torch.uint8).cuda()
    pc_lab = torch.randint(0, 8, (B, xp.shape[2]), generator=g).cuda()
    gt0 = torch.zeros(B, 8, 5).cuda()
    cnt0 = torch.zeros(B, dtype=torch.int32).cuda()
    _, (rows_w, _, cnt_w) = warm.update(x, xr, xp, gt0, cnt0, seg_png, lane_png, pc_lab)
    rows_w, cnt_w = rows_w.cpu(), cnt_w.cpu()
    gt = torch.zeros(B, 8, 5)
    gt_counts = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        k = min(int(cnt_w[b]), 6)
        for j in range(k):
            box = torch.floor(rows_w[b, j, :4] * R) + torch.tensor([2.0, -1.0, 3.0, 1.0])
            gt[b, j] = torch.cat([box, rows_w[b, j, 6:7]])
        if k:
            gt[b, k] = gt[b, 0]                                                  # a doubled box
            gt[b, k, 4] = (gt[b, 0, 4] + 1) % 7                                  # of another class
            k += 1
        gt_counts[b] = k
    difficult = torch.zeros(B, 8, dtype=torch.uint8)
    difficult[:, 1] = 1
    ev = M.Evaluator(net, 7, 9, 8, iou_thresholds=MC.THRESHOLDS, capacity_images=4)
    args = (x, xr, xp, gt.cuda(), gt_counts.cuda(), seg_png, lane_png, pc_lab, difficult.cuda())
    torch.cuda.synchronize()
    guarded = False
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            torch.ones(1, device='cuda').item()                                  # the mode must actually refuse a host read on this build
        except RuntimeError:
            guarded = True
    except Exception:
        pass
    try:
        outs, (rows, idx, cnt) = ev.update(*args)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    print('sync debug mode effective:', guarded)
    res = ev.compute()
    det, se, lane, pc = outs
    # host side: the same outputs, copied back
    rows_px = (rows * torch.tensor([R, R, R, R, 1.0, 1.0, 1.0], device='cuda')).cpu().numpy()
    cnt_h = cnt.cpu().numpy()
    print('detections', cnt_h.tolist(), 'boxes', gt_counts.tolist())
    assert cnt_h.sum() > 0
    flags, match, iou, score, gtc = MC.host_match(rows_px, cnt_h, gt.numpy(), gt_counts.numpy(), difficult.numpy(), MC.THRESHOLDS, truncate=True)
    assert np.array_equal(ev.det.flags[:, :B].cpu().numpy(), flags) and np.array_equal(ev.det.match[:B].cpu().numpy(), match)
    assert np.array_equal(ev.det.iou[:B].cpu().numpy(), iou) and np.array_equal(ev.det.score[:B].cpu().numpy(), score)
    assert (flags == M.FLAG_TP).any()
    for t in range(len(MC.THRESHOLDS)):
        exp = M.average_precision(flags[t], score, rows_px[..., 6].astype(np.int64), gtc)
        assert np.array_equal(res['det'][t]['ap'], exp['ap'], equal_nan=True) and res['det'][t]['map'] == exp['map']

    def host_hist(logits, labels, n, axis):
        pred = torch.argmax(logits.float().cpu(), dim=axis).reshape(-1).numpy()
        lab = labels.cpu().reshape(-1).numpy().astype(np.int64)
        k = (lab >= 0) & (lab < n)
        return np.bincount(n * lab[k] + pred[k], minlength=n * n).reshape(n, n)
    for key, logits, labels, n, axis in (('seg', se, seg_png, 9, 1), ('lane', lane, lane_png, 2, 1)):
        h = host_hist(logits, labels, n, axis)
        assert np.array_equal(res[key]['hist'], h), key
        assert np.array_equal(res[key]['iou'], M.per_class_iu(h)) and res[key]['miou'] == float(np.nanmean(M.per_class_iu(h)))
        assert res[key]['accuracy'] == float(M.per_Accuracy(h))
    h = host_hist(pc, pc_lab, 8, -1)
    assert np.array_equal(ev.pc.hist.cpu().numpy(), h)
    ious, miou = M.mean_iou(h)
    assert np.array_equal(res['pc'][0], ious, equal_nan=True) and (res['pc'][1] == miou or (np.isnan(miou) and np.isnan(res['pc'][1])))
