#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz and metrics.meta.json by IMPORTING the reference's evaluation functions (read-only) on the CPU.

Runs ONLY where the reference exists (ACHELOUS_REFERENCE, default /root/reference).  Nothing of the reference's program text is stored: the fixtures are the inputs
of the detection case and the results the reference computes on the seeded inputs of tests/metrics_cases.py.
  * utils_seg/utils_metrics.py: `fast_hist`, `per_class_iu`, `per_class_PA_Recall`, `per_class_Precision`, `per_Accuracy` (not `compute_mIoU`: it uses the removed
    `np.int`); utils_seg_pc/utils_metrics.py: `mean_iou`.
  * utils/utils_map.py: `get_map`, run in a temporary directory once per IoU threshold on text files written as utils/callbacks.py:216-217 writes them.  Its
    `import cv2` is satisfied by an empty stub module placed in `sys.modules` (only the animation path, which is off, calls into it).  `voc_ap` and
    `log_average_miss_rate` are wrapped to record, per class, the `rec` / `prec` lists, the cumulative fp counts and the AP.
`get_map` does not expose its per-detection decisions.  Those (match, IoU, flag of every detection) come from tests/metrics_cases.py::host_match, the same
statements per image in Python floats, and are CHECKED here against `get_map`: per class, the detections ranked by score must give exactly its cumulative tp
and fp lists.

Conditions on the detection case, ASSERTED here (they are not tolerances): integer coordinates; scores within a class pairwise distinct after the reference's
6-character truncation and in the same order as before it; at least one repeated match, one difficult match, one IoU exactly equal to each threshold, two identical
ground-truth boxes (an ovmax tie), an image without ground truth, one without detections, counts of 0 and 100, a class detected but never labelled and a class
labelled but never detected.
"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('ACHELOUS_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'tests'), REPO, REF]

import metrics_cases as MC                                                  # noqa: E402


def _reference():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))                  # the stub (docstring)
    from utils import utils_map as UM                                       # the reference (never copied)
    from utils_seg import utils_metrics as SM
    from utils_seg_pc import utils_metrics as PM
    return UM, SM, PM


def gen_confusion(SM, PM, out, meta):
    for name, cfg in MC.CONF_CASES.items():
        logits, quant, labels = MC.make_conf_case(**cfg)
        C, ax = cfg['C'], MC.class_axis(cfg['layout'])
        out[f'conf/{name}/checksum'] = np.array([MC.checksum(logits), MC.checksum(quant), MC.checksum(labels)])
        lab = labels.numpy().reshape(-1)
        ties = {}
        for dkey in MC.DTYPES:
            x = MC.logits_of(logits, quant, dkey).float().numpy()
            pred = np.argmax(x, axis=ax).reshape(-1)
            top = np.sort(x, axis=ax).take([-1, -2], axis=ax)
            ties[dkey] = int((top.take(0, axis=ax) == top.take(1, axis=ax)).sum())
            hist = SM.fast_hist(lab, pred, C)
            out[f'conf/{name}/hist_{dkey}'] = hist.astype(np.int64)
            if dkey == 'f32':
                out[f'conf/{name}/iou'] = SM.per_class_iu(hist)
                out[f'conf/{name}/pa_recall'] = SM.per_class_PA_Recall(hist)
                out[f'conf/{name}/precision'] = SM.per_class_Precision(hist)
                out[f'conf/{name}/accuracy'] = np.array([SM.per_Accuracy(hist)])
                out[f'conf/{name}/miou'] = np.array([np.nanmean(SM.per_class_iu(hist))])
                # the point-cloud formula on a matrix with an ABSENT class (the last one removed from both axes' counts): plain division -> NaN, nanmean
                h2 = hist.copy()
                h2[-1, :] = 0
                h2[:, -1] = 0
                with np.errstate(divide='ignore', invalid='ignore'):
                    ious, miou = PM.mean_iou(h2)
                out[f'conf/{name}/pc_hist'] = h2.astype(np.int64)
                out[f'conf/{name}/pc_ious'] = ious
                out[f'conf/{name}/pc_miou'] = np.array([miou])
        assert ties['bf16'] > 0 and ties['f16'] > 0, (name, ties)            # the 16-bit inputs contain exact ties at the maximum
        meta['conf'][name] = dict(cfg=dict(cfg, shape=list(cfg['shape'])), pixels=int(lab.size), counted=int(((lab >= 0) & (lab < C)).sum()), max_ties=ties)
    # every pixel in one bin
    n, px = 9, 2 * 37 * 41
    out['conf/onebin/hist'] = SM.fast_hist(np.zeros(px, np.int64), np.zeros(px, np.int64), n).astype(np.int64)


def run_get_map(UM, names, rows, counts, gt, gt_counts, difficult, thr):
    """the reference on the case's text files; returns {class index: (rec, prec, fp_cum, ap)} and the mAP"""
    log = {'voc': [], 'fp': []}
    voc, lamr = UM.voc_ap, UM.log_average_miss_rate

    def rec_voc(rec, prec):
        r = voc(rec[:], prec[:])
        log['voc'].append((list(rec), list(prec), r[0]))
        return r

    def rec_lamr(rec, fp, n_images):
        log['fp'].append(np.array(fp).tolist())
        return lamr(rec, fp, n_images)
    UM.voc_ap, UM.log_average_miss_rate = rec_voc, rec_lamr
    path = tempfile.mkdtemp()
    try:
        os.makedirs(path + '/ground-truth')
        os.makedirs(path + '/detection-results')
        for b in range(rows.shape[0]):
            with open(f'{path}/ground-truth/{b:04d}.txt', 'w') as f:
                for g in range(gt_counts[b]):
                    x1, y1, x2, y2, c = gt[b, g]
                    f.write(f'{names[int(c)]} {int(x1)} {int(y1)} {int(x2)} {int(y2)}' + (' difficult' if difficult[b, g] else '') + '\n')
            with open(f'{path}/detection-results/{b:04d}.txt', 'w') as f:
                for i in range(counts[b]):
                    x1, y1, x2, y2, obj, conf, c = rows[b, i]
                    score = str(obj * conf)                                 # numpy float32, as utils/callbacks.py:200,212
                    f.write('%s %s %s %s %s %s\n' % (names[int(c)], score[:6], str(int(x1)), str(int(y1)), str(int(x2)), str(int(y2))))
        with contextlib.redirect_stdout(io.StringIO()):
            mAP = UM.get_map(thr, False, path=path)
    finally:
        shutil.rmtree(path)
        UM.voc_ap, UM.log_average_miss_rate = voc, lamr
    labelled = sorted({int(gt[b, g, 4]) for b in range(rows.shape[0]) for g in range(gt_counts[b]) if not difficult[b, g]})
    assert len(labelled) == len(log['voc']) == len(log['fp'])
    return {c: (np.array(r), np.array(p), np.array(fp, np.float64), float(ap)) for c, (r, p, ap), fp in zip(labelled, log['voc'], log['fp'])}, float(mAP)


def gen_detection(UM, out, meta):
    rows, counts, gt, gt_counts, difficult = MC.make_det_case()
    names = ['c%d' % i for i in range(MC.NUM_DET)]
    B, D, _ = rows.shape
    # ---- conditions on the case
    assert np.array_equal(rows[..., :4], np.trunc(rows[..., :4])) and np.array_equal(gt[..., :4], np.trunc(gt[..., :4]))
    score = rows[..., 4] * rows[..., 5]
    for c in range(MC.NUM_DET):
        s = np.array([score[b, i] for b in range(B) for i in range(counts[b]) if int(rows[b, i, 6]) == c])
        if not len(s):
            continue
        t = np.array([float(str(v)[:6]) for v in s])
        assert len(set(t.tolist())) == len(t), f'class {c}: truncated scores collide'
        assert np.array_equal(np.argsort(-t, kind='stable'), np.argsort(-s.astype(np.float64), kind='stable')), f'class {c}: truncation reorders'
    flags, match, iou, sc, gtc = MC.host_match(rows, counts, gt, gt_counts, difficult, MC.THRESHOLDS, truncate=True)
    assert np.array_equal(sc, score)
    det_cls = {int(rows[b, i, 6]) for b in range(B) for i in range(counts[b])}
    gt_cls = {int(gt[b, g, 4]) for b in range(B) for g in range(gt_counts[b])}
    assert det_cls - gt_cls and gt_cls - det_cls                             # detected-never-labelled and labelled-never-detected
    assert (gt_counts == 0).any() and (counts == 0).any() and (counts == D).any() and gt_counts.max() <= MC.MAX_GT
    assert any(tuple(gt[b, g]) == tuple(gt[b, h]) for b in range(B) for g in range(gt_counts[b]) for h in range(g))       # identical boxes
    for t, thr in enumerate(MC.THRESHOLDS):
        assert (flags[t] == MC.FLAG_IGNORED).any(), 'no difficult match'
        assert (iou == thr).any(), f'no IoU exactly {thr}'
        rep = [(b, i) for b in range(B) for i in range(counts[b]) if flags[t, b, i] == MC.FLAG_FP and iou[b, i] >= thr]
        assert rep, 'no repeated match'
    # ---- the reference, and the per-detection decisions checked against it
    for t, thr in enumerate(MC.THRESHOLDS):
        per_class, mAP = run_get_map(UM, names, rows, counts, gt, gt_counts, difficult, thr)
        assert sorted(per_class) == [c for c in range(MC.NUM_DET) if gtc[c] > 0]
        for c, (rec, prec, fp_cum, ap) in per_class.items():
            sel = [(b, i) for b in range(B) for i in range(counts[b]) if int(rows[b, i, 6]) == c]
            sel.sort(key=lambda bi: -float(score[bi]))
            f = np.array([flags[t, b, i] for b, i in sel])
            assert np.array_equal(np.cumsum(f == MC.FLAG_FP), fp_cum), (thr, c)
            assert np.array_equal(np.cumsum(f == MC.FLAG_TP) / max(gtc[c], 1), rec), (thr, c)
            s = np.array([score[bi] for bi in sel])
            above = np.nonzero(s >= 0.5)[0]
            k = int(above[-1]) if len(above) else 0
            pr = (rec[k], prec[k]) if len(rec) else (0.0, 0.0)
            f1 = pr[0] * pr[1] * 2 / (1 if pr[0] + pr[1] == 0 else pr[0] + pr[1])
            out[f'det/t{t}/c{c}/rec'], out[f'det/t{t}/c{c}/prec'], out[f'det/t{t}/c{c}/fp'] = rec, prec, fp_cum
            out[f'det/t{t}/c{c}/ap'] = np.array([ap, f1, pr[0], pr[1]])
        out[f'det/t{t}/map'] = np.array([mAP])
        meta['det'][f'iou_{thr}'] = dict(mAP=mAP, ap={str(c): v[3] for c, v in per_class.items()}, tp=int((flags[t] == MC.FLAG_TP).sum()),
                                         fp=int((flags[t] == MC.FLAG_FP).sum()), ignored=int((flags[t] == MC.FLAG_IGNORED).sum()))
    for k, v in dict(rows=rows, counts=counts, gt=gt, gt_counts=gt_counts, difficult=difficult, flags=flags, match=match, iou=iou, score=sc, gt_per_class=gtc).items():
        out[f'det/{k}'] = v
    meta['det']['detections'] = int(counts.sum())
    meta['det']['boxes'] = int(gt_counts.sum())


def main():
    UM, SM, PM = _reference()
    out, meta = {}, {'conf': {}, 'det': {}, 'torch': torch.__version__, 'numpy': np.__version__}
    gen_confusion(SM, PM, out, meta)
    gen_detection(UM, out, meta)
    np.savez_compressed(os.path.join(HERE, 'metrics.npz'), **out)
    with open(os.path.join(HERE, 'metrics.meta.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print('wrote metrics.npz:', os.path.getsize(os.path.join(HERE, 'metrics.npz')), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
