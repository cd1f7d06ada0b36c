"""The reference's per-epoch evaluation on the native kernels (csrc/k_metrics.h; C ABI `ach_eval_confusion`, `ach_eval_match`).

What the reference does frame by frame on the host — `utils/callbacks.py::EvalCallback` + `utils/utils_map.py::get_map` (detection mAP),
`utils_seg/callbacks.py` + `utils_seg/utils_metrics.py` (mIoU / mPA / accuracy of the two segmentation heads), `utils_seg_pc/utils_metrics.py::mean_iou` (point
cloud) — split in two:
  * per BATCH, on the device, one launch each and no host read: arg-max + confusion matrix (`SegConfusion.update`) and detection-to-ground-truth matching
    (`DetectionAP.update`).  The accumulators stay on the device; `update()` never synchronises.
  * per EPOCH, on the host, in float64 with the reference's formulas: `compute()` (it reads the accumulators back, so it synchronises).
`Evaluator` ties both to one `forward_detect` per batch.  No torch-op or CPU fallback for the per-batch half: without the HIP library these raise.

Not covered: the COCO path (`get_coco_map`, needs pycocotools), the log-average miss rate, plots and files, and the reference's `str(score)[:6]` truncation of
the scores it writes to its text files (it can only reorder detections whose scores agree to four decimals).  NaN logits: the arg-max is unspecified.
"""
import ctypes

import numpy as np
import torch

from ._native import lib as _lib, check as _check, ptr as _p, stream as _stream

MAX_CLASSES = 16         # CONF_MAXN of k_metrics.h
MAX_DET = 1024           # MATCH_MAXD
MAX_BOXES = 128          # MATCH_MAXG
MAX_THRESHOLDS = 10      # MATCH_MAXT
FLAG_EMPTY, FLAG_TP, FLAG_FP, FLAG_IGNORED = 0, 1, 2, 3

_LABEL_KIND = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
_PRED_KIND = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.uint8: 3}


# ------------------------------------------------------------------------------------------------------------------ segmentation
def _confusion(hist, pred, labels, n, layout=None):
    """hist [n, n] int64 += the confusion counts of `pred` against `labels`; one launch, nothing read back."""
    n = int(n)
    if not 1 <= n <= MAX_CLASSES:
        raise ValueError(f"confusion matrix: 1 <= num_classes <= {MAX_CLASSES} (got {n})")
    if pred.dtype not in _PRED_KIND:
        raise TypeError(f"confusion matrix: predictions are fp32 / bf16 / fp16 logits or a uint8 class map (got {pred.dtype})")
    if labels.dtype not in _LABEL_KIND:
        raise TypeError(f"confusion matrix: labels must be int64, int32 or uint8 (got {labels.dtype})")
    if pred.device != hist.device or labels.device != hist.device:
        raise ValueError("confusion matrix: predictions, labels and the accumulator must be on one device")
    kind = _PRED_KIND[pred.dtype]
    if kind == 3:
        if tuple(pred.shape) != tuple(labels.shape) or pred.dim() < 2:
            raise ValueError(f"confusion matrix: class map {tuple(pred.shape)} and labels {tuple(labels.shape)} must have one shape [B, ...]")
        lay = 0
    else:
        if pred.dim() < 3:
            raise ValueError("confusion matrix: logits [B, C, ...] or [B, ..., C] expected")
        first = pred.shape[1] == n and tuple(labels.shape) == (pred.shape[0],) + tuple(pred.shape[2:])
        last = pred.shape[-1] == n and tuple(labels.shape) == tuple(pred.shape[:-1])
        if layout is None:
            if not (first or last):
                raise ValueError(f"confusion matrix: logits {tuple(pred.shape)} with {n} classes do not fit labels {tuple(labels.shape)}")
            lay = 0 if first else 1
        else:
            lay = {'first': 0, 'last': 1}[layout]
            if not (first if lay == 0 else last):
                raise ValueError(f"confusion matrix: logits {tuple(pred.shape)} with {n} classes (channels {layout}) do not fit labels {tuple(labels.shape)}")
    if labels.numel() == 0:
        return
    pred, labels = pred.contiguous(), labels.contiguous()
    B = int(labels.shape[0])
    HW = labels.numel() // B
    lib = _lib(pred)
    _check(lib, lib.lib.ach_eval_confusion(_p(pred), kind, lay, _p(labels), _LABEL_KIND[labels.dtype], B, n, HW, _p(hist), _stream(pred)))


class SegConfusion:
    """The confusion matrix of one segmentation head over an epoch: `update(pred, labels)` per batch (one launch; `pred`: logits [B, C, H, W] / [B, C, HW] or
    [B, points, C] in fp32 / bf16 / fp16 — the arg-max is taken inside the kernel, equal values go to the lowest class — or a uint8 class map of the labels' shape,
    e.g. `prepost.seg_class_map_original`; `labels` int64 / int32 / uint8, counted only where 0 <= label < num_classes), `.hist` the device int64 [n, n]
    (row = label, column = prediction), `compute()` the reference's figures."""

    def __init__(self, num_classes, device='cuda'):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= MAX_CLASSES:
            raise ValueError(f"SegConfusion: 1 <= num_classes <= {MAX_CLASSES} (got {num_classes})")
        self.hist = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=device)

    def reset(self):
        self.hist.zero_()

    def update(self, pred, labels, layout=None):
        """`layout` ('first' / 'last') names the class axis of the logits where the shapes alone leave it open."""
        _confusion(self.hist, pred, labels, self.num_classes, layout)

    def compute(self):
        """utils_seg/utils_metrics.py:47-60 (`np.maximum(..., 1)` denominators) and :103-110 in float64 on the host.  Synchronises."""
        h = self.hist.cpu().numpy()
        iou, pa, pr = per_class_iu(h), per_class_PA_Recall(h), per_class_Precision(h)
        return {'hist': h, 'iou': iou, 'pa_recall': pa, 'precision': pr, 'accuracy': float(per_Accuracy(h)), 'miou': float(np.nanmean(iou)),
                'mpa': float(np.nanmean(pa))}

    def pc_mean_iou(self):
        """utils_seg_pc/utils_metrics.py:6-16: plain division (an absent class gives NaN), `nanmean`.  Synchronises."""
        return mean_iou(self.hist.cpu().numpy())


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def fast_hist(a, b, n):
    """utils_seg/utils_metrics.py:35-44 on the device: labels `a`, predicted classes `b` (integer tensors of one shape) -> int64 [n, n] tensor."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    b = b.to(a.device)
    if a.dtype not in _LABEL_KIND:
        a = a.to(torch.int64)
    if b.dtype != torch.uint8:
        b = b.clamp(0, 255).to(torch.uint8)
    hist = torch.zeros(int(n), int(n), dtype=torch.int64, device=a.device)
    _confusion(hist, b.reshape(1, -1), a.reshape(1, -1), n)
    return hist


def per_class_iu(hist):
    h = _np(hist).astype(np.float64)
    return np.diag(h) / np.maximum(h.sum(1) + h.sum(0) - np.diag(h), 1)


def per_class_PA_Recall(hist):
    h = _np(hist).astype(np.float64)
    return np.diag(h) / np.maximum(h.sum(1), 1)


def per_class_Precision(hist):
    h = _np(hist).astype(np.float64)
    return np.diag(h) / np.maximum(h.sum(0), 1)


def per_Accuracy(hist):
    h = _np(hist).astype(np.float64)
    return np.sum(np.diag(h)) / np.maximum(np.sum(h), 1)


def mean_iou(cf_mtx):
    """utils_seg_pc/utils_metrics.py:6-16 -> (per-class IoU, their nanmean)"""
    h = _np(cf_mtx).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ious = np.diag(h) / (np.sum(h, axis=1) + np.sum(h, axis=0) - np.diag(h))
        return ious, np.nanmean(ious)


# ------------------------------------------------------------------------------------------------------------------ detection
def match_detections(rows, counts, gt_boxes, gt_counts, difficult=None, iou_thresholds=(0.5,), num_classes=1, truncate=True, yx_order=False, out=None):
    """One launch of the match kernel.  rows [B, D, 7] fp32 + counts [B] int32 (as `nms_device` returns them; `yx_order=True`: as `correct_boxes_device` does),
    gt_boxes [B, G, 5] fp32 = (x1, y1, x2, y2, class) + gt_counts [B] int32, difficult [B, G] uint8 or None.
    Returns (flags [T, B, D] uint8, match [B, D] int32, iou [B, D] float64, score [B, D] fp32, gt_per_class [C] int64); `out` supplies the last four (added to /
    written in place)."""
    thr = [float(t) for t in iou_thresholds]
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError(f"match: 1 to {MAX_THRESHOLDS} IoU thresholds (got {len(thr)})")
    if rows.dim() != 3 or rows.shape[2] != 7 or rows.dtype != torch.float32:
        raise ValueError("match: detection rows [B, max_det, 7] fp32 expected")
    B, D = int(rows.shape[0]), int(rows.shape[1])
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 5 or gt_boxes.dtype != torch.float32:
        raise ValueError(f"match: ground truth [B = {B}, G, 5] fp32 expected, got {tuple(gt_boxes.shape)} {gt_boxes.dtype}")
    G = int(gt_boxes.shape[1])
    if D > MAX_DET or G > MAX_BOXES or D < 1 or G < 1:
        raise ValueError(f"match: 1 <= max_det <= {MAX_DET} and 1 <= G <= {MAX_BOXES} (got {D}, {G})")
    if counts.dtype != torch.int32 or gt_counts.dtype != torch.int32 or tuple(counts.shape) != (B,) or tuple(gt_counts.shape) != (B,):
        raise ValueError("match: counts and gt_counts are int32 [B]")
    if difficult is not None and (difficult.dtype != torch.uint8 or tuple(difficult.shape) != (B, G)):
        raise ValueError("match: difficult is uint8 [B, G]")
    dev = rows.device
    rows, counts, gt_boxes, gt_counts = rows.contiguous(), counts.contiguous(), gt_boxes.contiguous(), gt_counts.contiguous()
    difficult = difficult.contiguous() if difficult is not None else None
    flags = torch.empty(len(thr), B, D, dtype=torch.uint8, device=dev)
    if out is None:
        match, iou = torch.empty(B, D, dtype=torch.int32, device=dev), torch.empty(B, D, dtype=torch.float64, device=dev)
        score, gtc = torch.empty(B, D, dtype=torch.float32, device=dev), torch.zeros(int(num_classes), dtype=torch.int64, device=dev)
    else:
        match, iou, score, gtc = out
    lib = _lib(rows)
    thr_c = (ctypes.c_double * len(thr))(*thr)
    _check(lib, lib.lib.ach_eval_match(_p(rows), _p(counts), int(bool(yx_order)), int(bool(truncate)), _p(gt_boxes), _p(difficult), _p(gt_counts), B, D, G,
                                       int(gtc.numel()), ctypes.cast(thr_c, ctypes.c_void_p), len(thr), _p(flags), _p(match), _p(iou), _p(score), _p(gtc),
                                       _stream(rows)))
    return flags, match, iou, score, gtc


def voc_area(rec, prec):
    """The VOC-2012 area under the precision envelope (utils_map.py:95-136) of float64 arrays."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]))


def average_precision(flags, score, cls, gt_per_class, score_threshold=0.5):
    """The per-epoch finalisation of utils_map.py:427-599 for ONE IoU threshold, on the host: flags / score / cls [images, max_det] in image order (numpy),
    gt_per_class [C].  Classes without a non-difficult box are left out (NaN), their detections dropped, as `get_map` does."""
    C = len(gt_per_class)
    flags, score, cls = flags.reshape(-1), score.reshape(-1), cls.reshape(-1)
    ap = np.full(C, np.nan)
    f1, recall, precision = np.full(C, np.nan), np.full(C, np.nan), np.full(C, np.nan)
    curves = {}
    for c in range(C):
        if gt_per_class[c] <= 0:
            continue
        sel = np.nonzero((flags != FLAG_EMPTY) & (cls == c))[0]                    # (image, slot) order
        order = sel[np.argsort(-score[sel].astype(np.float64), kind='stable')]
        tp = np.cumsum(flags[order] == FLAG_TP).astype(np.float64)
        fp = np.cumsum(flags[order] == FLAG_FP).astype(np.float64)
        rec = tp / np.maximum(gt_per_class[c], 1)
        prec = tp / np.maximum(tp + fp, 1)
        ap[c] = voc_area(rec, prec)
        curves[c] = {'rec': rec, 'prec': prec, 'fp': fp, 'score': score[order]}
        f1[c] = recall[c] = precision[c] = 0.0
        if len(order):
            above = np.nonzero(score[order] >= score_threshold)[0]
            k = int(above[-1]) if len(above) else 0                                # utils_map.py:436-441: the LAST detection at or above the threshold
            s = rec[k] + prec[k]
            f1[c], recall[c], precision[c] = rec[k] * prec[k] * 2 / (1 if s == 0 else s), rec[k], prec[k]
    have = ~np.isnan(ap)
    return {'ap': ap, 'map': float(ap[have].mean()) if have.any() else 0.0, 'f1': f1, 'recall': recall, 'precision': precision, 'curves': curves}


class DetectionAP:
    """VOC mAP over an epoch.  `update(rows, counts, gt_boxes, gt_counts, difficult=None)` per batch: one launch of the match kernel, filed at the slab of the
    images seen so far (a host integer) in dense device buffers of `capacity_images` images; nothing is read back.  `compute(score_threshold)` reads them and
    finishes on the host.  `truncate`: the reference's `int()` of the detection coordinates (utils/callbacks.py:216-217); `yx_order`: rows as
    `correct_boxes_device` returns them."""

    def __init__(self, num_classes, iou_thresholds=(0.5,), max_det=100, capacity_images=4096, truncate=True, yx_order=False, device='cuda'):
        self.num_classes, self.max_det, self.capacity = int(num_classes), int(max_det), int(capacity_images)
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.truncate, self.yx_order = bool(truncate), bool(yx_order)
        if not 1 <= len(self.iou_thresholds) <= MAX_THRESHOLDS:
            raise ValueError(f"DetectionAP: 1 to {MAX_THRESHOLDS} IoU thresholds")
        if not 1 <= self.max_det <= MAX_DET:
            raise ValueError(f"DetectionAP: 1 <= max_det <= {MAX_DET}")
        T, N, D = len(self.iou_thresholds), self.capacity, self.max_det
        self.flags = torch.zeros(T, N, D, dtype=torch.uint8, device=device)
        self.match = torch.full((N, D), -1, dtype=torch.int32, device=device)
        self.iou = torch.full((N, D), -1.0, dtype=torch.float64, device=device)
        self.score = torch.zeros(N, D, dtype=torch.float32, device=device)
        self.cls = torch.zeros(N, D, dtype=torch.float32, device=device)
        self.gt_per_class = torch.zeros(self.num_classes, dtype=torch.int64, device=device)
        self.images = 0

    def reset(self):
        self.flags.zero_()
        self.gt_per_class.zero_()
        self.images = 0

    def update(self, rows, counts, gt_boxes, gt_counts, difficult=None):
        B = int(rows.shape[0])
        if rows.dim() != 3 or rows.shape[1] != self.max_det:
            raise ValueError(f"DetectionAP: rows [B, max_det = {self.max_det}, 7] expected, got {tuple(rows.shape)}")
        if self.images + B > self.capacity:
            raise RuntimeError(f"DetectionAP: {self.images} + {B} images exceed capacity_images = {self.capacity}")
        s = slice(self.images, self.images + B)
        flags = match_detections(rows, counts, gt_boxes, gt_counts, difficult, self.iou_thresholds, self.num_classes, self.truncate, self.yx_order,
                                 out=(self.match[s], self.iou[s], self.score[s], self.gt_per_class))[0]
        self.flags[:, s].copy_(flags)
        self.cls[s].copy_(rows[:, :, 6])
        self.images += B

    def compute(self, score_threshold=0.5):
        """Per threshold: per-class AP (NaN: no non-difficult box of that class), mAP over the classes that have one, and F1 / recall / precision at the last
        detection with score >= `score_threshold`.  Synchronises.  One threshold: its dict; several: a list in the order of `iou_thresholds`."""
        n = self.images
        flags, score = self.flags[:, :n].cpu().numpy(), self.score[:n].cpu().numpy()
        cls, gtc = self.cls[:n].cpu().numpy().astype(np.int64), self.gt_per_class.cpu().numpy()
        res = [dict(average_precision(flags[t], score, cls, gtc, score_threshold), iou_threshold=thr) for t, thr in enumerate(self.iou_thresholds)]
        return res[0] if len(res) == 1 else res


# ------------------------------------------------------------------------------------------------------------------ the whole evaluation
class Evaluator:
    """The reference's evaluation configuration (utils/callbacks.py:88-92: confidence 0.05, nms_iou 0.5, 100 boxes) on one `forward_detect` per batch, at NETWORK
    resolution: detection mAP, the confusion matrices of the two segmentation heads and of the point-cloud head.  `update()` copies nothing to the host and does
    not synchronise; `compute()` does.  (Original-size evaluation: `prepost.seg_class_map_original` -> `SegConfusion.update`, `correct_boxes_device` ->
    `DetectionAP(yx_order=True).update`; INTEGRATION.md.)"""

    def __init__(self, net, num_det, num_seg, pc_classes, conf_thres=0.05, nms_thres=0.5, max_det=100, iou_thresholds=(0.5,), capacity_images=4096, device='cuda'):
        self.net, self.conf_thres, self.nms_thres, self.max_det = net, float(conf_thres), float(nms_thres), int(max_det)
        self.det = DetectionAP(num_det, iou_thresholds, max_det, capacity_images, truncate=True, device=device)
        self.seg = SegConfusion(num_seg, device)
        self.lane = SegConfusion(2, device)
        self.pc = SegConfusion(pc_classes, device) if pc_classes else None
        R = float(net.resolution)
        self._to_pixels = torch.tensor([R, R, R, R, 1.0, 1.0, 1.0], dtype=torch.float32).to(device)       # NMS rows are normalised to the network input

    def reset(self):
        for m in (self.det, self.seg, self.lane, self.pc):
            if m is not None:
                m.reset()

    def update(self, images, radar, points, gt_boxes, gt_counts, seg_png, lane_png, pc_labels=None, difficult=None):
        """gt_boxes [B, G, 5] = (x1, y1, x2, y2, class) in pixels of the network input.  Returns what `forward_detect` returned."""
        with torch.no_grad():
            outs, (rows, idx, cnt) = self.net.forward_detect(images, radar, points, self.conf_thres, self.nms_thres, self.max_det)
            self.det.update(rows * self._to_pixels, cnt, gt_boxes, gt_counts, difficult)
            self.seg.update(outs[1], seg_png)
            self.lane.update(outs[2], lane_png)
            if pc_labels is not None and self.pc is not None:
                self.pc.update(outs[3], pc_labels, layout='last')
        return outs, (rows, idx, cnt)

    def compute(self, score_threshold=0.5):
        return {'det': self.det.compute(score_threshold), 'seg': self.seg.compute(), 'lane': self.lane.compute(),
                'pc': self.pc.pc_mean_iou() if self.pc is not None else None}
