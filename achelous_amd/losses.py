"""The training losses on the native kernels (csrc/k_loss.h; C ABI `ach_train_yolo_loss`, `ach_train_loss_scale`, `ach_train_seg_loss`).

Behind the reference's own names and signatures: `YOLOLoss` (loss/detection_loss.py:60-411, YOLOX with SimOTA assignment), `CE_Loss`, `Focal_Loss`, `Dice_loss`
(loss/segmentation_loss.py:9-59), plus the fused `SegLoss` a training loop should use and `MultiTaskLoss`, the `loss_fn` of `train_graph.GraphedTrainStep`.
Forward AND gradient are hand-written HIP; nothing reads device memory on the host, so a whole step with its loss can be captured into a graph.  fp32, contiguous;
under `torch.autocast` the inputs are cast to fp32.  No torch-op or CPU fallback: without the HIP library these raise.

Differences to the reference, all deliberate:
  * `YOLOLoss` does NOT modify its inputs (the reference decodes the boxes in place on a view of the head maps, which fails on a leaf tensor).
  * Ties between equal costs (`torch.topk` / `torch.min` leave them unspecified) go to the lowest anchor index, then the lowest box index.
  * A box for which no anchor is a candidate matches nothing (the reference raises).
  * Logits and labels must have the same size (the reference interpolates; the network's outputs are always at label size).
  * Every sum runs in a fixed order: the same inputs give the same bits on every run.
The point-cloud loss is `F.nll_loss` on 16 k log-probabilities: capture-safe as it is, left to torch.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._native import lib as _lib, check as _check, ptr as _p, stream as _stream, f32c as _f32c

MAX_BOXES = 128          # boxes per image (YL_MAXG of k_loss.h)
_MAX_ANCHORS = 5376      # YL_MAXA
_MAX_CLASSES = 16        # SEG_MAXC
_SEG_BLOCKS = 1024


def _amp_forward(fn):
    """custom_fwd(cast_inputs=float32) for 'cuda' autocast regions, whatever spelling this torch has."""
    try:
        return torch.amp.custom_fwd(fn, device_type='cuda', cast_inputs=torch.float32)
    except (AttributeError, TypeError):
        return torch.cuda.amp.custom_fwd(fn, cast_inputs=torch.float32)


def _amp_backward(fn):
    try:
        return torch.amp.custom_bwd(fn, device_type='cuda')
    except (AttributeError, TypeError):
        return torch.cuda.amp.custom_bwd(fn)


# ------------------------------------------------------------------------------------------------------------------ detection
def pack_labels(labels, max_boxes=None, device=None):
    """The reference's list of [n_i, 5] tensors (cx, cy, w, h in input pixels, class) -> (boxes [B, G, 5] fp32, counts [B] int32), the form a graph capture needs.
    Nothing is read from device memory: the counts come from the shapes.  G = `max_boxes` (default: the largest n_i, at least 1), at most MAX_BOXES."""
    ns = [int(t.shape[0]) for t in labels]
    G = max(1, max(ns) if ns else 1) if max_boxes is None else int(max_boxes)
    if G > MAX_BOXES or G < 1:
        raise ValueError(f"pack_labels: 1 <= G <= {MAX_BOXES} boxes per image (got {G})")
    if ns and max(ns) > G:
        raise ValueError(f"pack_labels: an image has {max(ns)} boxes, G = {G}")
    if device is None:
        device = labels[0].device if labels else 'cpu'
    boxes = torch.zeros(len(labels), G, 5, dtype=torch.float32, device=device)
    for b, t in enumerate(labels):
        if ns[b]:
            boxes[b, :ns[b]] = t.to(device=device, dtype=torch.float32)
    return boxes, torch.tensor(ns, dtype=torch.int32).to(device)


class _YoloLossFn(torch.autograd.Function):
    @staticmethod
    @_amp_forward
    def forward(ctx, r0, r1, r2, boxes, counts, num_classes, strides):
        raws = [_f32c(r, 'YOLOLoss') for r in (r0, r1, r2)]
        boxes = _f32c(boxes, 'YOLOLoss boxes')
        if counts.dtype != torch.int32:
            raise TypeError(f"YOLOLoss: counts must be int32 (got {counts.dtype})")
        counts = counts.contiguous()
        B, G = boxes.shape[0], boxes.shape[1]
        C = int(num_classes)
        if boxes.dim() != 3 or boxes.shape[2] != 5 or tuple(counts.shape) != (B,):
            raise ValueError("YOLOLoss: packed labels are boxes [B, G, 5] and counts [B]")
        if G > MAX_BOXES:
            raise ValueError(f"YOLOLoss: at most {MAX_BOXES} boxes per image (got G = {G})")
        for r in raws:
            if r.dim() != 4 or r.shape[0] != B or r.shape[1] != 5 + C:
                raise ValueError(f"YOLOLoss: head maps [B = {B}, 5 + {C}, H, W] expected, got {tuple(r.shape)}")
        hw = [(int(r.shape[2]), int(r.shape[3])) for r in raws]
        A = sum(h * w for h, w in hw)
        if A > _MAX_ANCHORS:
            raise ValueError(f"YOLOLoss: {A} anchors per image, the assignment kernel holds {_MAX_ANCHORS} (inputs up to 512 x 512)")
        lib = _lib(raws[0])
        dev = raws[0].device
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        claim_a, claim_c, claim_i = torch.empty(B, G, 10, **i32), torch.empty(B, G, 10, **f32), torch.empty(B, G, 10, **f32)
        matched, pred_iou, num_fg = torch.empty(B, A, **i32), torch.empty(B, A, **f32), torch.empty(B, **i32)
        grad = torch.empty(B * (5 + C) * A, **f32)
        partial, loss = torch.empty(B * ((A + 255) // 256), **f32), torch.empty(1, **f32)
        _check(lib, lib.lib.ach_train_yolo_loss(_p(raws[0]), _p(raws[1]), _p(raws[2]), _p(boxes), _p(counts), B, C, G, hw[0][0], hw[0][1], hw[1][0], hw[1][1], hw[2][0], hw[2][1],
                                                float(strides[0]), float(strides[1]), float(strides[2]), _p(claim_a), _p(claim_c), _p(claim_i), _p(matched), _p(pred_iou),
                                                _p(num_fg), _p(grad), _p(partial), _p(loss), _stream(raws[0])))
        ctx.save_for_backward(grad)
        ctx.shapes = [tuple(r.shape) for r in raws]
        ctx.mark_non_differentiable(matched, pred_iou, num_fg)
        return loss.view(()), matched, pred_iou, num_fg

    @staticmethod
    @_amp_backward
    def backward(ctx, dloss, _dm, _di, _dn):
        (grad,) = ctx.saved_tensors
        lib = _lib(grad)
        out = torch.empty_like(grad)
        dloss = dloss.to(torch.float32).contiguous()          # bound to a name: a temporary would be freed before the kernel reads it
        _check(lib, lib.lib.ach_train_loss_scale(_p(grad), _p(dloss), _p(out), grad.numel(), _stream(grad)))
        res, o = [], 0
        for shp in ctx.shapes:
            n = shp[0] * shp[1] * shp[2] * shp[3]
            res.append(out[o:o + n].view(shp))
            o += n
        return res[0], res[1], res[2], None, None, None, None


class YOLOLoss(nn.Module):
    """`loss.detection_loss.YOLOLoss`: `forward(inputs, labels)` with `inputs` the three raw head maps [B, 5 + C, H_k, W_k] as `net(...)` returns them in training mode
    (NOT modified) and `labels` the reference's list of [n_i, 5] tensors or the packed `(boxes [B, G, 5] fp32, counts [B] int32)` of `pack_labels`.  Returns the scalar of
    detection_loss.py:71-191, differentiable down to the raw maps.  Five launches forward + backward, no host read.  `fp16` is accepted and changes nothing."""

    def __init__(self, num_classes, fp16=False, strides=(8, 16, 32)):
        super().__init__()
        self.num_classes, self.fp16, self.strides = int(num_classes), fp16, tuple(strides)
        if len(self.strides) != 3:
            raise ValueError("YOLOLoss: three head levels expected")

    def _packed(self, inputs, labels):
        if isinstance(labels, (tuple, list)) and len(labels) == 2 and torch.is_tensor(labels[0]) and labels[0].dim() == 3:
            return labels
        return pack_labels(labels, device=inputs[0].device)

    def forward_with_assignment(self, inputs, labels):
        """(loss, matched [B, A] int32: box index or -1, pred_iou [B, A], num_fg [B] int32); anchors ordered level by level, row-major."""
        if len(inputs) != 3:
            raise ValueError("YOLOLoss: three head maps expected")
        boxes, counts = self._packed(inputs, labels)
        return _YoloLossFn.apply(inputs[0], inputs[1], inputs[2], boxes, counts, self.num_classes, self.strides)

    def forward(self, inputs, labels=None):
        return self.forward_with_assignment(inputs, labels)[0]


# ------------------------------------------------------------------------------------------------------------------ segmentation
_LABEL_KIND = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
_MODE_CE, _MODE_FOCAL, _MODE_NONE = 0, 1, 2


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    @_amp_forward
    def forward(ctx, logits, png, weights, mode, dice, alpha, gamma, beta, smooth):
        x = _f32c(logits, 'segmentation loss')
        if x.dim() != 4 or png.dim() != 3:
            raise ValueError("segmentation loss: logits [B, C, H, W] and labels [B, H, W] expected")
        B, C, H, W = x.shape
        if tuple(png.shape) != (B, H, W):
            raise ValueError(f"segmentation loss: logits {tuple(x.shape)} and labels {tuple(png.shape)} differ in size (the reference interpolates; the network's "
                             f"outputs are always at label size, so this is an error here)")
        if C > _MAX_CLASSES:
            raise ValueError(f"segmentation loss: at most {_MAX_CLASSES} classes (got {C})")
        if png.dtype not in _LABEL_KIND:
            raise TypeError(f"segmentation loss: labels must be int64, int32 or uint8 (got {png.dtype})")
        png = png.contiguous()
        w = None
        if mode != _MODE_NONE:
            w = _f32c(torch.as_tensor(weights, device=x.device), 'class weights')
            if w.numel() != C:
                raise ValueError(f"segmentation loss: {C} class weights expected, got {w.numel()}")
        lib = _lib(x)
        partial = torch.empty(_SEG_BLOCKS * (2 + 3 * C), dtype=torch.float32, device=x.device)
        stats = torch.empty(2 + 2 * C, dtype=torch.float32, device=x.device)
        cfg = (_LABEL_KIND[png.dtype], B, C, H * W, int(mode), int(bool(dice)), float(alpha), float(gamma), float(beta), float(smooth))
        _check(lib, lib.lib.ach_train_seg_loss(_p(x), _p(png), cfg[0], _p(w), *cfg[1:], _p(partial), _p(stats), _p(None), _p(None), _stream(x)))
        ctx.save_for_backward(x, png, w, partial, stats) if w is not None else ctx.save_for_backward(x, png, partial, stats)
        ctx.cfg = cfg
        return stats[0].clone()

    @staticmethod
    @_amp_backward
    def backward(ctx, dloss):
        saved = ctx.saved_tensors
        x, png, w, partial, stats = saved if len(saved) == 5 else (saved[0], saved[1], None, saved[2], saved[3])
        lib = _lib(x)
        dx = torch.empty_like(x)
        dloss = dloss.to(torch.float32).contiguous()
        cfg = ctx.cfg
        _check(lib, lib.lib.ach_train_seg_loss(_p(x), _p(png), cfg[0], _p(w), *cfg[1:], _p(partial), _p(stats), _p(dloss), _p(dx), _stream(x)))
        return dx, None, None, None, None, None, None, None, None


def CE_Loss(inputs, target, cls_weights, num_classes=21):
    """segmentation_loss.py:9-19: class-weighted cross entropy with ignore_index = num_classes, nn.CrossEntropyLoss's weighted mean.  Same sizes only (ValueError otherwise)."""
    return _SegLossFn.apply(inputs, target, cls_weights, _MODE_CE, False, 1.0, 0.0, 1.0, 1e-5)


def Focal_Loss(inputs, target, cls_weights, num_classes=21, alpha=0.5, gamma=2):
    """segmentation_loss.py:22-38: focal loss on the un-reduced weighted CE, mean over ALL pixels (ignored ones included).  Same sizes only (ValueError otherwise)."""
    return _SegLossFn.apply(inputs, target, cls_weights, _MODE_FOCAL, False, 1.0 if alpha is None else alpha, gamma, 1.0, 1e-5)


def Dice_loss(inputs, target, beta=1, smooth=1e-5):
    """segmentation_loss.py:41-59 with the reference's ONE-HOT float target [B, H, W, C + 1] (utils/dataloader.py:122-125 builds it as eye(C + 1)[png]; the label map is
    recovered from it by an arg-max over the last axis, so soft targets are not supported — use `SegLoss`, which takes the label map and never builds the one-hot).
    The last channel is dropped: ignored pixels still add their softmax to the false positives.  Same sizes only (ValueError otherwise)."""
    if target.dim() != 4:
        raise ValueError("Dice_loss: one-hot target [B, H, W, C + 1] expected")
    if tuple(target.shape[1:3]) != tuple(inputs.shape[2:]):
        raise ValueError(f"Dice_loss: logits {tuple(inputs.shape)} and target {tuple(target.shape)} differ in size (the reference interpolates; not supported)")
    return _SegLossFn.apply(inputs, target.argmax(-1), None, _MODE_NONE, True, 1.0, 0.0, beta, smooth)


class SegLoss(nn.Module):
    """`Focal_Loss` (or `CE_Loss`) `+ Dice_loss` in one pass each way: `forward(logits [B, C, H, W], png [B, H, W] int64 / int32 / uint8)` with label C = ignored.  The
    one-hot target is taken from `png` inside the kernel — the float [B, H, W, C + 1] target is never built, uploaded or read.  Two kernels + one reducer per
    forward + backward."""

    def __init__(self, num_classes, cls_weights, focal=True, dice=True, alpha=0.5, gamma=2, beta=1, smooth=1e-5):
        super().__init__()
        self.num_classes, self.focal, self.dice = int(num_classes), bool(focal), bool(dice)
        self.alpha, self.gamma, self.beta, self.smooth = alpha, gamma, beta, smooth
        self.register_buffer('cls_weights', torch.as_tensor(cls_weights, dtype=torch.float32).clone())

    def forward(self, logits, png):
        if logits.shape[1] != self.num_classes:
            raise ValueError(f"SegLoss: {self.num_classes} classes expected, logits have {logits.shape[1]}")
        w = self.cls_weights if self.cls_weights.device == logits.device else self.cls_weights.to(logits.device)
        if self.focal:
            return _SegLossFn.apply(logits, png, w, _MODE_FOCAL, self.dice, 1.0 if self.alpha is None else self.alpha, self.gamma, self.beta, self.smooth)
        return _SegLossFn.apply(logits, png, w, _MODE_CE, self.dice, 1.0, 0.0, self.beta, self.smooth)


# ------------------------------------------------------------------------------------------------------------------ the whole step
class MultiTaskLoss(nn.Module):
    """The scalar utils/utils_fit.py:84-106 trains on: `seg + lane + det (+ pc)` (its `HUncertainty` is re-created every iteration, so its weights are exp(0) = 1).
    `loss_fn` of `train_graph.GraphedTrainStep`: `__call__(outputs, boxes, counts, png, png_w, pc_labels=None)` with `outputs = (det_list, se, lane, pc)` as the
    network returns them, packed detection labels (`pack_labels`), integer label maps, and point labels [B, N] int64 for the `F.nll_loss` of the point-cloud branch."""

    def __init__(self, num_det, num_seg, cls_weights, cls_weights_wl, focal=True, dice=True, alpha=0.5, gamma=2, strides=(8, 16, 32)):
        super().__init__()
        self.det = YOLOLoss(num_det, strides=strides)
        self.seg = SegLoss(num_seg, cls_weights, focal, dice, alpha, gamma)
        self.lane = SegLoss(2, cls_weights_wl, focal, dice, alpha, gamma)

    def forward(self, outputs, boxes, counts, png, png_w, pc_labels=None):
        det, se, lane, pc = outputs
        loss = self.seg(se, png) + self.lane(lane, png_w) + self.det(det, (boxes, counts))
        if pc_labels is not None:
            loss = loss + F.nll_loss(pc.float().permute(0, 2, 1), pc_labels)
        return loss
