"""The checker of tests/test_losses.py: our own batched, mask-based torch statement of the training losses, written from the formulas of the reference
(loss/detection_loss.py:13-57, 71-411; loss/segmentation_loss.py:9-59) on padded [B, G, A] tensors without a host read.  It exists because the reference is not
available where the GPU tests run; `test_checker_matches_reference_fixtures` pins it to results recorded from the reference (tests/golden/loss_*.npz).
It also returns, per image, the three margins that say whether two correct fp32 evaluations of the assignment can disagree."""
import torch
import torch.nn.functional as F


def anchor_grid(hw, strides, device, dtype):
    """x index, y index and stride of every anchor, level by level, row-major (:97-104)."""
    xs, ys, ss = [], [], []
    for (h, w), s in zip(hw, strides):
        yv, xv = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing='ij')
        xs.append(xv.reshape(-1).to(dtype)); ys.append(yv.reshape(-1).to(dtype)); ss.append(torch.full((h * w,), float(s), device=device, dtype=dtype))
    return torch.cat(xs), torch.cat(ys), torch.cat(ss)


def decode(inputs, strides):
    """[B, A, 5 + C]: boxes decoded (:106-108) out of place; objectness and class logits as they are."""
    hw = [tuple(t.shape[2:]) for t in inputs]
    xg, yg, s = anchor_grid(hw, strides, inputs[0].device, inputs[0].dtype)
    o = torch.cat([t.flatten(2).permute(0, 2, 1) for t in inputs], 1)
    xy = (o[..., :2] + torch.stack([xg, yg], -1)) * s[:, None]
    wh = torch.exp(o[..., 2:4]) * s[:, None]
    return torch.cat([xy, wh, o[..., 4:]], -1), (xg, yg, s)


def _pair_iou(gt, pr):
    """:250-273 centre form; gt [B, G, 1, 4], pr [B, 1, A, 4] -> [B, G, A]"""
    tl = torch.max(gt[..., :2] - gt[..., 2:] / 2, pr[..., :2] - pr[..., 2:] / 2)
    br = torch.min(gt[..., :2] + gt[..., 2:] / 2, pr[..., :2] + pr[..., 2:] / 2)
    en = (tl < br).to(gt.dtype).prod(-1)
    ai = (br - tl).prod(-1) * en
    return ai / (gt[..., 2:].prod(-1) + pr[..., 2:].prod(-1) - ai)


@torch.no_grad()
def simota_assign(dec, grid, boxes, counts, num_classes):
    """dec [B, A, 5 + C] decoded, boxes [B, G, 5], counts [B] -> dict(matched [B, A] (-1 = background), pred_iou [B, A], num_fg [B], margins...)."""
    xg, yg, s = grid
    B, A = dec.shape[0], dec.shape[1]
    G = boxes.shape[1]
    dt = dec.dtype
    boxes = boxes.to(dt)
    valid = torch.arange(G, device=dec.device)[None, :] < counts[:, None].long()                       # [B, G]
    xc, yc = ((xg + 0.5) * s)[None, None, :], ((yg + 0.5) * s)[None, None, :]
    gx, gy, gw, gh = (boxes[..., i][:, :, None] for i in range(4))
    in_box = torch.stack([xc - (gx - 0.5 * gw), yc - (gy - 0.5 * gh), (gx + 0.5 * gw) - xc, (gy + 0.5 * gh) - yc], -1).min(-1).values > 0.0
    rad = 2.5 * s[None, None, :]
    in_ctr = torch.stack([xc - (gx - rad), yc - (gy - rad), (gx + rad) - xc, (gy + rad) - yc], -1).min(-1).values > 0.0
    in_box, in_ctr = in_box & valid[:, :, None], in_ctr & valid[:, :, None]
    cand = (in_box | in_ctr).any(1)                                                                    # [B, A]
    pair = valid[:, :, None] & cand[:, None, :]
    iou = _pair_iou(boxes[:, :, None, :4], dec[:, None, :, :4])
    prob = torch.sqrt(torch.sigmoid(dec[..., 5:]) * torch.sigmoid(dec[..., 4:5]))                       # [B, A, C]
    onehot = F.one_hot(boxes[..., 4].long().clamp(0, num_classes - 1), num_classes).to(dt)             # [B, G, C]
    cls = F.binary_cross_entropy(prob[:, None].expand(B, G, A, num_classes), onehot[:, :, None].expand(B, G, A, num_classes), reduction='none').sum(-1)
    cost = cls + 3.0 * -torch.log(iou + 1e-8) + 100000.0 * (~(in_box & in_ctr)).to(dt)
    inf = torch.tensor(float('inf'), device=dec.device, dtype=dt)
    cost = torch.where(pair, cost, inf)
    kk = min(10, A)
    top_iou = torch.where(pair, iou, torch.full_like(iou, -1.0)).topk(kk, dim=2).values.clamp(min=0.0)
    iou_sum = top_iou.sum(2)                                                                            # [B, G]
    dyn_k = iou_sum.int().clamp(min=1)
    srt = cost.topk(min(kk + 1, A), dim=2, largest=False)
    rank = torch.arange(srt.values.shape[2], device=dec.device)[None, None, :]
    sel = (rank < dyn_k[:, :, None]) & torch.isfinite(srt.values) & valid[:, :, None]
    claims = torch.zeros(B, G, A, dtype=torch.bool, device=dec.device)
    claims.scatter_(2, srt.indices, sel)
    nclaim = claims.sum(1)
    multi = nclaim > 1
    amin = cost.argmin(1)                                                                               # over every box of the image (:389)
    matching = torch.where(multi[:, None, :], F.one_hot(amin, G).permute(0, 2, 1).bool(), claims)
    fg = matching.any(1)
    matched = torch.where(fg, matching.int().argmax(1), torch.full_like(amin, -1))
    pred_iou = (matching.to(dt) * torch.where(pair, iou, torch.zeros_like(iou))).sum(1)
    # margins (per image; +inf where there is nothing to decide)
    big = torch.full((B,), float('inf'), device=dec.device, dtype=dt)
    kth = srt.values.gather(2, (dyn_k[:, :, None] - 1).long().clamp(max=srt.values.shape[2] - 1)).squeeze(2)
    nxt = srt.values.gather(2, dyn_k[:, :, None].long().clamp(max=srt.values.shape[2] - 1)).squeeze(2)
    gap = torch.where(valid & torch.isfinite(nxt) & torch.isfinite(kth), nxt - kth, inf)
    frac = torch.where(iou_sum >= 1.0, torch.minimum(iou_sum - iou_sum.floor(), iou_sum.ceil() - iou_sum), 1.0 - iou_sum)
    frac = torch.where((iou_sum == iou_sum.floor()) & (iou_sum >= 1.0), torch.zeros_like(frac), frac)
    frac = torch.where(valid, frac, inf)
    two = cost.topk(min(2, G), dim=1, largest=False).values
    cgap = torch.where(multi & (counts[:, None] > 1), two[:, -1] - two[:, 0], inf) if G > 1 else big[:, None].expand(B, A)
    reaches = (sel & (srt.values > 5e4)).any(2).any(1)
    margin = torch.minimum(torch.minimum(gap.min(1).values, frac.min(1).values), cgap.min(1).values)
    margin = torch.where(reaches, torch.zeros_like(margin), margin)
    return dict(matched=matched.int(), pred_iou=pred_iou, num_fg=fg.sum(1).int(), fg=fg, margin=margin, cost_gap=gap.min(1).values, int_gap=frac.min(1).values,
                contest_gap=cgap.min(1).values, contested=multi.sum(1), reaches_1e5=reaches)


def giou_loss(pred, target):
    """IOUloss(reduction='none', loss_type='giou') (:13-57)"""
    p1, p2 = pred[..., :2] - pred[..., 2:] / 2, pred[..., :2] + pred[..., 2:] / 2
    t1, t2 = target[..., :2] - target[..., 2:] / 2, target[..., :2] + target[..., 2:] / 2
    tl, br = torch.max(p1, t1), torch.min(p2, t2)
    en = (tl < br).to(pred.dtype).prod(-1)
    ai = (br - tl).prod(-1) * en
    au = pred[..., 2:].prod(-1) + target[..., 2:].prod(-1) - ai
    iou = ai / (au + 1e-16)
    ac = (torch.max(p2, t2) - torch.min(p1, t1)).prod(-1)
    giou = iou - (ac - au) / ac.clamp(1e-16)
    return 1 - giou.clamp(min=-1.0, max=1.0)


def detection_loss(inputs, boxes, counts, num_classes, strides=(8, 16, 32)):
    """The scalar of :71-191 from the three raw maps (autograd reaches them) and packed labels; also the assignment."""
    dec, grid = decode(inputs, strides)
    asg = simota_assign(dec.detach(), grid, boxes, counts, num_classes)
    fg, m = asg['fg'], asg['matched'].long().clamp(min=0)
    bt = boxes.to(dec.dtype).gather(1, m[..., None].expand(-1, -1, 5))                                  # [B, A, 5]
    fgf = fg.to(dec.dtype)
    l_iou = (giou_loss(dec[..., :4], bt[..., :4]) * fgf).sum()
    l_obj = F.binary_cross_entropy_with_logits(dec[..., 4], fgf, reduction='none').sum()
    tcls = F.one_hot(bt[..., 4].long().clamp(0, num_classes - 1), num_classes).to(dec.dtype) * asg['pred_iou'][..., None]
    l_cls = (F.binary_cross_entropy_with_logits(dec[..., 5:], tcls, reduction='none').sum(-1) * fgf).sum()
    nfg = fg.sum().clamp(min=1).to(dec.dtype)
    return (5.0 * l_iou + l_obj + l_cls) / nfg, asg


# ------------------------------------------------------------------------------------------------------------------ segmentation
def _weighted_ce(logits, png, w):
    C = logits.shape[1]
    logp = F.log_softmax(logits, 1)
    valid = (png >= 0) & (png < C)
    L = png.long().clamp(0, C - 1)
    wl = w.to(logits.dtype)[L] * valid.to(logits.dtype)
    return -wl * logp.gather(1, L[:, None]).squeeze(1), wl


def ce_loss(logits, png, w):
    ce, wl = _weighted_ce(logits, png, w)
    return ce.sum() / wl.sum()


def focal_loss(logits, png, w, alpha=0.5, gamma=2):
    ce, _ = _weighted_ce(logits, png, w)
    logpt = -ce
    pt = torch.exp(logpt)
    return (-((1 - pt) ** gamma) * (logpt * (1.0 if alpha is None else alpha))).mean()


def dice_loss(logits, png, beta=1, smooth=1e-5):
    C = logits.shape[1]
    p = torch.softmax(logits, 1)
    valid = (png >= 0) & (png < C)
    onehot = F.one_hot(png.long().clamp(0, C - 1), C).permute(0, 3, 1, 2).to(logits.dtype) * valid[:, None].to(logits.dtype)
    tp = (onehot * p).sum((0, 2, 3))
    fp = p.sum((0, 2, 3)) - tp
    fn = onehot.sum((0, 2, 3)) - tp
    score = ((1 + beta ** 2) * tp + smooth) / ((1 + beta ** 2) * tp + beta ** 2 * fn + fp + smooth)
    return 1 - score.mean()


def seg_loss(logits, png, w, focal=True, dice=True, alpha=0.5, gamma=2):
    main = focal_loss(logits, png, w, alpha, gamma) if focal else ce_loss(logits, png, w)
    return main + dice_loss(logits, png) if dice else main
