"""Case table of the wide device NMS (csrc/k_nmswide.h: 4096 < A <= 15309 anchors, 448 x 448 .. 864 x 864), shared by
tests/test_nms_wide_emulated.py (CPU emulation) and tests/test_gpu_nms_wide.py.

Inputs are synthetic decoded tensors [B, A, 5 + C] made the way test_emulated_nms_more_candidates_than_fit_in_lds makes its own.  An
anchor is a candidate when its objectness lies in [0.5, 1) (class scores in [0.5, 1): score >= 0.25) and not one when its objectness is
0.01 (score < 0.01), so with conf 0.2 the candidate count is exactly the number of chosen anchors.  Expected values come from
oracle.achelous_oracle.non_max_suppression on the CPU, computed once per case.

  past4096      448 (4116)   first size on the wide path; conf 0: 4116 candidates, still the coordinate trick
  rule_5000/1   512 (5376)   exactly 5000 candidates (trick) / exactly 5001 (per class): torchvision's switch at boxes.numel() > 20000
  cross_5000/1  512          the same with one pair of boxes [-50, 50]^2 of classes 0 and 1, nms_thres 0.1: under the trick the offset
                             (51) leaves the pair an IoU of 49^2 / (2 * 100^2 - 49^2) = 0.136, per class they cannot meet
  mixed_batch   512, B = 3   5001 candidates, 40, none: per-image strides and rule choice in one launch
  sparse_tail   864 (15309)  60 candidates, all among the last 729 anchors (>= 14580): the index width
  all_864       864          conf 0, 15309 candidates, max_det = A
  ties          448, C = 1   scores drawn from 8 distinct values: stable order
  nan_cls       448          NaN in some class scores: the anchor is dropped
  max_det_cut   512          more survivors than max_det = 50
"""
import functools

import numpy as np
import torch

from oracle.achelous_oracle import non_max_suppression as o_nms

MAX_ANCHORS = 15309
CASES = ('past4096', 'rule_5000', 'rule_5001', 'cross_5000', 'cross_5001', 'mixed_batch', 'sparse_tail', 'all_864', 'ties', 'nan_cls', 'max_det_cut')
CROSS_PAIR = (100, 2000)            # anchors of the cross-class pair (both among the candidates of cross_*)


def anchors(res):
    return sum((res // s) ** 2 for s in (8, 16, 32))


def _image(rng, A, C, candidates, lo=0.05, hi=0.95, wmin=0.01, wmax=0.08):
    """one image [A, 5 + C]; `candidates`: anchor indices whose score reaches 0.25, or None for all"""
    d = np.zeros((A, 5 + C), np.float32)
    d[:, 0:2] = rng.uniform(lo, hi, (A, 2))
    d[:, 2:4] = rng.uniform(wmin, wmax, (A, 2))
    d[:, 4] = rng.uniform(0.5, 1, A)
    d[:, 5:] = rng.uniform(0.5, 1, (A, C))
    if candidates is not None:
        off = np.ones(A, bool)
        off[candidates] = False
        d[off, 4] = 0.01
    return d


def _cross(d):
    """the pair of CROSS_PAIR: the same box [-50, 50]^2 under class 0 and class 1, the two best scores of the image"""
    for a, c, s in ((CROSS_PAIR[0], 0, 0.99), (CROSS_PAIR[1], 1, 0.98)):
        d[a, 0:4] = (0.0, 0.0, 100.0, 100.0)
        d[a, 4] = 1.0
        d[a, 5:] = 0.1
        d[a, 5 + c] = s
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(res, C, dec float32 [B, A, 5 + C] (read-only), conf, iou, max_det)"""
    rng = np.random.default_rng(CASES.index(name) + 100)
    C, conf, iou, max_det = 7, 0.2, 0.45, None
    if name == 'past4096':
        res, conf = 448, 0.0
        dec = _image(rng, anchors(res), C, None)[None]
    elif name in ('rule_5000', 'rule_5001', 'cross_5000', 'cross_5001'):
        res = 512
        rng = np.random.default_rng(7)                                  # the four share boxes and the candidate order
        perm = np.concatenate([np.array(CROSS_PAIR), np.setdiff1d(rng.permutation(anchors(res)), CROSS_PAIR, assume_unique=True)])
        d = _image(rng, anchors(res), C, perm[:int(name[-4:])])
        if name.startswith('cross'):
            d, iou = _cross(d), 0.1
        dec = d[None]
    elif name == 'mixed_batch':
        res = 512
        A = anchors(res)
        dec = np.stack([_image(rng, A, C, rng.permutation(A)[:5001]), _image(rng, A, C, rng.permutation(A)[:40], 0.4, 0.6, 0.05, 0.15),
                        _image(rng, A, C, np.zeros(0, np.int64))])
    elif name == 'sparse_tail':
        res = 864
        dec = _image(rng, anchors(res), C, 14580 + rng.permutation(729)[:60], 0.4, 0.6, 0.05, 0.15)[None]
    elif name == 'all_864':
        res, conf = 864, 0.0
        dec = _image(rng, anchors(res), C, None)[None]
    elif name == 'ties':
        res, C, conf = 448, 1, 0.0
        d = _image(rng, anchors(res), C, None)
        d[:, 4] = rng.choice(np.linspace(0.5, 0.85, 8).astype(np.float32), anchors(res))
        d[:, 5] = 0.75
        dec = d[None]
    elif name == 'nan_cls':
        res = 448
        A = anchors(res)
        d = _image(rng, A, C, rng.permutation(A)[:3000])
        hit = rng.permutation(A)[:200]
        d[hit, 5 + rng.integers(0, C, 200)] = np.nan                    # class 0 (the running maximum's start) and later classes alike
        dec = d[None]
    elif name == 'max_det_cut':
        res, max_det = 512, 50
        dec = _image(rng, anchors(res), C, rng.permutation(anchors(res))[:3000])[None]
    else:
        raise KeyError(name)
    dec = np.ascontiguousarray(dec, np.float32)
    dec.setflags(write=False)
    return dict(res=res, C=C, dec=dec, conf=conf, iou=iou, max_det=max_det or dec.shape[1])


def candidates(name):
    """candidates per image, counted as the oracle's filter counts them"""
    c = case(name)
    d = c['dec']
    with np.errstate(invalid='ignore'):
        return [int((d[b, :, 4] * d[b, :, 5:].max(1) >= np.float32(c['conf'])).sum()) for b in range(d.shape[0])]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle on the CPU, cut to max_det -> (rows [B, max_det, 7] float32, idx [B, max_det] int32, cnt [B] int32), read-only"""
    c = case(name)
    return expected_of(c['dec'], c['C'], c['conf'], c['iou'], c['max_det'])


def expected_of(dec, C, conf, iou, max_det):
    B = dec.shape[0]
    rows, idx, cnt = np.zeros((B, max_det, 7), np.float32), np.full((B, max_det), -1, np.int32), np.zeros(B, np.int32)
    for b, (r, k) in enumerate(o_nms(torch.from_numpy(np.array(dec)), C, conf, iou)):
        n = min(len(k), max_det)
        rows[b, :n], idx[b, :n], cnt[b] = r[:n], k[:n], n
    for a in (rows, idx, cnt):
        a.setflags(write=False)
    return rows, idx, cnt


def check(name, rows, idx, cnt, want=None):
    """exact: every slot of the three outputs (rows as bit patterns, so zeros and signs count)"""
    e_rows, e_idx, e_cnt = want or expected(name)
    rows, idx, cnt = (np.asarray(t.cpu() if hasattr(t, 'cpu') else t) for t in (rows, idx, cnt))
    assert np.array_equal(cnt, e_cnt), (name, cnt, e_cnt)
    assert np.array_equal(idx, e_idx), (name, 'first difference at', np.argwhere(idx != e_idx)[:3])
    assert np.array_equal(rows.view(np.int32), e_rows.view(np.int32)), name
