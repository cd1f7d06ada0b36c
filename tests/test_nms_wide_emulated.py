"""The wide device NMS (csrc/k_nmswide.h, more than 4096 anchors: 448 x 448 .. 864 x 864) compiled for the host (tests/hostemu) and run
through the C ABI on CPU memory: kept anchors, rows and counts equal oracle.achelous_oracle.non_max_suppression in every slot, for the
cases of tests/nms_wide_cases.py.  `all_864` (15309 candidates, 240 suppression rounds) takes the emulator 1.4 s and the oracle 0.4 s, so it runs here as well as
on the GPU (tests/test_gpu_nms_wide.py)."""
import numpy as np
import pytest
import torch

import nms_wide_cases as W
from achelous_amd.engine import DTYPE_F32, NativeEngine
from emu_util import emu_library
from oracle.nms import batched_nms_np

EMU_CASES = list(W.CASES)


def _handle(res, C):
    return NativeEngine(emu_library(), num_det=C, num_seg=1, phi='S0', backbone='en', resolution=res, pc_channels=3, pc_classes=1,
                        num_points=16, nano_head=True, spp=True, dtype=DTYPE_F32)


def _run(c):
    h = _handle(c['res'], c['C'])
    dec = torch.from_numpy(np.array(c['dec']))
    B, md = dec.shape[0], c['max_det']
    # poisoned outputs and workspace: every slot has to be written, nothing may be read before it is
    rows, idx, cnt = torch.full((B, md, 7), 7.5), torch.full((B, md), 123, dtype=torch.int32), torch.full((B,), 77, dtype=torch.int32)
    ws = torch.full((h.nms_workspace_bytes(B),), 0xA5, dtype=torch.uint8)
    h.nms(B, dec, c['conf'], c['iou'], md, rows, idx, cnt, ws)
    return rows, idx, cnt


@pytest.mark.parametrize('name', EMU_CASES)
def test_emulated_wide_nms_equals_oracle(name):
    c = W.case(name)
    assert c['dec'].shape[1] == W.anchors(c['res']) > 4096
    W.check(name, *_run(c))


def test_case_table_sets_the_candidate_counts_it_names():
    assert W.candidates('past4096') == [4116] and W.candidates('rule_5000') == [5000] and W.candidates('rule_5001') == [5001]
    assert W.candidates('cross_5000') == [5000] and W.candidates('cross_5001') == [5001] and W.candidates('mixed_batch') == [5001, 40, 0]
    assert W.candidates('sparse_tail') == [60] and W.candidates('all_864') == [W.MAX_ANCHORS] and W.candidates('ties') == [4116]
    assert W.expected('sparse_tail')[1][0, 0] >= 14580 and 0 < W.expected('sparse_tail')[2][0] < 60      # some of the 60 are suppressed
    ties = W.case('ties')['dec'][0]
    assert len(np.unique(ties[:, 4] * ties[:, 5])) == 8
    assert 0 < W.expected('nan_cls')[2][0] and W.candidates('nan_cls')[0] < 3000
    assert W.expected('max_det_cut')[2][0] == 50 and W.expected('rule_5000')[2][0] > 50


@pytest.mark.parametrize('name', ['cross_5000', 'cross_5001'])
def test_cross_class_pair_tells_the_two_rules_apart(name):
    """On the cross-class input the coordinate trick and the per-class form keep different lists (the pair's second box falls under the trick only), so the
    exact match of test_emulated_wide_nms_equals_oracle shows which rule ran at 5000 and at 5001 candidates."""
    c = W.case(name)
    d = c['dec'][0]
    score = d[:, 4] * d[:, 5:].max(1)
    sel = np.where(score >= np.float32(c['conf']))[0]
    boxes = np.stack([d[sel, 0] - d[sel, 2] / np.float32(2), d[sel, 1] - d[sel, 3] / np.float32(2), d[sel, 0] + d[sel, 2] / np.float32(2), d[sel, 1] + d[sel, 3] / np.float32(2)], 1)
    cid = d[sel, 5:].argmax(1)
    trick = sel[batched_nms_np(boxes, score[sel], cid, c['iou'], variant='trick')]
    vanilla = sel[batched_nms_np(boxes, score[sel], cid, c['iou'], variant='vanilla')]
    first, second = W.CROSS_PAIR
    assert first in trick and second not in trick and first in vanilla and second in vanilla
    assert not np.array_equal(trick, vanilla)
    want = trick if name == 'cross_5000' else vanilla
    assert np.array_equal(W.expected(name)[1][0, :len(want)], want) and W.expected(name)[2][0] == len(want)


def test_more_than_15309_anchors_are_refused_with_nothing_written():
    h = _handle(896, 7)                                   # 16464 anchors
    A = W.anchors(896)
    assert A > W.MAX_ANCHORS
    dec = torch.from_numpy(np.random.default_rng(0).uniform(0.1, 0.9, (1, A, 12)).astype(np.float32))
    rows, idx, cnt = torch.full((1, A, 7), 7.5), torch.full((1, A), 123, dtype=torch.int32), torch.full((1,), 77, dtype=torch.int32)
    ws = torch.full((max(h.nms_workspace_bytes(1), 1 << 20),), 0xA5, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match='15309'):
        h.nms(1, dec, 0.2, 0.45, A, rows, idx, cnt, ws)
    assert bool((rows == 7.5).all()) and bool((idx == 123).all()) and int(cnt[0]) == 77 and bool((ws == 0xA5).all())
