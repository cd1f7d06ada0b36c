"""The wide device NMS (csrc/k_nmswide.h: 448 x 448 .. 864 x 864, up to 15309 anchors) on the MI355X: every case of tests/nms_wide_cases.py
through postprocess.nms_device, exact in every output slot against the oracle on the CPU; forward_detect / submit_detect at 448 against the
separate calls and against the oracle NMS of the device's own decoded tensor; the drop-in non_max_suppression at 640."""
import numpy as np
import pytest
import torch

import nms_wide_cases as W
from achelous_amd import Achelous, decode_outputs
from achelous_amd.postprocess import nms_device, non_max_suppression
from achelous_amd.synth import condition_state_dict, make_inputs

pytestmark = pytest.mark.gpu
KW = dict(num_det=7, num_seg=9, phi='S0', resolution=448, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)


@pytest.fixture(scope='module')
def model():
    m = Achelous(**KW).eval()
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=0))
    return m.cuda()


def _inputs(batch, seed, dt):
    return tuple(t.cuda().to(dt) for t in make_inputs(batch, seed, resolution=448, pc_channels=KW['pc_channels']))


def _flat(o):
    return (*o[0], o[1], o[2], o[3])


@pytest.mark.parametrize('name', W.CASES)
def test_wide_nms_equals_oracle(name):
    c = W.case(name)
    rows, idx, cnt = nms_device(torch.from_numpy(np.array(c['dec'])).cuda(), c['C'], c['conf'], c['iou'], c['max_det'])
    W.check(name, rows, idx, cnt)


def test_frame_result_does_not_depend_on_its_batch():
    """image 1 of mixed_batch alone and between two other images: the same bits"""
    c = W.case('mixed_batch')
    dec = torch.from_numpy(np.array(c['dec'])).cuda()
    three = nms_device(dec, c['C'], c['conf'], c['iou'], c['max_det'])
    for b in range(3):
        one = nms_device(dec[b:b + 1].contiguous(), c['C'], c['conf'], c['iou'], c['max_det'])
        assert all(torch.equal(a[b:b + 1], o) for a, o in zip(three, one)), b


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_forward_detect_at_448_equals_the_separate_calls_and_the_oracle(model, dt):
    A = W.anchors(448)
    x, xr, xp = _inputs(2, 31, dt)
    for conf, iou in ((0.05, 0.5), (0.0, 0.6)):
        with torch.no_grad():
            outs, (rows, idx, cnt) = model.forward_detect(x, xr, xp, conf, iou)
            plain = model(x, xr, xp)
        dec = decode_outputs(plain[0], [448, 448])
        r2, i2, c2 = nms_device(dec, KW['num_det'], conf, iou)
        torch.cuda.synchronize()
        assert rows.shape == (2, A, 7) and all(torch.equal(a, b) for a, b in zip(_flat(outs), _flat(plain)))
        assert torch.equal(rows, r2) and torch.equal(idx, i2) and torch.equal(cnt, c2)
        W.check('forward_detect', rows, idx, cnt, W.expected_of(dec.cpu().numpy(), KW['num_det'], conf, iou, A))
        assert int(cnt.min()) > 0


def test_submit_detect_over_two_batches_equals_forward_detect(model):
    batches = [_inputs(2, 40 + i, torch.bfloat16) for i in range(2)]
    with torch.no_grad():
        want = [model.forward_detect(*b, 0.05, 0.5, 100) for b in batches]
        torch.cuda.synchronize()
        first = model.submit_detect(*batches[0], 0.05, 0.5, 100)
        second = model.submit_detect(*batches[1], 0.05, 0.5, 100)
        got = [first.wait(), second.wait()]
        torch.cuda.synchronize()
    for (o1, d1), (o2, d2) in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip((*_flat(o1), *d1), (*_flat(o2), *d2)))
    assert int(want[0][1][2].min()) > 0


def test_drop_in_non_max_suppression_at_640():
    """[K, 7] = (y1, x1, y2, x2 in image pixels, obj, class confidence, class id) per image, K the device count, rows in the oracle's order"""
    A, C = W.anchors(640), 7
    rng = np.random.default_rng(5)
    dec = np.stack([W._image(rng, A, C, rng.permutation(A)[:3000]), W._image(rng, A, C, rng.permutation(A)[:6000])])
    t = torch.from_numpy(dec).cuda()
    got = non_max_suppression(t, C, [640, 640], [640, 640], False, conf_thres=0.2, nms_thres=0.45)
    _, _, cnt = nms_device(t, C, 0.2, 0.45)
    e_rows, e_idx, e_cnt = W.expected_of(dec, C, 0.2, 0.45, A)
    assert np.array_equal(cnt.cpu().numpy(), e_cnt)
    for b in range(2):
        k = int(e_cnt[b])
        assert got[b].shape == (k, 7) and got[b].dtype == np.float32 and k > 0
        assert np.array_equal(got[b][:, 4:], e_rows[b, :k, 4:])
        assert np.allclose(got[b][:, :4], e_rows[b, :k][:, [1, 0, 3, 2]].astype(np.float64) * 640.0, rtol=0, atol=1e-2)
