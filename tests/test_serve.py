"""Serving a ragged batch (achelous_amd/prepost.py seg_maps_frames / correct_boxes_frames / detect_frames; csrc/k_serve.h, C ABI ach_seg_overlay_frames and
ach_correct_boxes_frames): B frames of different sizes in one call, both class maps and the overlay image at every frame's own size.

Every kernel case runs once under the emulation library (`-m "not gpu"`) and once on the MI355X (`-m gpu`), as tests/test_metrics.py does.  Everything here is held
EXACTLY: the class maps are the fp32 operation sequence of the shipped per-shape kernel and of oracle/prepost.py on the very probabilities the kernel read (so an
ulp of the device's expf is not this test's business), the overlay is PIL's own Image.blend / ImageEnhance.Brightness on those class maps (tests/serve_cases.py), the
boxes are the reference's recorded vectors."""
import os

import numpy as np
import pytest
import torch

import serve_cases as SC
from achelous_amd import data as D
from achelous_amd import prepost as P
from golden_util import GOLDEN_DIR

SENTINEL, TAIL = 0xA5, 64
CONFIGS = [pytest.param(('cpu', torch.float32), id='emu-f32'), pytest.param(('cuda', torch.float32), id='gpu-f32', marks=pytest.mark.gpu),
           pytest.param(('cuda', torch.bfloat16), id='gpu-bf16', marks=pytest.mark.gpu), pytest.param(('cuda', torch.float16), id='gpu-f16', marks=pytest.mark.gpu)]
DEVICES = [pytest.param(('cpu', torch.float32), id='emu'), pytest.param(('cuda', torch.float32), id='gpu', marks=pytest.mark.gpu)]
_FULL = {}


def _use(dev):
    if dev == 'cpu':
        from emu_util import emu_library
        P._pass_lib.test_library = emu_library()


@pytest.fixture(params=CONFIGS)
def cfg(request):
    """('cpu', dtype): the kernels under the emulation library; ('cuda', dtype): the HIP kernels"""
    _use(request.param[0])
    try:
        yield request.param
    finally:
        P._pass_lib.test_library = None


@pytest.fixture(params=DEVICES)
def dev(request):
    _use(request.param[0])
    try:
        yield request.param[0]
    finally:
        P._pass_lib.test_library = None


def _sentinel_arenas(dev, names=('semantic', 'waterline', 'overlay')):
    _, _, mbytes, _, _, obytes = P.frames_layout(SC.SHAPES)
    size = {'semantic': mbytes, 'waterline': mbytes, 'overlay': obytes}
    return {n: torch.full((size[n] + TAIL,), SENTINEL, dtype=torch.uint8, device=dev) for n in names}, size


def _call(dev, dtype, **kw):
    se, lane = SC.logits()
    arena = D.pack_arena(SC.images(), 3, dev, 'serve_test')
    return P.seg_maps_frames(torch.from_numpy(se).to(dev).to(dtype), torch.from_numpy(lane).to(dev).to(dtype), SC.SHAPES, kw.pop('arena', arena), **kw)


def _np(views):
    return [v.cpu().numpy() for v in views]


def _full(dev, dtype):
    """ONE full call per (device, dtype), shared by the tests below and left unchanged: default palettes, every output, sentinel-filled arenas with a tail, and the
    probability workspaces the kernel read"""
    key = (dev, dtype)
    if key not in _FULL:
        out, size = _sentinel_arenas(dev)
        ws = (torch.empty(SC.B * SC.C_SE * SC.R * SC.R, device=dev), torch.empty(SC.B * 2 * SC.R * SC.R, device=dev))
        r = _call(dev, dtype, workspaces=ws, out=out)
        _FULL[key] = dict(sem=_np(r['semantic']), line=_np(r['waterline']), ovl=_np(r['overlay']), arenas={n: a.cpu().numpy() for n, a in r['arenas'].items()}, size=size,
                          prob_se=ws[0].cpu().numpy().reshape(SC.B, SC.C_SE, SC.R, SC.R), prob_line=ws[1].cpu().numpy().reshape(SC.B, 2, SC.R, SC.R))
    return _FULL[key]


# ------------------------------------------------------------------------------------------------------------------ 1, 2: class maps
def test_class_maps_match_the_oracle_on_the_probabilities_the_kernel_read(cfg):
    dev, dtype = cfg
    fx = _full(dev, dtype)
    total = 0
    for b, (h, w) in enumerate(SC.SHAPES):
        for got, prob in ((fx['sem'][b], fx['prob_se'][b]), (fx['line'][b], fx['prob_line'][b])):
            want = SC.class_map_from_probabilities(prob, h, w)
            bad = int((got != want).sum())
            print(dev, dtype, (h, w), 'differing pixels', bad, 'of', want.size)
            assert got.shape == want.shape and bad == 0, ((h, w), bad)
            total += want.size
    assert total == 2 * sum(h * w for h, w in SC.SHAPES)
    if dtype == torch.float32 and dev == 'cpu':                       # the emulation's expf is libm's: the oracle run from the logits agrees too
        se, lane = SC.logits()
        for b, (h, w) in enumerate(SC.SHAPES):
            assert np.array_equal(fx['sem'][b], SC.O.seg_class_map_original(se[b], h, w)) and np.array_equal(fx['line'][b], SC.O.seg_class_map_original(lane[b], h, w))


def test_class_maps_match_the_shipped_per_shape_kernel(cfg):
    dev, dtype = cfg
    fx = _full(dev, dtype)
    se, lane = SC.logits()
    hnd = P._frames_handle(torch.empty(0, device=dev), SC.R, dtype)
    for name, x in (('sem', se), ('line', lane)):
        t = torch.from_numpy(x).to(dev).to(dtype)
        C = t.shape[1]
        for b, (h, w) in enumerate(SC.SHAPES):
            ws = torch.empty(C * SC.R * SC.R, device=dev)
            out = torch.empty(1, h, w, dtype=torch.uint8, device=dev)
            hnd.seg_resize_argmax(1, C, t[b:b + 1].contiguous(), h, w, ws, out)
            assert np.array_equal(fx[name][b], out[0].cpu().numpy()), (name, (h, w))


# ------------------------------------------------------------------------------------------------------------------ 3: overlay
def _check_overlay(got, fx, keep, blend, brightness):
    pal_se, pal_line = SC.palettes()
    for b, img in enumerate(SC.images()):
        want = SC.overlay(img, fx['sem'][b], fx['line'][b], pal_se, pal_line, keep, blend, brightness)
        assert got[b].shape == want.shape and np.array_equal(got[b], want), (SC.SHAPES[b], keep, blend, brightness, int((got[b] != want).sum()))


def test_overlay_is_pils_blend_and_nothing_outside_a_frame_is_written(cfg):
    dev, dtype = cfg
    fx = _full(dev, dtype)
    _check_overlay(fx['ovl'], fx, None, (0.45, 0.3), 1.3)
    for name, a in fx['arenas'].items():
        assert a.size == fx['size'][name] + TAIL and (a[fx['size'][name]:] == SENTINEL).all(), name      # the bytes after the last frame


# keep_classes x brightness x blend factors; the default combination (None, 1.3, (0.45, 0.3)) is the shared full call above
OPTIONS = [(k, br, bl) for k in (None, (0, 8)) for br in (1.3, None) for bl in ((0.45, 0.3), (0.0, 1.0))][1:]


@pytest.mark.parametrize('keep,brightness,blend', OPTIONS, ids=[f"keep{'all' if k is None else '08'}-b{br}-blend{bl[0]}_{bl[1]}" for k, br, bl in OPTIONS])
def test_overlay_options(dev, keep, brightness, blend):
    fx = _full(dev, torch.float32)
    r = _call(dev, torch.float32, keep_classes=keep, brightness=brightness, blend=blend, want=('overlay',))
    assert set(r) == {'arenas', 'overlay'}
    _check_overlay(_np(r['overlay']), fx, keep, blend, brightness)


# ------------------------------------------------------------------------------------------------------------------ 4: optional outputs
def test_each_output_alone_gives_the_same_bytes(cfg):
    dev, dtype = cfg
    fx = _full(dev, dtype)
    for name, key in (('semantic', 'sem'), ('waterline', 'line'), ('overlay', 'ovl')):
        out, size = _sentinel_arenas(dev, (name,))
        r = _call(dev, dtype, want=(name,), out=out)
        assert set(r) == {'arenas', name}
        assert all(np.array_equal(a, b) for a, b in zip(_np(r[name]), fx[key])), name
        assert (r['arenas'][name][size[name]:] == SENTINEL).all()
    r = _call(dev, dtype, arena=None)                                    # no image arena: class maps only
    assert set(r) == {'arenas', 'semantic', 'waterline'}
    assert all(np.array_equal(a, b) for a, b in zip(_np(r['semantic']), fx['sem'])) and all(np.array_equal(a, b) for a, b in zip(_np(r['waterline']), fx['line']))


# ------------------------------------------------------------------------------------------------------------------ 5: palettes
def test_default_palettes_are_the_reference_lists():
    pal_se, pal_line = SC.palettes()
    assert [tuple(c) for c in P.PALETTE_SEG] == pal_se and [tuple(c) for c in P.PALETTE_LINE] == pal_line
    assert len(pal_se) == 22 and pal_line == pal_se[::-1]
    for f in (0.7, 1.0, 1.3, 2.5):                                       # the host-built brightness table is ImageEnhance.Brightness on every byte
        from PIL import Image, ImageEnhance
        ramp = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
        assert np.array_equal(P.brightness_table(f), np.array(ImageEnhance.Brightness(Image.fromarray(ramp)).enhance(f))[0, :, 0]), f


# ------------------------------------------------------------------------------------------------------------------ 6: ragged boxes
def test_ragged_box_correction_matches_the_reference_vectors(dev):
    g = np.load(os.path.join(GOLDEN_DIR, 'prepost.npz'))
    shapes = [(1080, 1920), (720, 405), (1080, 1920)]
    rows = np.zeros((3, 80, 7), np.float32)
    rows[0, :64], rows[1, :64], rows[2, :10] = g['boxes'], g['boxes'], g['boxes'][:10]
    cnt = torch.tensor([64, 64, 10], dtype=torch.int32).to(dev)
    t = torch.from_numpy(rows).to(dev)
    got = P.correct_boxes_frames(t, cnt, (320, 320), shapes, True).cpu().numpy()
    assert np.array_equal(got[0, :64], g['boxes_lb_1080x1920']) and np.array_equal(got[1, :64], g['boxes_lb_720x405']) and np.array_equal(got[2, :10], g['boxes_lb_1080x1920'][:10])
    assert not got[0, 64:].any() and not got[1, 64:].any() and not got[2, 10:].any()
    hnd = P._frames_handle(t, 320, torch.float32)                        # the shipped single-shape kernel (what correct_boxes_device launches), frame by frame
    for lb in (True, False):
        many = P.correct_boxes_frames(t, cnt, (320, 320), shapes, lb).cpu().numpy()
        for b, (h, w) in enumerate(shapes):
            one = torch.empty(1, 80, 7, device=dev)
            hnd.correct_boxes(1, 80, t[b:b + 1].contiguous(), cnt[b:b + 1].contiguous(), h, w, lb, one)
            assert np.array_equal(many[b], one[0].cpu().numpy()), (b, lb)
    plain = P.correct_boxes_frames(t, cnt, (320, 320), shapes, False).cpu().numpy()
    assert np.array_equal(plain[0, :64], g['boxes_plain_1080x1920']) and np.array_equal(plain[2, :10], g['boxes_plain_1080x1920'][:10]) and not plain[2, 10:].any()


# ------------------------------------------------------------------------------------------------------------------ 7: rejections, on the host, before any launch
def test_bad_arguments_are_rejected_before_any_launch(dev):
    se, lane = SC.logits()
    tse, tlane = torch.from_numpy(se).to(dev), torch.from_numpy(lane).to(dev)
    arena = D.pack_arena(SC.images(), 3, dev, 'serve_test')
    out, _ = _sentinel_arenas(dev)

    def untouched():
        return all(bool((a == SENTINEL).all()) for a in out.values())
    past = D.Arena(arena.data, [arena.frames[0]] + [(arena.data.numel() - 16,) + tuple(f[1:]) for f in arena.frames[1:]])       # frames that run past the arena
    with pytest.raises(ValueError, match='passes the image arena'):
        P.seg_maps_frames(tse, tlane, SC.SHAPES, past, out=out)
    with pytest.raises(ValueError, match='one .H, W. per frame'):
        P.seg_maps_frames(tse, tlane, SC.SHAPES[:-1], arena, out=out)
    for bad in ((0, 5), (5, 0), (-3, 4)):
        with pytest.raises(ValueError, match='at least 1'):
            P.seg_maps_frames(tse, tlane, (bad,) + SC.SHAPES[1:], None, out=out)
    with pytest.raises(ValueError, match='palette is shorter'):
        P.seg_maps_frames(tse, tlane, SC.SHAPES, arena, palette_se=P.PALETTE_SEG[:5], out=out)
    with pytest.raises(ValueError, match='palette is shorter'):
        P.seg_maps_frames(tse, tlane, SC.SHAPES, arena, palette_se=P.PALETTE_SEG[:8], keep_classes=(0, 8), out=out)
    with pytest.raises(ValueError, match='palette is shorter'):
        P.seg_maps_frames(tse, tlane, SC.SHAPES, arena, palette_line=P.PALETTE_LINE[:1], out=out)
    with pytest.raises(ValueError, match='blend factors'):
        P.seg_maps_frames(tse, tlane, SC.SHAPES, arena, blend=(1.5, 0.3), out=out)
    with pytest.raises(ValueError, match='window leaves'):
        P.seg_maps_frames(tse, tlane, SC.SHAPES, arena, windows=[(0, 0, SC.R + 1, SC.R)] * SC.B, out=out)
    with pytest.raises(ValueError):
        P.seg_maps_frames(tse, tlane, SC.SHAPES, arena, out={'overlay': out['overlay'][:100]})
    assert untouched()
    rows, cnt = torch.zeros(2, 8, 7, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match='one .H, W. per frame'):
        P.correct_boxes_frames(rows, cnt, (320, 320), [(10, 10)], True)
    with pytest.raises(ValueError, match='at least 1'):
        P.correct_boxes_frames(rows, cnt, (320, 320), [(10, 10), (0, 4)], True)
    # a palette that is long enough for the classes that survive the remap is accepted
    r = P.seg_maps_frames(tse, tlane, SC.SHAPES, arena, palette_se=P.PALETTE_SEG[:1], keep_classes=(0,), want=('overlay',))
    assert len(r['overlay']) == SC.B


# ------------------------------------------------------------------------------------------------------------------ 8: end to end
@pytest.mark.gpu
def test_gpu_detect_frames_matches_the_per_frame_path():
    """detect_frames against the same stages done the old way on the same letterboxed batch: one forward_detect, then per frame correct_boxes_device and
    seg_class_map_original (the engine is deterministic on identical inputs: everything is array_equal)"""
    from achelous_amd import Achelous
    from achelous_amd.postprocess import correct_boxes_device
    from achelous_amd.synth import condition_state_dict, make_inputs
    from golden_util import Golden, ctor_kwargs
    g = Golden('en_s0')
    kw = ctor_kwargs(g.meta)
    m = Achelous(**kw).eval()
    m.load_state_dict(g.calibrate(condition_state_dict(m.state_dict(), seed=g.meta['weight_seed'])), strict=True)
    m = m.cuda()
    shapes = [(90, 160), (160, 90), (120, 120)]
    rng = np.random.default_rng(9)
    frames = []
    for H, W in shapes:
        yy, xx = np.mgrid[0:H, 0:W]
        frames.append(np.clip(127 + 100 * np.sin(xx / 23.0)[..., None] * np.cos(yy[..., None] / 17.0 + np.arange(3)) + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8))
    _, xr, _ = make_inputs(3, 77, resolution=320, pc_channels=kw['pc_channels'])
    radar = (xr * 30.0 - 3.0).float().cuda()
    pts = (torch.randn(3, 512, kw['pc_channels'], generator=torch.Generator().manual_seed(4)) * 3.0).cuda()
    arena = D.pack_arena(frames, 3, 'cuda', 'serve_e2e')
    got = P.detect_frames(m, arena, radar, pts, 0.35, 0.35, True, 100, dtype=torch.float32)
    # the old way
    canvases = D.letterbox_batch(arena, 320, dtype=torch.uint8)
    for b, f in enumerate(frames):                                       # letterbox_batch's own guarantee (tests/test_data.py), asserted only
        assert torch.equal(canvases[b], P.resize_image(torch.from_numpy(f).cuda(), (320, 320), True))
    x = D.letterbox_batch(arena, 320, dtype=torch.float32)
    (det, se, lane, pc), (rows, idx, cnt) = m.forward_detect(x, P.preprocess_input_radar(radar, torch.float32), P.normalize_points(pts, torch.float32), 0.35, 0.35, 100)
    assert torch.equal(got['count'], cnt) and int(cnt.sum()) > 0
    assert torch.equal(got['point_class'], pc.float().argmax(-1))
    pal_se, pal_line = SC.palettes()
    for b, (H, W) in enumerate(shapes):
        assert torch.equal(got['boxes'][b:b + 1], correct_boxes_device(rows[b:b + 1], cnt[b:b + 1], (320, 320), (H, W), True)), b
        sem, line = P.seg_class_map_original(se[b:b + 1], (H, W))[0], P.seg_class_map_original(lane[b:b + 1], (H, W))[0]
        assert torch.equal(got['semantic'][b], sem) and torch.equal(got['waterline'][b], line), b
        want = SC.overlay(frames[b], sem.cpu().numpy(), line.cpu().numpy(), pal_se, pal_line, None, (0.45, 0.3), 1.3)
        assert np.array_equal(got['overlay'][b].cpu().numpy(), want), b
