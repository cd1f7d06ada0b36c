"""Training batches assembled on the device (achelous_amd/data.py, csrc/k_data.h): batched PIL-exact letterbox of ragged frames, label maps, boxes, points.

Truth is the reference itself: tests/golden/data.npz holds what `utils.dataloader.YoloDataset` + `yolo_dataset_collate_all` return on the seeded inputs of
tests/data_cases.py (gen_data_golden.py; the inputs are regenerated here and checked against a stored checksum), and PIL's own resize + paste for the general
placements.  Every kernel case runs once under the emulation library (`-m "not gpu"`) and once on the MI355X (`-m gpu`).

Bounds: every image, label and box result is an integer result or a single rounding and is held EXACTLY.  The points go through the existing
`normalize_points` kernel and are held to the bound tests/test_prepost.py holds it to (rtol 1e-5, atol 1e-7: fp32 sums of squares against float64)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import data_cases as DC
from achelous_amd import data as D
from achelous_amd import prepost, train_ops

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICES = [pytest.param('cpu', id='emu'), pytest.param('cuda', id='gpu', marks=pytest.mark.gpu)]
_FX = None
_FRAMES = {}


@pytest.fixture(params=DEVICES)
def dev(request):
    """'cpu': the kernels under the emulation library; 'cuda': the HIP kernels"""
    if request.param == 'cpu':
        from emu_util import emu_library
        train_ops._lib.test_library = prepost._pass_lib.test_library = emu_library()
        try:
            yield 'cpu'
        finally:
            train_ops._lib.test_library = prepost._pass_lib.test_library = None
    else:
        yield 'cuda'


def _fx():
    global _FX
    if _FX is None:
        with np.load(os.path.join(HERE, 'golden', 'data.npz')) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def _frames(name):
    if name not in _FRAMES:
        fr = [DC.make_frame(name, i) for i in range(len(DC.BATCHES[name]['frames']))]
        assert np.isclose(DC.checksum(fr), _fx()[f'{name}/checksum'][0], rtol=1e-12, atol=0), 'tests/data_cases.py no longer generates the inputs the fixtures were recorded on'
        _FRAMES[name] = fr
    return _FRAMES[name]


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def _np(t):
    return t.float().cpu().numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ the reference's batch
@pytest.mark.parametrize('name', list(DC.BATCHES))
def test_batch_matches_reference(dev, name):
    """ragged frames (down-scale, portrait, up-scale, tiny, equal size), labels above the class counts, a frame without a water-line map, boxes that leave the image /
    collapse / truncate to width 1 and 2, an empty box list, clouds of 700 / 3 / 40 rows: everything `MultiTaskLoss` and the network take, against the reference"""
    fx, frames, R = _fx(), _frames(name), DC.BATCHES[name]['R']
    idx = fx[f'{name}/indices'].astype(np.int64)
    for label_dtype in (torch.uint8, torch.int64):
        out = D.TrainBatcher(R, DC.NUM_SEG, DC.NUM_POINTS, label_dtype=label_dtype, device=dev)(frames, indices=idx)
        assert out.images.dtype == torch.float32 and out.png.dtype == label_dtype and out.counts.dtype == torch.int32 and out.boxes.dtype == torch.float32
        got, ref = _np(out.images), fx[f'{name}/images']
        print(name, 'image values differing', int((got != ref).sum()), 'of', ref.size)
        assert np.array_equal(got, ref)
        assert np.array_equal(_np(out.png), fx[f'{name}/png']) and np.array_equal(_np(out.png_w), fx[f'{name}/png_w'])
        assert int(out.png.max()) == DC.NUM_SEG and int(out.png_w.max()) == 2
    counts = _np(out.counts)
    assert np.array_equal(counts, fx[f'{name}/counts'])
    boxes, ref = _np(out.boxes), fx[f'{name}/boxes']
    assert boxes.shape == ref.shape
    for b, n in enumerate(counts):                                               # the reference shuffles: a multiset per frame
        assert np.array_equal(_sorted_rows(boxes[b, :n]), _sorted_rows(ref[b, :n])), b
        assert not boxes[b, n:].any()
    assert np.array_equal(_np(out.pc_labels), fx[f'{name}/pc_labels']) and out.pc_labels.dtype == torch.int64
    err = np.abs(_np(out.points) - fx[f'{name}/points']).max()
    print(name, 'points max abs error', err)
    assert out.points.shape == fx[f'{name}/points'].shape and np.allclose(_np(out.points), fx[f'{name}/points'], rtol=1e-5, atol=1e-7)
    assert np.array_equal(_np(out.radar), np.stack([f['radar'] for f in frames]).astype(np.float32))
    missing = [b for b, f in enumerate(frames) if f['png_w'] is None]
    assert all(not _np(out.png_w)[b].any() for b in missing)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_images_16bit_are_one_rounding_of_the_fixture(dev, dtype):
    for name in DC.BATCHES:
        R = DC.BATCHES[name]['R']
        got = D.letterbox_batch([f['image'] for f in _frames(name)], R, dtype=dtype, device=dev).cpu()
        ref = torch.from_numpy(_fx()[f'{name}/images']).to(dtype)
        assert got.dtype == dtype and torch.equal(got.view(torch.int16), ref.view(torch.int16)), name


def test_value_table_is_exact_for_every_byte(dev):
    """a 16 x 16 image holding every byte value in every channel, pasted unscaled: ((v / 255) - mean) / std in float64, rounded once"""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([v, v[::-1].copy(), v.T.copy()], -1)
    x = img.astype(np.float64)
    x /= 255.0
    x -= np.array([0.485, 0.456, 0.406])
    x /= np.array([0.229, 0.224, 0.225])
    ref = np.transpose(x, (2, 0, 1)).astype(np.float32)
    got = D.letterbox_batch([img], 16, dtype=torch.float32, device=dev)
    assert np.array_equal(_np(got)[0], ref)
    for dtype in (torch.bfloat16, torch.float16):
        got = D.letterbox_batch([img], 16, dtype=dtype, device=dev).cpu()
        assert torch.equal(got[0].view(torch.int16), torch.from_numpy(ref).to(dtype).view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ placements, batching
def test_general_placements_match_pil(dev):
    """dx < 0, a window overhanging the right / bottom edge, nw > R, a window wholly outside (all grey, all-zero labels), nw == iw: PIL's own resize + paste"""
    fx = _fx()
    frames = [_frames('r96')[i] for i in DC.PLACEMENT_FRAMES]
    got = D.letterbox_batch([f['image'] for f in frames], 96, placements=DC.PLACEMENTS, dtype=torch.uint8, device=dev)
    for b, p in enumerate(DC.PLACEMENTS):
        assert np.array_equal(_np(got)[b], fx['place/canvas'][b]), p
    png, png_w = D.labels_batch([f['png'] for f in frames], [f['png_w'] for f in frames], 96, DC.NUM_SEG, placements=DC.PLACEMENTS, device=dev)
    assert np.array_equal(_np(png), fx['place/png']) and np.array_equal(_np(png_w), fx['place/png_w'])
    f32 = _np(D.letterbox_batch([f['image'] for f in frames], 96, placements=DC.PLACEMENTS, device=dev))
    lut = np.stack([((np.arange(256) / 255.0) - m) / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]).astype(np.float32)
    for b in range(len(frames)):
        for c in range(3):
            assert np.array_equal(f32[b, c], lut[c][fx['place/canvas'][b, :, :, c]])
    with pytest.raises(ValueError):
        D.letterbox_batch([frames[0]['image']], 96, placements=[(0, 5, 0, 0)], device=dev)


def test_a_frame_does_not_depend_on_its_batch(dev):
    """B = 1 against B = 5 in a permuted order: the same bytes for every output of every frame"""
    frames = _frames('r96') + _frames('r64')
    imgs, png, png_w = [f['image'] for f in frames], [f['png'] for f in frames], [f['png_w'] for f in frames]
    order = [3, 0, 4, 2, 1]
    big = D.letterbox_batch([imgs[i] for i in order], 96, device=dev)
    big_l = D.labels_batch([png[i] for i in order], [png_w[i] for i in order], 96, DC.NUM_SEG, device=dev)
    for slot, i in enumerate(order):
        one = D.letterbox_batch([imgs[i]], 96, device=dev)
        assert torch.equal(one[0], big[slot]), i
        one_l = D.labels_batch([png[i]], [png_w[i]], 96, DC.NUM_SEG, device=dev)
        assert torch.equal(one_l[0][0], big_l[0][slot]) and torch.equal(one_l[1][0], big_l[1][slot]), i


def test_uint8_mode_equals_resize_image(dev):
    """the bytes of the batched path are those of the existing per-image `prepost.resize_image`"""
    for name in DC.BATCHES:
        R = DC.BATCHES[name]['R']
        imgs = [f['image'] for f in _frames(name)]
        got = D.letterbox_batch(imgs, R, dtype=torch.uint8, device=dev)
        assert tuple(got.shape) == (len(imgs), R, R, 3)
        for b, img in enumerate(imgs):
            assert torch.equal(got[b], prepost.resize_image(torch.from_numpy(img).to(dev), (R, R))), (name, b)


def test_entry_calls_do_not_grow_with_the_batch(dev, monkeypatch):
    """one call of each C entry (two image launches, one label launch) and one `normalize_points` per batch, at B = 1 and B = 4"""
    lib = train_ops._lib(torch.empty(1, device=dev))
    calls = {}
    for sym in ('ach_data_letterbox_batch', 'ach_data_labels_batch', 'ach_normalize_points'):
        fn = getattr(lib.lib, sym)

        def counted(*a, _fn=fn, _sym=sym):
            calls[_sym] = calls.get(_sym, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib.lib, sym, counted)
    frames = _frames('r96')
    idx = _fx()['r96/indices'].astype(np.int64)
    for B in (1, 4):
        calls.clear()
        D.TrainBatcher(96, DC.NUM_SEG, DC.NUM_POINTS, device=dev)(frames[:B], indices=idx[:B])
        assert calls == {'ach_data_letterbox_batch': 1, 'ach_data_labels_batch': 1, 'ach_normalize_points': 1}, (B, calls)


def test_python_face_rejects(dev):
    frames = _frames('r96')
    many = dict(frames[0], boxes=np.array([(2 * i % 200, 0, 2 * i % 200 + 20, 100, 0) for i in range(129)]))
    with pytest.raises(ValueError, match='pack_labels'):
        D.TrainBatcher(96, DC.NUM_SEG, DC.NUM_POINTS, device=dev)([many], indices=np.zeros((1, DC.NUM_POINTS), np.int64))
    empty = dict(frames[0], points=np.zeros((0, 5)), point_labels=np.zeros(0, np.int64))
    with pytest.raises(ValueError, match='empty'):
        D.TrainBatcher(96, DC.NUM_SEG, DC.NUM_POINTS, device=dev)([empty], rng=np.random.default_rng(0))
    with pytest.raises(TypeError):
        D.letterbox_batch([frames[0]['image'].astype(np.float32)], 96, device=dev)
    with pytest.raises(TypeError):
        D.TrainBatcher(96, DC.NUM_SEG, label_dtype=torch.int32, device=dev)
    drawn = D.TrainBatcher(96, DC.NUM_SEG, DC.NUM_POINTS, device=dev)(frames[:2], rng=np.random.default_rng(3))          # a Generator instead of indices
    assert np.array_equal(_np(drawn.pc_labels)[0], frames[0]['point_labels'][np.random.default_rng(3).choice(700, DC.NUM_POINTS, replace=True)])


# ------------------------------------------------------------------------------------------------------------------ host-side validation (emulation only)
def _raw_call(table_edit=None, label_edit=None):
    """one 8 x 8 frame to R = 8 through the C entries themselves, the tables built by hand; returns (rc image, rc labels, outputs still untouched)"""
    from emu_util import emu_library
    lib = emu_library()
    arena = torch.zeros(8 * 8 * 3, dtype=torch.uint8)
    larena = torch.zeros(8 * 8, dtype=torch.uint8)
    hb, hk, ks = [t.numpy().reshape(-1) for t in prepost._pil_coeffs(8, 8, 'cpu')[:2]] + [prepost._pil_coeffs(8, 8, 'cpu')[2]]
    nn = np.arange(8, dtype=np.int32)
    tabs = torch.from_numpy(np.concatenate([hb, hk, nn]).astype(np.int32))
    o_k, o_n = hb.size, hb.size + hk.size
    table = torch.tensor([[0, 8, 8, 24, 8, 8, 0, 0, 0, o_k, ks, 0, o_k, ks, 0, 0]], dtype=torch.int64)
    ltable = torch.tensor([[8, 8, 0, 0, 0, 8, 8, 8, o_n, o_n, -1, 0, 0, 0, 0, 0]], dtype=torch.int64)
    if table_edit:
        table[0, table_edit[0]] = table_edit[1]
    if label_edit:
        ltable[0, label_edit[0]] = label_edit[1]
    lut = torch.from_numpy(D.value_table())
    mid = torch.zeros(8 * 3 * 8, dtype=torch.uint8)
    out = torch.full((1, 3, 8, 8), 7.0)
    png, png_w = torch.full((1, 8, 8), 9, dtype=torch.uint8), torch.full((1, 8, 8), 9, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.lib.ach_data_letterbox_batch(p(arena), arena.numel(), p(table), p(table), p(tabs), p(tabs), tabs.numel(), p(lut), 1, 8, p(mid), mid.numel(), p(out), 0, None)
    msg = lib.lib.ach_last_error(None).decode() if rc else ''
    rcl = lib.lib.ach_data_labels_batch(p(larena), larena.numel(), p(ltable), p(ltable), p(tabs), p(tabs), tabs.numel(), 1, 8, 9, p(png), p(png_w), 2, None)
    msgl = lib.lib.ach_last_error(None).decode() if rcl else ''
    return rc, msg, bool((out == 7.0).all()), rcl, msgl, bool((png == 9).all() and (png_w == 9).all())


def test_entries_validate_the_frame_table_before_any_launch():
    """an extent past the arena and a table offset past its buffer: ACH_ERR_INVALID with a message, nothing launched (the outputs keep their fill); the untouched
    tables run"""
    rc, msg, kept, rcl, msgl, keptl = _raw_call()
    assert rc == 0 and rcl == 0 and not kept and not keptl
    for edit in ((1, 9), (0, 16), (3, 25), (2, 9)):                              # H, offset, pitch, W: the frame no longer fits the 192-byte arena
        rc, msg, kept, _, _, _ = _raw_call(table_edit=edit)
        assert rc == -1 and 'arena' in msg and kept, edit
    for edit in ((9, 10 ** 6), (8, 10 ** 6), (12, -1), (11, 10 ** 6), (10, 10 ** 6)):
        rc, msg, kept, _, _, _ = _raw_call(table_edit=edit)
        assert rc == -1 and 'table' in msg and kept, edit
    rc, msg, kept, _, _, _ = _raw_call(table_edit=(8, 2))                        # a shifted bounds table: its entries leave the source axis
    assert rc == -1 and kept
    for edit in ((5, 9), (4, 16), (7, 7)):                                       # H, offset, pitch of the label map
        _, _, _, rcl, msgl, keptl = _raw_call(label_edit=edit)
        assert rcl == -1 and 'arena' in msgl and keptl, edit
    for edit in ((8, 10 ** 6), (9, 10 ** 6), (8, -5)):
        _, _, _, rcl, msgl, keptl = _raw_call(label_edit=edit)
        assert rcl == -1 and 'table' in msgl and keptl, edit
    train_ops._lib.test_library = __import__('emu_util').emu_library()           # and through the Python face: a ValueError
    try:
        bad = D.Arena(torch.zeros(192, dtype=torch.uint8), [(0, 9, 8, 24)])
        with pytest.raises(ValueError, match='arena'):
            D.letterbox_batch(bad, 8, device='cpu')
    finally:
        train_ops._lib.test_library = None


# ------------------------------------------------------------------------------------------------------------------ GPU only
@pytest.mark.gpu
def test_gpu_full_hd_frames():
    """the deployment shape: two 1080 x 1920 frames with label maps to R = 320 (6x antialiased down-scale, 25-tap kernels, 8-row blocks of 5760-byte rows) against
    `oracle.prepost.resize_image` (pinned to PIL in tests/test_prepost.py) and the NEAREST restatement"""
    from oracle import prepost as O
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(2)]
    imgs[1][::2] //= 3
    maps = [rng.integers(0, 14, (1080, 1920)).astype(np.uint8) for _ in range(2)]
    wl = [rng.integers(0, 4, (1080, 1920)).astype(np.uint8), None]
    got = D.letterbox_batch(imgs, 320, dtype=torch.uint8).cpu().numpy()
    for b in range(2):
        ref = O.resize_image(imgs[b], (320, 320), True)
        print('frame', b, 'bytes differing', int((got[b] != ref).sum()))
        assert np.array_equal(got[b], ref)
    png, png_w = D.labels_batch(maps, wl, 320, DC.NUM_SEG)
    nw, nh, dx, dy = DC.letterbox(1920, 1080, 320)
    for b in range(2):
        ref = DC.paste(np.zeros((320, 320), np.uint8), np.minimum(DC.nearest_resize(maps[b], nw, nh), DC.NUM_SEG), dx, dy)
        assert np.array_equal(png[b].cpu().numpy(), ref)
    ref = DC.paste(np.zeros((320, 320), np.uint8), np.minimum(DC.nearest_resize(wl[0], nw, nh), 2), dx, dy)
    assert np.array_equal(png_w[0].cpu().numpy(), ref) and not png_w[1].any()


@pytest.mark.gpu
def test_gpu_batcher_never_synchronises_and_feeds_the_loss():
    """`TrainBatcher(...)(frames)` under torch's sync debug mode (no device-to-host copy, no blocking copy), then its outputs through one `MultiTaskLoss` forward +
    backward on an EN-S0 net at R = 96, batch 3: an integration check, the result is finite"""
    from achelous_amd import Achelous
    from achelous_amd.losses import MultiTaskLoss
    from achelous_amd.synth import condition_state_dict
    frames = _frames('r96')[:3]
    idx = _fx()['r96/indices'].astype(np.int64)[:3]
    batcher = D.TrainBatcher(96, DC.NUM_SEG, DC.NUM_POINTS, device='cuda')
    batcher(frames, indices=idx)                                                 # warm-up: pinned allocations, the engine handle of normalize_points
    torch.cuda.synchronize()
    guarded = False
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            torch.ones(1, device='cuda').item()                                  # the mode must actually refuse a host read on this build
        except RuntimeError:
            guarded = True
        out = batcher(frames, indices=idx)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    print('sync debug mode effective:', guarded)
    assert guarded
    assert np.array_equal(out.images.cpu().numpy(), _fx()['r96/images'][:3])
    kw = dict(num_det=7, num_seg=DC.NUM_SEG, phi='S0', resolution=96, backbone='en', neck='gdf', pc_seg='pn', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
    net = Achelous(**kw)
    net.load_state_dict(condition_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.cuda().train()
    g = torch.Generator().manual_seed(1)
    loss_fn = MultiTaskLoss(7, DC.NUM_SEG, torch.rand(DC.NUM_SEG, generator=g) + 0.5, torch.rand(2, generator=g) + 0.5).cuda()
    loss = loss_fn(net(out.images, out.radar, out.points), out.boxes, out.counts, out.png, out.png_w, out.pc_labels)
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    print('loss', float(loss.detach()))
    assert torch.isfinite(loss) and grads and all(torch.isfinite(g_).all() for g_ in grads)
