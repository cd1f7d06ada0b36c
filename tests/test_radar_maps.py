"""Both radar inputs of the network from raw radar point clouds (achelous_amd/data.py radar_maps_batch / radar_points_batch, csrc/k_radarmap.h).

Truth is the reference itself: tests/golden/radar_maps.npz holds what the loop cell of radar_feature_map_generate.ipynb wrote for the seeded clouds of
tests/radar_cases.py (gen_radar_golden.py executes the cell; the clouds are regenerated here and checked against a stored checksum), and next to it the
independent-walk restatement of tests/radar_cases.py.  Every kernel case runs once under the emulation library (`-m "not gpu"`) and once on the MI355X (`-m gpu`).

Bounds: the raw map is a selection of input values, each rounded once to fp32, and is held EXACTLY (NaN for NaN).  The normalised map is held bit for bit to the
existing `preprocess_radar` kernels on the same device, and for fp32 to rtol 1e-6, atol 1e-7 of the float64 rule (the bound tests/test_prepost.py holds that
step to).  Gathered labels are exact; points are held to rtol 1e-5, atol 1e-7 of sklearn's normalize in float64 (the bound of `normalize_points`)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import data_cases as DC
import radar_cases as RC
from achelous_amd import data as D
from achelous_amd import prepost, train_ops
from achelous_amd._native import stateless_handle

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICES = [pytest.param('cpu', id='emu'), pytest.param('cuda', id='gpu', marks=pytest.mark.gpu)]
KINDS = {'f64': np.float64, 'f32': np.float32}
_FX = None
_CLOUDS = {}


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
        with np.load(os.path.join(HERE, 'golden', 'radar_maps.npz')) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def _clouds(name):
    if name not in _CLOUDS:
        c = RC.make_clouds(name)
        assert np.isclose(RC.checksum(c), _fx()[f'{name}/checksum'][0], rtol=1e-12, atol=0), 'tests/radar_cases.py no longer generates the inputs the fixture was recorded on'
        _CLOUDS[name] = c
    return _CLOUDS[name]


def _np(t):
    return t.float().cpu().numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _chunk():
    with open(os.path.join(os.path.dirname(HERE), 'achelous_amd', 'csrc', 'k_radarmap.h')) as f:
        return int(re.search(r'constexpr int RADAR_CHUNK = (\d+);', f.read()).group(1))


# ------------------------------------------------------------------------------------------------------------------ the raw map
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('name', ['r16', 'r20', 'rev16', 'r320', 'r96'])
def test_raw_map_is_the_notebooks(dev, name, kind):
    """clouds of 0 / 1 / 37 / 300 / 2500 points in one call on 16 x 16 and 20 x 20 maps (every cell hit several times: collisions, moves into occupied cells, moves
    from x = 1 to 0, the zero-is-free rule, NaN values), a quarter of the points wrapping or outside, the planted NaN / +-inf / 1e300 / -0.5 / first-out-of-range /
    wrap-to-0 coordinates; R = 320 with image-plane coordinates (the band tiling at the real size); seven-column clouds with the map's columns out of order.
    float64 input, and the same clouds rounded to float32 (the truth then comes from the rounded values)."""
    cfg = RC.CASES[name]
    given, truth_from = RC.as_input(_clouds(name), KINDS[kind])
    cols = RC.map_columns(name)
    got = D.radar_maps_batch(given, cfg['R'], columns=cols, device=dev)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(given), 3, cfg['R'], cfg['R'])
    got = _np(got)
    notebook = _fx()[f'{name}/{kind}/maps'].astype(np.float32)
    restated = RC.rasterise_batch(truth_from, cfg['R'], cols).astype(np.float32)
    print(name, kind, 'cells differing from the notebook', int((~((got == notebook) | (np.isnan(got) & np.isnan(notebook)))).sum()), 'non-zero', int((notebook != 0).sum()))
    assert _same(got, notebook)
    assert _same(got, restated)
    if name in ('r16', 'r20'):
        assert max(cfg['sizes']) > _chunk() and not got[0].any()              # more than one staged chunk; the empty cloud gives a zero map
        assert np.isnan(notebook).any() and (notebook[2:] != 0).mean() > 0.3


def test_order_matters(dev):
    """the same cloud reversed gives the reversed-order truth, and the two truths differ: the walk is sequential, not a scatter"""
    clouds = _clouds('rev16')
    assert np.array_equal(clouds[1], clouds[0][::-1], equal_nan=True)
    truth = RC.rasterise_batch(clouds, 16).astype(np.float32)
    assert not _same(truth[0], truth[1])
    got = _np(D.radar_maps_batch(clouds, 16, device=dev))
    assert _same(got[0], truth[0]) and _same(got[1], truth[1])


def test_a_frame_does_not_depend_on_its_batch_or_its_row_stride(dev):
    """B = 1 against B = 5 in a permuted order; the same clouds as the first five of eight columns (row stride 8)"""
    clouds = _clouds('r20')
    order = [3, 0, 4, 2, 1]
    big = D.radar_maps_batch([clouds[i] for i in order], 20, device=dev)
    wide = D.radar_maps_batch([np.hstack([np.full((len(clouds[i]), 3), 9.0), clouds[i]]) for i in order], 20, columns=(3, 4, 5, 6, 7), device=dev)
    assert _same(_np(big), _np(wide))
    for slot, i in enumerate(order):
        assert _same(_np(D.radar_maps_batch([clouds[i]], 20, device=dev))[0], _np(big)[slot]), i


def test_cell_size_is_an_argument(dev):
    """cell = (3.0, 2.0) on a 20 x 20 map: the restatement with that cell"""
    clouds = _clouds('r16')
    got = _np(D.radar_maps_batch(clouds, 20, cell=(3.0, 2.0), device=dev))
    assert _same(got, RC.rasterise_batch(clouds, 20, cell=(3.0, 2.0)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ the normalised map
def _existing_normalisation(raw, dtype, dev):
    """`prepost.preprocess_input_radar(raw, dtype)`; under the emulation library the same two kernels through that library's engine handle"""
    if dev == 'cuda':
        return prepost.preprocess_input_radar(raw, dtype)
    B, C, R, _ = raw.shape
    out = torch.empty(B, C, R, R, dtype=dtype)
    stateless_handle(1, R, dtype, train_ops._lib.test_library).preprocess_radar(B, C, raw.contiguous(), out)
    return out


@pytest.mark.parametrize('name', ['clean16', 'r320'])
def test_normalised_map_is_the_existing_normalisation_of_the_raw_map(dev, name):
    """bit for bit `preprocess_input_radar(raw, dtype)` on the same device for fp32, bf16 and fp16, and for fp32 within rtol 1e-6, atol 1e-7 of the float64 rule.
    The inputs hold no NaN (min / max with NaN depends on the order of the reduction) and no empty cloud (an all-zero map is 0 / 0)."""
    cfg = RC.CASES[name]
    clouds = _clouds(name)
    assert all(len(c) and not np.isnan(c).any() for c in clouds)
    raw = D.radar_maps_batch(clouds, cfg['R'], device=dev)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        got = D.radar_maps_batch(clouds, cfg['R'], normalize=True, dtype=dtype, device=dev)
        want = _existing_normalisation(raw, dtype, dev)
        assert got.dtype == dtype and got.shape == want.shape
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(got.cpu().view(bits), want.cpu().view(bits)), dtype
        if dtype == torch.float32:
            x = _fx()[f'{name}/f64/maps'].astype(np.float32).astype(np.float64)
            lo, hi = x.min(axis=(1, 2, 3), keepdims=True), x.max(axis=(1, 2, 3), keepdims=True)
            ref = (x - lo) / (hi - lo) + 1e-13
            print(name, 'normalised fp32 max abs error against float64', np.abs(_np(got) - ref).max())
            assert np.allclose(_np(got), ref, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------------ the points
def _normalize64(x):
    """sklearn.preprocessing.normalize(X, axis=0) in float64: a zero column is left as it is"""
    nrm = np.sqrt((x * x).sum(axis=0))
    nrm[nrm == 0] = 1.0
    return x / nrm


@pytest.mark.parametrize('kind', list(KINDS))
def test_points_and_labels(dev, kind):
    """clouds of 700 / 3 / 40 / 17 rows of eight columns (the last all zeros) sampled 64 times each — the cloud of 3 rows holds every row many times —, five point
    columns out of order, the label column between them"""
    lay = RC.CASES['r96']['layout']
    clouds = [np.hstack([c, np.zeros((len(c), 1))]) for c in _clouds('r96')]
    given, truth_from = RC.as_input(clouds, KINDS[kind])
    cols = (0, 7, 5, 6, 2)
    idx = np.stack([np.random.default_rng([5, b]).choice(len(c), RC.NUM_POINTS, replace=True) for b, c in enumerate(clouds)])
    pts, lab = D.radar_points_batch(given, cols, lay['label'], RC.NUM_POINTS, indices=idx, device=dev)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (4, 5, RC.NUM_POINTS) and lab.dtype == torch.int64 and tuple(lab.shape) == (4, RC.NUM_POINTS)
    for b, c in enumerate(truth_from):
        assert np.array_equal(_np(lab)[b], c[idx[b], lay['label']].astype(np.int64)), b
        ref = _normalize64(c[idx[b]][:, list(cols)]).T
        print(kind, 'frame', b, 'points max abs error', np.abs(_np(pts)[b] - ref).max())
        assert np.allclose(_np(pts)[b], ref, rtol=1e-5, atol=1e-7), b
        assert not _np(pts)[b, 1].any()                                          # the all-zero column stays zero (0 / 1, not 0 / 0)
    for dtype in (torch.bfloat16, torch.float16):                                # one rounding of the fp32 result
        p16, _ = D.radar_points_batch(given, cols, None, RC.NUM_POINTS, indices=idx, dtype=dtype, device=dev)
        assert torch.equal(p16.cpu().view(torch.int16), pts.cpu().to(dtype).view(torch.int16)), dtype
    drawn, _ = D.radar_points_batch(given, cols, None, RC.NUM_POINTS, rng=np.random.default_rng(3), device=dev)      # a Generator instead of indices
    again = np.stack([np.random.default_rng(3).choice(700, RC.NUM_POINTS, replace=True)] + [idx[b] for b in (1, 2, 3)])
    assert torch.equal(drawn[0], D.radar_points_batch(given, cols, None, RC.NUM_POINTS, indices=again, device=dev)[0][0])


def test_entry_calls_do_not_grow_with_the_batch(dev, monkeypatch):
    """one call of each C entry per batch (one launch for the raw map, two for the normalised one, one for the points: api_frames.cpp), at B = 1 and B = 4"""
    lib = train_ops._lib(torch.empty(1, device=dev))
    calls = {}
    for sym in ('ach_data_radar_maps', 'ach_data_radar_points', 'ach_preprocess_radar', 'ach_normalize_points'):
        fn = getattr(lib.lib, sym)

        def counted(*a, _fn=fn, _sym=sym):
            calls[_sym] = calls.get(_sym, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib.lib, sym, counted)
    clouds = _clouds('r96')
    for B in (1, 4):
        calls.clear()
        packed = D.pack_clouds(clouds[:B], dev)
        D.radar_maps_batch(packed, 96, columns=RC.map_columns('r96'), normalize=True, device=dev)
        D.radar_points_batch(packed, (0, 3), 1, 16, rng=np.random.default_rng(0), device=dev)
        assert calls == {'ach_data_radar_maps': 1, 'ach_data_radar_points': 1}, (B, calls)


# ------------------------------------------------------------------------------------------------------------------ host-side validation (emulation only)
def _raw_call(edit=None, index=0, column=1):
    """one cloud of 4 rows x 5 columns to R = 8 through the C entries themselves, the table built by hand; returns (rc maps, message, map output untouched, rc points,
    message, point outputs untouched)"""
    from emu_util import emu_library
    lib = emu_library()
    arena = torch.arange(20, dtype=torch.float64)
    table = torch.zeros(1, 16, dtype=torch.int64)
    table[0, :9] = torch.tensor([0, 4, 5, 5, 0, 1, 2, 3, 4])
    if edit:
        table[0, edit[0]] = edit[1]
    raw, part, out = torch.full((1, 3, 8, 8), 7.0), torch.full((16,), 7.0), torch.full((1, 3, 8, 8), 7.0)
    idx = torch.tensor([[0, 3, index]], dtype=torch.int64)
    cols = torch.tensor([0, column], dtype=torch.int32)
    pts, lab = torch.full((1, 2, 3), 7.0), torch.full((1, 3), 7, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.lib.ach_data_radar_maps(p(arena), arena.numel(), 1, p(table), p(table), 1, 8, 6.0, 3.375, p(raw), p(part), part.numel(), p(out), 0, None)
    msg = lib.lib.ach_last_error(None).decode() if rc else ''
    rcp = lib.lib.ach_data_radar_points(p(arena), arena.numel(), 1, p(table), p(table), p(idx), p(idx), p(cols), 2, 2, 1, 3, p(pts), 0, p(lab), None)
    msgp = lib.lib.ach_last_error(None).decode() if rcp else ''
    return rc, msg, bool((raw == 7.0).all() and (out == 7.0).all()), rcp, msgp, bool((pts == 7.0).all() and (lab == 7).all())


def test_entries_validate_the_cloud_table_before_any_launch():
    """an offset + extent that leaves the arena, a column index >= F, a negative n, a row index >= n: ACH_ERR_INVALID with a message, nothing launched (the outputs
    keep their fill); the untouched table runs"""
    rc, msg, kept, rcp, msgp, keptp = _raw_call()
    assert rc == 0 and rcp == 0 and not kept and not keptp
    for edit in ((0, 1), (0, 21), (0, -1), (1, 5), (3, 6), (1, -1), (1, -2 ** 40), (3, 4), (2, 0)):      # offset, n, stride: the cloud no longer fits 20 elements; n < 0
        rc, msg, kept, rcp, msgp, keptp = _raw_call(edit=edit)
        assert rc == -1 and 'arena' in msg and kept and rcp == -1 and 'arena' in msgp and keptp, edit
    for edit in ((4, 5), (8, 5), (6, -1), (7, 2 ** 40), (2, 4)):                                          # a map column at or past F (F = 4 cuts column 4 off)
        rc, msg, kept, rcp, msgp, keptp = _raw_call(edit=edit)
        assert rc == -1 and 'column' in msg and kept and rcp == -1 and keptp, edit
    for kw in (dict(index=4), dict(index=-1), dict(column=5), dict(column=-1)):                           # a sampled row at or past n, a point column at or past F
        rc, _, _, rcp, msgp, keptp = _raw_call(**kw)
        assert rc == 0 and rcp == -1 and ('index' in msgp) and keptp, kw
    _, _, _, rcp, msgp, keptp = _raw_call(edit=(1, 0), index=0)                                           # an empty cloud has nothing to sample
    assert rcp == -1 and keptp
    train_ops._lib.test_library = __import__('emu_util').emu_library()                                    # and through the Python face: a ValueError
    try:
        bad = D.Clouds(torch.zeros(20, dtype=torch.float64), [(0, 5, 5, 5)])
        with pytest.raises(ValueError, match='arena'):
            D.radar_maps_batch(bad, 8, device='cpu')
        with pytest.raises(ValueError, match='column'):
            D.radar_maps_batch([np.zeros((4, 5))], 8, columns=(0, 1, 2, 3, 5), device='cpu')
        with pytest.raises(NotImplementedError):
            D.radar_maps_batch([np.zeros((4, 5))], 2049, device='cpu')
        with pytest.raises(TypeError):
            D.radar_maps_batch([np.zeros((4, 5), np.int32)], 8, device='cpu')
        with pytest.raises(ValueError, match='empty'):
            D.radar_points_batch([np.zeros((0, 5))], (0, 1), None, 8, rng=np.random.default_rng(0), device='cpu')
        with pytest.raises(ValueError, match='indices'):
            D.radar_points_batch([np.zeros((4, 5))], (0, 1), None, 8, indices=np.full((1, 8), 4), device='cpu')
    finally:
        train_ops._lib.test_library = None
    with pytest.raises(RuntimeError):                                                                     # no library, no CPU path
        D.radar_maps_batch([np.zeros((4, 5))], 8, device='cpu')


# ------------------------------------------------------------------------------------------------------------------ TrainBatcher
def test_batcher_on_clouds_equals_the_batch_from_ready_maps(dev):
    """the four frames of tests/data_cases.py 'r96' carrying raw seven-column clouds against the same frames carrying the fixture's maps and the host-sampled
    points: radar, points and point labels are equal, images, label maps and boxes unchanged"""
    lay = RC.CASES['r96']['layout']
    clouds = _clouds('r96')
    frames = [DC.make_frame('r96', i) for i in range(4)]
    idx = np.stack([np.random.default_rng([8, b]).choice(len(c), DC.NUM_POINTS, replace=True) for b, c in enumerate(clouds)])
    mapping = dict(map=lay['map'], points=lay['points'], label=lay['label'])
    with_clouds = [dict({k: v for k, v in f.items() if k not in ('radar', 'points', 'point_labels')}, cloud=c, cloud_columns=mapping) for f, c in zip(frames, clouds)]
    with_maps = [dict(f, radar=m, points=c[:, list(lay['points'])], point_labels=c[:, lay['label']].astype(np.int64))
                 for f, c, m in zip(frames, clouds, _fx()['r96/f64/maps'])]
    batcher = D.TrainBatcher(96, DC.NUM_SEG, DC.NUM_POINTS, device=dev)
    got, want = batcher(with_clouds, indices=idx), batcher(with_maps, indices=idx)
    for field in D.Batch._fields:
        g, w = getattr(got, field), getattr(want, field)
        assert g.dtype == w.dtype and g.shape == w.shape and _same(_np(g), _np(w)), field
    assert got.radar.any() and got.pc_labels.any()
    maps_only = batcher([dict(f, cloud_columns=dict(map=lay['map'])) for f in with_clouds])
    assert maps_only.points is None and maps_only.pc_labels is None and torch.equal(maps_only.radar, got.radar)
    with pytest.raises(ValueError, match='cloud'):
        batcher(with_clouds[:1] + with_maps[1:2], indices=idx[:2])


# ------------------------------------------------------------------------------------------------------------------ GPU only
@pytest.mark.gpu
def test_gpu_radar_calls_never_synchronise():
    """`radar_maps_batch` and `radar_points_batch` under torch's sync debug mode: no device-to-host copy, no blocking copy"""
    clouds = _clouds('r320')
    run = lambda: (D.radar_maps_batch(clouds, 320, normalize=True, dtype=torch.bfloat16), D.radar_points_batch(clouds, (0, 1, 2, 3, 4), 2, 64, rng=np.random.default_rng(1)))
    run()                                                                        # warm-up: pinned allocations
    torch.cuda.synchronize()
    guarded = False
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            torch.ones(1, device='cuda').item()                                  # the mode must actually refuse a host read on this build
        except RuntimeError:
            guarded = True
        run()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert guarded


@pytest.mark.gpu
def test_gpu_detect_frames_from_clouds_equals_detect_frames_on_the_fixture_maps():
    """EN-S0 at R = 320, B = 2 (the configuration of tests/test_serve.py): `detect_frames_from_clouds` against `detect_frames` fed the fixture's maps and the
    host-sampled points: boxes, counts, class maps and point classes are equal"""
    from achelous_amd import Achelous
    from achelous_amd.synth import condition_state_dict
    from golden_util import Golden, ctor_kwargs
    g = Golden('en_s0')
    kw = ctor_kwargs(g.meta)
    m = Achelous(**kw).eval()
    m.load_state_dict(g.calibrate(condition_state_dict(m.state_dict(), seed=g.meta['weight_seed'])), strict=True)
    m = m.cuda()
    rng = np.random.default_rng(9)
    frames = []
    for H, W in ((90, 160), (160, 90)):
        yy, xx = np.mgrid[0:H, 0:W]
        frames.append(np.clip(127 + 100 * np.sin(xx / 23.0)[..., None] * np.cos(yy[..., None] / 17.0 + np.arange(3)) + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8))
    clouds = _clouds('r320')[:2]
    idx = np.stack([np.random.default_rng([4, b]).choice(len(c), 512, replace=True) for b, c in enumerate(clouds)])
    got = prepost.detect_frames_from_clouds(m, frames, clouds, indices=idx, num_points=512, conf_thres=0.35, nms_thres=0.35, dtype=torch.float32)
    maps = torch.from_numpy(_fx()['r320/f64/maps'][:2].astype(np.float32)).cuda()
    pts = torch.from_numpy(np.stack([c[i] for c, i in zip(clouds, idx)]).astype(np.float32)).cuda()
    want = prepost.detect_frames(m, frames, maps, pts, 0.35, 0.35, True, 100, dtype=torch.float32)
    assert torch.equal(got['count'], want['count']) and torch.equal(got['boxes'], want['boxes'])
    assert torch.equal(got['point_class'], want['point_class'])
    for b in range(2):
        assert torch.equal(got['semantic'][b], want['semantic'][b]) and torch.equal(got['waterline'][b], want['waterline'][b]), b
        assert torch.equal(got['overlay'][b], want['overlay'][b]), b
