"""The radar point classes on served frames (achelous_amd/prepost.py scatter_points_frames / ScatterStyle, detect_frames(scatter=...); csrc/k_scatter.h, C ABI
ach_scatter_points_frames in include/achelous_points.h): per frame the unique sorted (u, v, rcs, class) rows and their discs painted in place, in two launches.

Truth.  The rows are the reference's own statements: tests/golden/scatter.npz holds what tests/golden/gen_scatter_golden.py got when it executed achelous.py:262-268
(read out of the reference's source) on the cases of tests/scatter_cases.py, and matplotlib's viridis colours of them.  Coverage, colour index and paint are the oracle
of tests/scatter_cases.py: the float64 expression in numpy, the integer index rule (held to matplotlib here), real PIL blends row after row.  Every kernel case runs
once under the emulation library (`-m "not gpu"`) and once on the MI355X (`-m gpu`).  Everything is exact: rows (by value), count, range and every byte of the arena."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scatter_cases as SC
from achelous_amd import prepost as P
from achelous_amd.colormaps import VIRIDIS

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICES = [pytest.param('cpu', id='emu'), pytest.param('cuda', id='gpu', marks=pytest.mark.gpu)]
_FX = None
_RUNS = {}
_WANT = {}


@pytest.fixture(params=DEVICES)
def dev(request):
    """'cpu': the kernels under the emulation library; 'cuda': the HIP kernels"""
    if request.param == 'cpu':
        from emu_util import emu_library
        P._pass_lib.test_library = emu_library()
    try:
        yield request.param
    finally:
        P._pass_lib.test_library = None


def _fx():
    global _FX
    if _FX is None:
        with np.load(os.path.join(HERE, 'golden', 'scatter.npz')) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def _want(name):
    """the oracle's result for a case, computed once and left unchanged"""
    if name not in _WANT:
        _WANT[name] = SC.oracle(name, _fx()['viridis'])
    return _WANT[name]


def _arena(images):
    """packed HWC frames the way the kernels must cope with: offsets and pitches multiples of 4, 8 bytes of padding behind every row, 12 between frames, a sentinel in all of it"""
    offs, pitches, total = [], [], 8
    for img in images:
        h, w, _ = img.shape
        pitches.append((3 * w + 3) // 4 * 4 + 8)
        offs.append(total)
        total += h * pitches[-1] + 12
    a = np.full(total + 16, SC.SENTINEL, np.uint8)
    for img, o, p in zip(images, offs, pitches):
        np.lib.stride_tricks.as_strided(a[o:], img.shape, (p, 3, 1))[:] = img
    return a, offs, pitches


def _call(dev, name, frames=None, dense=False, device_indices=False):
    """one scatter_points_frames call on (frames of) a case; everything downloaded"""
    c = SC.case(name)
    pick = list(range(len(c['frames']))) if frames is None else list(frames)
    images = [SC.make_base(c['frames'][i]) for i in pick]
    shapes = [SC.SHAPES[c['frames'][i]] for i in pick]
    before, offs, pitches = _arena(images)
    arena = torch.from_numpy(before.copy()).to(dev)
    cls = torch.from_numpy(np.ascontiguousarray(c['classes'][pick])).to(dev)
    idx = np.ascontiguousarray(c['indices'][pick])
    clouds = [c['clouds'][i] for i in pick]
    if dense:                                                            # (u, v, s) of every cloud row as one [B, n, 3] tensor; the case has n = N for every frame
        r, cu, cv = c['columns'] or (2, 3, 4)
        points = torch.from_numpy(np.stack([cl[:, [cu, cv, r]] for cl in clouds])).to(dev)
    else:
        points = clouds
    res = P.scatter_points_frames(arena, (offs, pitches), shapes, points, cls, SC.NUM_CLASSES, P.ScatterStyle(**c['style']),
                                  torch.from_numpy(idx).to(dev) if device_indices else idx)
    assert res['point_rows'].dtype == torch.float64 and tuple(res['point_rows'].shape) == (len(pick), c['N'], 4)
    assert res['point_count'].dtype == torch.int32 and res['point_class_range'].dtype == torch.int32 and tuple(res['point_class_range'].shape) == (len(pick), 2)
    assert all(v.data_ptr() == arena.data_ptr() + o and v.stride() == (p, 3, 1) for v, o, p in zip(res['frames'], offs, pitches))
    return dict(rows=res['point_rows'].cpu().numpy(), count=res['point_count'].cpu().numpy(), range=res['point_class_range'].cpu().numpy(),
                after=arena.cpu().numpy(), before=before, offs=offs, pitches=pitches, shapes=shapes, pick=pick)


def _run(dev, name):
    if (dev, name) not in _RUNS:
        _RUNS[(dev, name)] = _call(dev, name)
    return _RUNS[(dev, name)]


def _frame(r, i):
    h, w = r['shapes'][i]
    return np.lib.stride_tricks.as_strided(r['after'][r['offs'][i]:], (h, w, 3), (r['pitches'][i], 3, 1))


# ------------------------------------------------------------------------------------------------------------------ the kernels, every case
@pytest.mark.parametrize('name', SC.CASE_NAMES)
def test_rows_count_range_and_every_arena_byte_are_exact(dev, name):
    """rows (by value), count and class range of every frame are the oracle's, rows past the count are zero, and the WHOLE arena is the arena before with the oracle's
    pictures in the frames' places: covered pixels are PIL's bytes in the rows' order, uncovered pixels, padded pitches and the gaps between frames keep theirs"""
    r, want = _run(dev, name), _want(name)
    expect = r['before'].copy()
    for i, w in enumerate(want):
        n = int(r['count'][i])
        print(dev, name, r['shapes'][i], 'rows', n, 'of', SC.case(name)['N'], 'range', r['range'][i].tolist(), 'covered pixels', int(w['union'].sum()))
        assert n == w['count'] and r['range'][i].tolist() == list(w['range']), i
        assert np.array_equal(r['rows'][i, :n], w['rows']) and not r['rows'][i, n:].any(), i
        h, wd = r['shapes'][i]
        np.lib.stride_tricks.as_strided(expect[r['offs'][i]:], (h, wd, 3), (r['pitches'][i], 3, 1))[:] = w['image']
    assert np.array_equal(r['after'], expect)


def test_the_cases_hold_what_they_are_meant_to(dev):
    """the properties the cases exist for, read off the oracle and the kernel's output: a frame with no row (count 0, range (0, 0), untouched), duplicates removed,
    rows equal in (u, v, s) with two classes, -0.0 and 0.0 one row, negative coordinates, huge finite rows kept, s <= 0 kept, hi == lo, lo > 0, order matters"""
    r, want, c = _run(dev, 'mix64'), _want('mix64'), SC.case('mix64')
    assert r['count'][0] == 0 and r['range'][0].tolist() == [0, 0] and np.array_equal(_frame(r, 0), SC.make_base(0)) and not r['rows'][0].any()
    for i in range(1, 6):
        rows = r['rows'][i, :r['count'][i]]
        assert len(rows) < 64 - 11 and np.isfinite(rows).all()                                   # 9 non-finite, 2 bad classes, 1 bad index and the duplicates left
        uvs = [tuple(x) for x in rows[:, :3]]
        assert len(set(uvs)) < len(uvs), 'rows equal in (u, v, s) but not in class'
        c6 = c['clouds'][i][6]
        assert ((rows[:, 0] == 0) & (rows[:, 1] == c6[4]) & (rows[:, 2] == c6[2]) & (rows[:, 3] == c['classes'][i][6])).sum() == 1, '-0.0 and 0.0 are one row'
        assert (rows[:, 0] == -3.5).any() and (rows[:, 0] == 1e300).any() and (rows[:, 0] == -1e300).any() and (rows[:, 1] == 1e300).any()
        assert (rows[:, 2] == 0).any() and (rows[:, 2] < 0).any()
        assert rows[:, 3].min() >= 0 and rows[:, 3].max() < SC.NUM_CLASSES
    assert all(w['range'][0] == w['range'][1] == 4 and w['count'] == 1 for w in _want('identical'))
    assert all(w['range'][0] >= 3 for w in _want('lo3')[1:])
    a, b = _want('order0.5'), _want('order0.98')
    assert all(not np.array_equal(x['image'], y['image']) for x, y in zip(a, b)) and all(x['count'] == 300 for x in a)
    assert np.array_equal(_want('order0.0')[0]['image'], SC.make_base(1)) and _want('order0.0')[0]['union'].any()
    geom = _want('geom')
    assert all(w['union'].all() for w in geom), 'a disc covers the whole frame'
    assert not all(w['union'].all() for w in _want('geom_r6')), 'max_radius clamps it'


def test_two_runs_agree_and_a_frame_alone_is_the_frame_in_its_batch(dev):
    """the same call again gives the same bytes, and every frame run as a batch of one gives the rows and the picture it has inside the batch"""
    for name in ('mix64', 'geom'):
        r = _run(dev, name)
        again = _call(dev, name)
        assert np.array_equal(again['after'], r['after']) and np.array_equal(again['rows'], r['rows'])
        for i in range(len(r['shapes'])):
            one = _call(dev, name, frames=[i])
            assert np.array_equal(one['rows'][0], r['rows'][i]) and one['count'][0] == r['count'][i] and np.array_equal(one['range'][0], r['range'][i]), (name, i)
            assert np.array_equal(_frame(one, 0), _frame(r, i)), (name, i)


def test_dense_points_and_device_indices_take_the_same_path(dev):
    """a dense device tensor [B, N, 3] = (u, v, s) with the indices on the device gives what the packed clouds give"""
    r = _run(dev, 'geom')
    d = _call(dev, 'geom', dense=True, device_indices=True)
    assert np.array_equal(d['rows'], r['rows']) and np.array_equal(d['count'], r['count']) and np.array_equal(d['range'], r['range']) and np.array_equal(d['after'], r['after'])
    o = _call(dev, 'order0.5', dense=True)
    assert np.array_equal(o['after'], _run(dev, 'order0.5')['after'])


# ------------------------------------------------------------------------------------------------------------------ rejections, on the host, before any launch
def test_wrong_arguments_are_rejected_before_any_launch(dev):
    """each a ValueError, and the arena keeps every byte"""
    c = SC.case('mix64')
    shapes = [SC.SHAPES[b] for b in c['frames']]
    before, offs, pitches = _arena([SC.make_base(b) for b in c['frames']])
    arena = torch.from_numpy(before.copy()).to(dev)
    cls = torch.from_numpy(c['classes']).to(dev)

    def call(arena=arena, offs=offs, pitches=pitches, clouds=c['clouds'], cls=cls, idx=c['indices'], style=None, nc=SC.NUM_CLASSES):
        return P.scatter_points_frames(arena, (offs, pitches), shapes, clouds, cls, nc, style or P.ScatterStyle(), idx)

    def edit(lst, i, v):
        out = list(lst)
        out[i] = v
        return out
    with pytest.raises(ValueError, match='1..4096 points per frame'):
        call(cls=torch.zeros(6, 4097, dtype=torch.int64, device=dev), idx=np.zeros((6, 4097), np.int64))
    with pytest.raises(ValueError, match="a frame's extent passes the arena"):
        call(arena=arena[:offs[5] + 100])                                                        # a frame past the arena
    with pytest.raises(ValueError, match="a frame's extent passes the arena"):
        call(pitches=edit(pitches, 3, 3 * 131 - 1))                                              # a pitch below 3 W (392: a multiple of 4, so only that is wrong)
    with pytest.raises(ValueError, match="a frame's extent passes the arena"):
        call(offs=edit(offs, 2, offs[2] + 2))                                                    # an offset that is no multiple of 4
    with pytest.raises(ValueError, match='a column index is not below F'):
        call(style=P.ScatterStyle(columns=(2, 5, 4)))
    with pytest.raises(ValueError, match='num_classes is 1..256'):
        call(nc=257)
    for kw, match in ((dict(alpha=1.5), 'alpha lies in'), (dict(alpha=-0.1), 'alpha lies in'), (dict(alpha=float('nan')), 'alpha lies in'), (dict(max_radius=0), 'max_radius'),
                      (dict(max_radius=257), 'max_radius'), (dict(size_scale=0.0), 'size_scale'), (dict(size_scale=-1.0), 'size_scale'), (dict(class_range=(5, 2)), 'class_range'),
                      (dict(cmap=np.zeros((255, 3), np.uint8)), 'uint8 .256, 3. table'), (dict(columns=(1, 2)), 'three columns')):
        with pytest.raises(ValueError, match=match):
            P.ScatterStyle(**kw)
    with pytest.raises(ValueError, match='colours for 9 classes'):
        call(style=P.ScatterStyle(colors=np.zeros((4, 3), np.uint8)))
    with pytest.raises(ValueError, match='one cloud per frame'):
        call(clouds=c['clouds'][:3])
    with pytest.raises(ValueError, match='indices are .B, N.'):
        call(idx=c['indices'][:, :10])
    assert np.array_equal(arena.cpu().numpy(), before)
    # the C entry's own checks of alpha, the radius and k, with a style that is edited after it was made
    for field, v, match in (('alpha', 2.0, 'alpha lies in'), ('max_radius', 0, 'max_radius is 1..256'), ('k', 0.0, 'k = size_scale'), ('k', float('inf'), 'k = size_scale')):
        st = P.ScatterStyle()
        setattr(st, field, v)
        with pytest.raises(ValueError, match=match):
            call(style=st)
    assert np.array_equal(arena.cpu().numpy(), before)
    with pytest.raises(ValueError, match='needs overlay=True'):                                  # before the network or any input is touched
        P.detect_frames(None, None, None, None, overlay=False, scatter=P.ScatterStyle())
    with pytest.raises(ValueError, match='needs overlay=True'):
        P.detect_frames_from_clouds(None, None, None, overlay=False, scatter=P.ScatterStyle())
    call()                                                                                       # and the unedited call goes through
    assert not np.array_equal(arena.cpu().numpy(), before)


# ------------------------------------------------------------------------------------------------------------------ the host side
def test_oracle_rows_and_colours_equal_the_fixture():
    """np.unique after the stated filter gives the rows the reference's own statements gave, and the integer index rule the colours matplotlib gave them"""
    fx = _fx()
    assert fx['source_lines'].tolist() == [262, 268]
    seen = 0
    for name in SC.CASE_NAMES:
        for i, w in enumerate(_want(name)):
            assert np.array_equal(w['rows'], fx[f'{name}/rows/{i}']), (name, i)
            if f'{name}/colours/{i}' in fx:
                assert np.array_equal(w['colours'], fx[f'{name}/colours/{i}']), (name, i)
                seen += 1
    assert seen >= 12 and all(f'{n}/colours/1' in fx for n in SC.FIXTURE_COLOUR_CASES)


def test_shipped_viridis_table_is_matplotlibs():
    """the 768 bytes in the package are the fixture's (matplotlib.cm.viridis(arange(256), bytes=True)), and the installed matplotlib's where there is one"""
    assert VIRIDIS.dtype == np.uint8 and VIRIDIS.shape == (256, 3) and np.array_equal(VIRIDIS, _fx()['viridis'])
    assert np.array_equal(P.ScatterStyle().cmap, VIRIDIS)
    try:
        from matplotlib import cm
    except ImportError:
        return
    assert np.array_equal(VIRIDIS, cm.viridis(np.arange(256), bytes=True)[:, :3])


def test_integer_index_rule_is_matplotlibs_normalize_for_all_small_ranges():
    """index = 0 when hi == lo, else min(((c - lo) * 256) // (hi - lo), 255): for all 0 <= lo <= c <= hi <= 16 the colour matplotlib gives (recorded in the fixture, and
    asked of the installed matplotlib where there is one)"""
    fx = _fx()
    try:
        from matplotlib import cm
        from matplotlib.colors import Normalize
    except ImportError:
        cm = None
    n = 0
    for lo in range(17):
        for hi in range(lo, 17):
            c = np.arange(lo, hi + 1)
            mine = VIRIDIS[SC.colour_index(c, lo, hi)]
            assert np.array_equal(mine, fx['index_rule'][lo, hi, lo:hi + 1]), (lo, hi)
            if cm is not None:
                assert np.array_equal(mine, cm.viridis(Normalize(lo, hi)(c.astype(np.float64)), bytes=True)[:, :3]), (lo, hi)
            n += len(c)
    assert n == 969


def test_the_entry_is_declared_in_its_own_header_and_bound_from_it():
    """include/achelous_points.h declares ach_scatter_points_frames and nothing else; the binding reads it into a table of its own and leaves PROTOTYPES, EXTENSIONS
    and SYMBOLS what they were; both libraries export the entry with the header's 27 parameters"""
    from achelous_amd import engine as E
    from emu_util import emu_library
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = (ctypes.c_int, [vp, i64, vp, vp, i32, vp, i64, i32, vp, vp, i32, i32, vp, i32, i32, i32, ctypes.c_float, ctypes.c_double, i32, vp, vp, vp, vp, i64, vp, i64, vp])
    assert E.POINT_ENTRIES == {'ach_scatter_points_frames': want}
    assert set(E.EXTENSIONS) == {'ach_heatmap_frames'} and E.EXTENSION_HEADERS == ('achelous_heatmap.h',)
    assert 'ach_scatter_points_frames' not in E.PROTOTYPES and E.NativeLibrary.SYMBOLS == tuple(E.PROTOTYPES) and len(E.PROTOTYPES) == 88
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(E.HEADER), 'achelous_points.h')).read(), flags=re.S)
    assert re.findall(r'\b(ach_[a-z_0-9]+)\s*\(', src) == ['ach_scatter_points_frames'] and '#include "achelous.h"' in src
    libs = [emu_library()] + ([E.NativeLibrary(E.HIP_LIBRARY)] if os.path.exists(E.HIP_LIBRARY) else [])
    for lib in libs:
        fn = lib.lib.ach_scatter_points_frames
        assert fn.restype is want[0] and list(fn.argtypes) == want[1], lib.path


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.gpu
def test_gpu_serving_with_scatter_is_scatter_points_frames_on_the_plain_overlay():
    """a small EN-S0 at R = 64, three ragged frames, N = 64: detect_frames_from_clouds(scatter=style) = scatter_points_frames by hand on the overlay of the plain call
    with the same inputs and indices, every other key is byte for byte the plain call's, and the same for detect_frames(scatter=, point_uvs=)"""
    from achelous_amd import Achelous
    from achelous_amd.synth import condition_state_dict
    m = Achelous(7, 9, phi='S0', resolution=64, backbone='en', pc_channels=5, pc_classes=8, nano_head=True).eval()
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=3), strict=True)
    m = m.cuda()
    shapes = [(40, 64), (64, 40), (37, 53)]
    frames = [SC.hashed(900 + b, h * w * 3, 256).astype(np.uint8).reshape(h, w, 3) for b, (h, w) in enumerate(shapes)]
    clouds = []
    for b, (h, w) in enumerate(shapes):
        c = SC._cloud(910 + 5 * b, 40, h, w, 5, (2, 3, 4), np.float64, smax=400, margin=3)
        c[1, 2] = -1.0                                                   # (no NaN here: the network reads these clouds, and NaN outputs compare unequal)
        clouds.append(c)
    idx = np.stack([SC.hashed(930 + b, 64, 40) for b in range(3)])
    style = P.ScatterStyle(alpha=0.9, size_scale=1.5, max_radius=12)
    lay = P.frames_layout(shapes)
    new = {'point_rows', 'point_count', 'point_class_range'}

    def check(got, plain, points, indices):
        assert set(got) == set(plain) | new and not new & set(plain)
        for k in ('boxes', 'count', 'point_class'):
            assert torch.equal(got[k], plain[k]), k
        for k in ('semantic', 'waterline'):
            assert all(torch.equal(a, b) for a, b in zip(got[k], plain[k])), k
        under = torch.zeros(lay[5], dtype=torch.uint8, device='cuda')
        for b, (h, w) in enumerate(shapes):
            torch.as_strided(under, (h, w, 3), (lay[4][b], 3, 1), lay[3][b]).copy_(plain['overlay'][b])
        mine = P.scatter_points_frames(under, lay, shapes, points, plain['point_class'], 8, style, indices)
        for k in new:
            assert torch.equal(got[k], mine[k]), k
        assert all(torch.equal(a, b) for a, b in zip(got['overlay'], mine['frames']))
        cnt = got['point_count'].cpu().numpy()
        print('rows per frame', cnt.tolist(), 'ranges', got['point_class_range'].cpu().numpy().tolist())
        assert (cnt > 0).all() and (cnt <= 64).all() and any(not torch.equal(a, b) for a, b in zip(got['overlay'], plain['overlay']))
        return mine

    args = dict(indices=idx, num_points=64, conf_thres=0.35, nms_thres=0.35, dtype=torch.float32)
    plain = P.detect_frames_from_clouds(m, frames, clouds, **args)
    got = P.detect_frames_from_clouds(m, frames, clouds, scatter=style, **args)
    mine = check(got, plain, clouds, idx)
    # the rows are the oracle's for the classes the network gave
    cls = plain['point_class'].cpu().numpy()
    for b in range(3):
        rows = SC.unique_rows(SC.gather(clouds[b], idx[b], cls[b], 8, (2, 3, 4)))
        n = int(mine['point_count'][b])
        assert n == len(rows) and np.array_equal(mine['point_rows'][b, :n].cpu().numpy(), rows), b
    radar = torch.from_numpy(np.stack([SC.hashed(950 + b, 3 * 64 * 64, 512).reshape(3, 64, 64) / 16.0 for b in range(3)]).astype(np.float32)).cuda()
    pts = torch.from_numpy(np.stack([c[i] for c, i in zip(clouds, idx)])[:, :, [4, 2, 0, 1, 3]].astype(np.float32)).cuda()
    uvs = torch.from_numpy(np.stack([c[i][:, [3, 4, 2]] for c, i in zip(clouds, idx)])).cuda()
    dargs = (m, frames, radar, pts, 0.35, 0.35, True, 100)
    plain2 = P.detect_frames(*dargs, dtype=torch.float32)
    got2 = P.detect_frames(*dargs, dtype=torch.float32, scatter=style, point_uvs=uvs)
    check(got2, plain2, uvs, None)
