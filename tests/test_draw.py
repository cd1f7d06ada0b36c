"""Drawing the kept detections on served frames (achelous_amd/prepost.py draw_detections_frames / DrawStyle / LabelAtlas, detect_frames(draw=...); csrc/k_draw.h, C ABI
ach_draw_detections_frames): box rings, label plates and label text of a ragged batch in two launches, in place.

Truth is PIL itself: tests/golden/draw.npz holds what ImageDraw left when tests/golden/gen_draw_golden.py executed the reference's own drawing statements (achelous.py:400-433) on
the seeded cases of tests/draw_cases.py, and the label atlases; the cases are regenerated here and checked against a stored checksum.  EVERY comparison is exact byte
equality — of the whole arena, so the padding between rows and the bytes behind the last frame are held too.  Every kernel case runs once under the emulation library
(`-m "not gpu"`) and once on the MI355X (`-m gpu`); the kernel cases take their atlases from the fixture (`LabelAtlas.from_arrays`), so they need no font."""
import colorsys
import os

import numpy as np
import pytest
import torch

import draw_cases as DC
from achelous_amd import data as D
from achelous_amd import prepost as P

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICES = [pytest.param('cpu', id='emu'), pytest.param('cuda', id='gpu', marks=pytest.mark.gpu)]
SENTINEL, TAIL = 0xA5, 64
FONT = 'tests/golden/draw.npz'             # the cache key the fixture's atlases are registered under (never opened as a font file)
_FX = None
_CASES = {}


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
        with np.load(os.path.join(HERE, 'golden', 'draw.npz')) as z:
            _FX = {k: z[k] for k in z.files}
        for s in DC.FONT_SIZES:
            P.LabelAtlas.from_arrays(DC.NAMES, s, _FX[f'atlas/{s}/table'], _FX[f'atlas/{s}/blob'], font=FONT)
    return _FX


def _case(name):
    if name not in _CASES:
        c = DC.make_case(name)
        assert DC.checksum(c) == int(_fx()[f'{name}/checksum'][0]), 'tests/draw_cases.py no longer generates the inputs the fixture was recorded on'
        _CASES[name] = c
    return _CASES[name]


def _style(case, frames=None, **kw):
    _fx()
    th = case['thickness']
    if th is not None and frames is not None:
        th = tuple(th[b] for b in frames)
    return P.DrawStyle(DC.NAMES, skip=DC.SKIP, font=FONT, font_size=case['font_size'], thickness=th, **kw)


def _layout(shapes, extra_pitch=0):
    offs, pitches, total = [], [], 0
    for h, w in shapes:
        pitches.append((3 * w + 15) // 16 * 16 + extra_pitch)
        offs.append(total)
        total += h * pitches[-1]
    return offs, pitches, total


def _arena(images, offs, pitches, total):
    a = np.full(total + TAIL, SENTINEL, np.uint8)
    for img, o, p in zip(images, offs, pitches):
        h, w, _ = img.shape
        np.lib.stride_tricks.as_strided(a[o:], (h, w, 3), (p, 3, 1))[:] = img
    return a


def _run(dev, name, frames=None, extra_pitch=0, with_counts=False):
    """draw frames `frames` (default all, in order) of case `name` in ONE call; returns (arena bytes after, the arena PIL's images give, class counts)"""
    case = _case(name)
    frames = list(range(len(case['shapes']))) if frames is None else list(frames)
    shapes = [case['shapes'][b] for b in frames]
    offs, pitches, total = _layout(shapes, extra_pitch)
    before = _arena([case['images'][b] for b in frames], offs, pitches, total)
    want = _arena([DC.expected(_fx(), case, name, b) for b in frames], offs, pitches, total)
    arena = torch.from_numpy(before.copy()).to(dev)
    boxes = torch.from_numpy(case['rows'][frames]).to(dev)
    count = torch.tensor([case['dev_counts'][b] for b in frames], dtype=torch.int32).to(dev)
    cc = torch.full((len(frames), len(DC.NAMES)), -1, dtype=torch.int32).to(dev) if with_counts else None
    views = P.draw_detections_frames(arena, (offs, pitches), boxes, count, shapes, _style(case, frames), DC.INPUT_SHAPE, class_counts=cc)
    got = arena.cpu().numpy()
    for v, (h, w), o, p in zip(views, shapes, offs, pitches):
        assert tuple(v.shape) == (h, w, 3) and v.stride() == (p, 3, 1) and v.storage_offset() == o and v.data_ptr() == arena.data_ptr() + o
    print(dev, name, frames, 'bytes differing from PIL', int((got != want).sum()), 'bytes drawn', int((want != before).sum()))
    return got, want, before, None if cc is None else cc.cpu().numpy()


def _tally(case, b):
    ids = case['rows'][b, :case['counts'][b], 6]
    ids = ids[(ids > -1) & (ids < len(DC.NAMES))].astype(np.int64)
    return np.bincount(ids, minlength=len(DC.NAMES))


# ------------------------------------------------------------------------------------------------------------------ the cases, against PIL
def test_one_call_three_frame_sizes(dev):
    """37 x 53, 96 x 128 and 150 x 200 in one call, thickness 1 / 2 / 5, counts 0 / 1 / max_det = 12, font sizes 1 / 3 / 5 from three concatenated atlases: widths that are
    no multiple of 4, more than one tile both ways, partial edge tiles.  The count-0 frame keeps its bytes although its rows hold real boxes."""
    got, want, before, cc = _run(dev, 'three', with_counts=True)
    assert np.array_equal(got, want)
    case = _case('three')
    assert case['counts'] == [0, 1, DC.MAX_DET] and [DC.font_size_of(case, b) for b in range(3)] == [1, 3, 5]
    n0 = case['shapes'][0][0] * ((3 * case['shapes'][0][1] + 15) // 16 * 16)
    assert np.array_equal(got[:n0], before[:n0]) and (want != before).sum() > 20000
    assert np.array_equal(cc, np.stack([_tally(case, b) for b in range(3)]))


def test_thickness_and_font_size_follow_the_references_rules(dev):
    """no thickness / font size given: (W + H) // mean(input_shape) = 1, 3, 5 and floor(0.03 H + 0.5) = 1, 3, 5"""
    case = _case('rule')
    assert [DC.thickness_of(case, b) for b in range(3)] == [1, 3, 5]
    got, want, _, _ = _run(dev, 'rule')
    assert np.array_equal(got, want)


def test_overlapping_boxes_are_drawn_in_order(dev):
    """the same detections reversed give another image, and both equal their truth: later drawing overwrites earlier, text blends over what lies under it"""
    case = _case('overlap')
    assert np.array_equal(case['rows'][1, :6], case['rows'][0, :6][::-1])
    a, b = DC.expected(_fx(), case, 'overlap', 0), DC.expected(_fx(), case, 'overlap', 1)
    assert (a != b).any(axis=2).sum() > 500
    got, want, _, _ = _run(dev, 'overlap')
    assert np.array_equal(got, want)


@pytest.mark.parametrize('name', ['edges', 'overflow'])
def test_boxes_and_labels_at_and_past_the_edges(dev, name):
    """edges: boxes past all four sides, negative coordinates, bottom == H, right == W, a box narrower than 2 * thickness (rings skipped), left == right, top == bottom
    (ImageDraw's height-0 outline), a box at the top (label inside), a plate past the right edge, a box wholly outside.  overflow: a label wider than the frame and one
    that runs past the bottom edge."""
    got, want, _, _ = _run(dev, name)
    assert np.array_equal(got, want)


def test_scores_pick_the_label_pythons_formatting_picks(dev):
    """0.0, 0.125, 0.995, 1.0 (and 0.005, 0.375): round-half-even on the exact value of the float32 product"""
    assert [DC.label_index(np.float32(s)) for s in DC.SCORES] == [0, 12, 100, 100, 0, 38]
    assert ['{:.2f}'.format(np.float32(s)) for s in DC.SCORES] == ['0.00', '0.12', '1.00', '1.00', '0.00', '0.38']
    got, want, _, _ = _run(dev, 'scores')
    assert np.array_equal(got, want)


def test_skipped_rows_and_the_count_clamp(dev):
    """a skipped class, ids -1 and num_classes, a NaN and an inf coordinate are not drawn (and index nothing); rows past count full of NaN and 1e30 change nothing; a
    device count of 50 with max_det = 12 draws the twelve rows.  class_counts tallies by id alone: the skipped class counts, ids outside the range do not."""
    case = _case('skips')
    assert case['dev_counts'] == [8, 50] and np.isnan(case['rows'][0, 8:10]).all() and (case['rows'][0, 10:] == 1e30).all()
    got, want, _, cc = _run(dev, 'skips', with_counts=True)
    assert np.array_equal(got, want)
    assert np.array_equal(cc, np.stack([_tally(case, 0), _tally(case, 1)])) and cc[0].sum() == 6 and cc[0, 1] == 1 and cc[1].sum() == DC.MAX_DET


def test_a_frame_does_not_depend_on_its_batch_or_its_pitch(dev):
    """B = 1 equals the frame's slot of B = 3 in a permuted order, and a pitch 32 bytes larger changes no pixel (and leaves the wider padding alone)"""
    order = [2, 0, 1]
    got, want, _, _ = _run(dev, 'rule', frames=order)
    assert np.array_equal(got, want)
    for b in order:
        one, want1, _, _ = _run(dev, 'rule', frames=[b])
        assert np.array_equal(one, want1), b
    wide, want_wide, _, _ = _run(dev, 'rule', extra_pitch=32)
    assert np.array_equal(wide, want_wide)


# ------------------------------------------------------------------------------------------------------------------ rejections, on the host, before any launch
def test_wrong_arguments_are_rejected_before_any_launch(dev):
    case = _case('rule')
    shapes = case['shapes']
    offs, pitches, total = _layout(shapes)
    before = _arena(case['images'], offs, pitches, total)
    arena = torch.from_numpy(before.copy()).to(dev)
    boxes, count = torch.from_numpy(case['rows']).to(dev), torch.tensor(case['dev_counts'], dtype=torch.int32).to(dev)

    def call(style, layout=(offs, pitches), **kw):
        return P.draw_detections_frames(arena, layout, kw.get('boxes', boxes), count, shapes, style, DC.INPUT_SHAPE)
    table = _fx()['atlas/5/table'].copy()
    table[17, 0] = _fx()['atlas/5/blob'].size - 3                       # an atlas entry that runs past the blob
    P.LabelAtlas.from_arrays(DC.NAMES, 5, table, _fx()['atlas/5/blob'], font='bad atlas')
    with pytest.raises(ValueError, match="a label's mask passes the atlas blob"):
        call(P.DrawStyle(DC.NAMES, font='bad atlas', font_size=5))
    with pytest.raises(ValueError, match='thickness is 1..64'):
        call(P.DrawStyle(DC.NAMES, font=FONT, thickness=0))
    with pytest.raises(ValueError, match='thickness is 1..64'):
        call(P.DrawStyle(DC.NAMES, font=FONT, thickness=(1, 65, 1)))
    with pytest.raises(ValueError, match="a frame's extent passes the arena"):
        call(_style(case), (offs[:2] + [total + TAIL - 64], pitches))
    with pytest.raises(ValueError, match="a frame's extent passes the arena"):
        call(_style(case), (offs, [pitches[0], 3 * shapes[1][1] - 4, pitches[2]]))           # pitch < 3 W
    with pytest.raises(ValueError, match='one .H, W. per frame'):
        P.draw_detections_frames(arena, (offs, pitches), boxes, count, shapes[:2], _style(case), DC.INPUT_SHAPE)
    with pytest.raises(ValueError, match='boxes .B, max_det, 7. float32'):
        call(_style(case), boxes=boxes.double())
    with pytest.raises(ValueError, match='`thickness` holds 2 values'):
        call(P.DrawStyle(DC.NAMES, font=FONT, thickness=(1, 2)))
    with pytest.raises(ValueError, match='1..256 class names'):
        P.DrawStyle(())
    with pytest.raises(ValueError, match='needs overlay=True'):                              # before the network or any input is touched
        P.detect_frames(None, None, None, None, overlay=False, draw=_style(case))
    with pytest.raises(ValueError, match='needs overlay=True'):
        P.detect_frames_from_clouds(None, None, None, overlay=False, draw=_style(case))
    assert np.array_equal(arena.cpu().numpy(), before)


# ------------------------------------------------------------------------------------------------------------------ the host side
def test_class_colors_are_the_references_hsv_wheel():
    """against the colour tables the reference's own lines (achelous.py:130-132) gave when the fixture was generated"""
    for n in DC.COLOR_COUNTS:
        got = P.class_colors(n)
        assert got.dtype == np.uint8 and got.shape == (n, 3) and np.array_equal(got, _fx()[f'colors/{n}']), n
    assert [tuple(int(v) for v in c) for c in P.class_colors(3)] == list(DC.COLORS)
    assert len({tuple(c) for c in _fx()['colors/20']}) == 20


def _freetype():
    try:
        from PIL import features
        return bool(features.check('freetype2'))
    except Exception:
        return False


def test_live_atlas_and_live_pil_agree_with_the_fixture():
    """the atlas PIL renders now is the recorded one, and PIL drawing the 'edges' case now gives the recorded image (skips only where PIL has no FreeType)"""
    if not _freetype():
        pytest.skip('PIL without FreeType: no ImageFont.load_default(size)')
    from PIL import ImageFont
    fx = _fx()
    for s in (5, 12):
        a = P.LabelAtlas(DC.NAMES, s)
        assert np.array_equal(a.table, fx[f'atlas/{s}/table']) and np.array_equal(a.blob, fx[f'atlas/{s}/blob']), s
    assert P.LabelAtlas.get(DC.NAMES, 12) is P.LabelAtlas.get(list(DC.NAMES), 12)
    case = _case('edges')
    live = DC.draw_pil(case['images'][0], case['rows'][0, :case['counts'][0]], ImageFont.load_default(12), 5)
    assert np.array_equal(live, DC.expected(fx, case, 'edges', 0))


def test_replaced_atlas_arrays_reach_the_device(dev):
    """`from_arrays` under a key that was already drawn with: the next call uses the new arrays, not a cached device copy of the old ones"""
    case = _case('scores')
    fx = _fx()
    blank = np.zeros_like(fx['atlas/12/blob'])
    runs = []
    for blob in (blank, fx['atlas/12/blob']):
        P.LabelAtlas.from_arrays(DC.NAMES, 12, fx['atlas/12/table'], blob, font='replaced')
        offs, pitches, total = _layout(case['shapes'])
        arena = torch.from_numpy(_arena(case['images'], offs, pitches, total)).to(dev)
        P.draw_detections_frames(arena, (offs, pitches), torch.from_numpy(case['rows']).to(dev), torch.tensor(case['dev_counts'], dtype=torch.int32).to(dev),
                                 case['shapes'], P.DrawStyle(DC.NAMES, skip=DC.SKIP, font='replaced', font_size=12, thickness=1), DC.INPUT_SHAPE)
        runs.append(arena.cpu().numpy())
    want = _arena([DC.expected(fx, case, 'scores', 0)], *_layout(case['shapes']))
    assert np.array_equal(runs[1], want) and not np.array_equal(runs[0], want)


def test_numpy_restatement_equals_the_fixture():
    """the fixture comparison itself never skips: the rules restated in tests/draw_cases.py give PIL's recorded bytes on every frame of every case"""
    fx = _fx()
    for name in DC.CASES:
        case = _case(name)
        for b, img in enumerate(case['images']):
            s = DC.font_size_of(case, b)
            got = DC.draw_numpy(img, case['rows'][b, :case['counts'][b]], fx[f'atlas/{s}/table'], fx[f'atlas/{s}/blob'], DC.thickness_of(case, b))
            assert np.array_equal(got, DC.expected(fx, case, name, b)), (name, b)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _e2e_style(n):
    """a style for n classes: PIL's default font where PIL has FreeType, else seeded random masks of plausible sizes registered as atlases (the truth below is the numpy
    restatement fed with the same arrays either way)"""
    names = tuple(f'class{i}' for i in range(n))
    if _freetype():
        return P.DrawStyle(names, skip=(names[1],))
    rng = np.random.default_rng(5)
    for s in range(1, 8):
        table, blobs, off = np.zeros((n * 101, 7), np.int32), [], 0
        for e in range(n * 101):
            w, h = 5 * s, s
            table[e] = (off, w, h, 0, 1, w, h + 1)
            blobs.append(rng.integers(0, 256, w * h, dtype=np.uint8))
            off += w * h
        P.LabelAtlas.from_arrays(names, s, table, np.concatenate(blobs), font='synthetic')
    return P.DrawStyle(names, skip=(names[1],), font='synthetic')


@pytest.mark.gpu
def test_gpu_detect_frames_draws_what_pil_draws():
    """detect_frames(draw=style) = detect_frames() followed by draw_detections_frames on its overlay = the rules applied to the downloaded undrawn overlay and the
    returned boxes[:count] (and PIL itself where it has FreeType); class_counts = bincount of the kept ids; draw=None returns what it returned before; the drawn call
    neither reads back nor synchronises once the atlas is cached"""
    from achelous_amd import Achelous
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
    arena = D.pack_arena(frames, 3, 'cuda', 'draw_e2e')
    style = _e2e_style(kw['num_det'])
    args = (m, arena, radar, pts, 0.35, 0.35, True, 100)
    plain = P.detect_frames(*args, dtype=torch.float32)
    assert 'class_counts' not in plain
    undrawn = [v.cpu().numpy() for v in plain['overlay']]
    drawn = P.detect_frames(*args, dtype=torch.float32, draw=style)
    got = [v.cpu().numpy() for v in drawn['overlay']]
    for k in ('boxes', 'count', 'point_class'):
        assert torch.equal(drawn[k], plain[k]), k
    for k in ('semantic', 'waterline'):
        assert all(torch.equal(a, b) for a, b in zip(drawn[k], plain[k])), k
    again = P.detect_frames(*args, dtype=torch.float32)                          # draw=None: the same bytes as before
    assert all(np.array_equal(v.cpu().numpy(), u) for v, u in zip(again['overlay'], undrawn))
    # the two steps by hand: the undrawn overlays in an arena of the same layout, then draw_detections_frames
    layout = P.frames_layout(shapes)
    mine = torch.zeros(layout[5], dtype=torch.uint8, device='cuda')
    for b, (H, W) in enumerate(shapes):
        torch.as_strided(mine, (H, W, 3), (layout[4][b], 3, 1), layout[3][b]).copy_(plain['overlay'][b])
    cc = torch.empty(3, kw['num_det'], dtype=torch.int32, device='cuda')
    views = P.draw_detections_frames(mine, layout, plain['boxes'], plain['count'], shapes, style, (320, 320), class_counts=cc)
    assert all(np.array_equal(v.cpu().numpy(), w) for v, w in zip(views, got))
    assert torch.equal(cc, drawn['class_counts'])
    count, boxes = drawn['count'].cpu().numpy(), drawn['boxes'].cpu().numpy()
    assert int(count.sum()) > 0
    skip_ids = (1,)
    changed = 0
    for b, (H, W) in enumerate(shapes):
        rows = boxes[b, :count[b]]
        a = P.LabelAtlas.get(style.class_names, style.font_size_for(H), style.font)
        want = DC.draw_numpy(undrawn[b], rows, a.table, a.blob, style.thickness_for(b, H, W, (320, 320)), colors=[tuple(int(v) for v in c) for c in style.colors], skip_ids=skip_ids)
        print('frame', b, 'detections', int(count[b]), 'pixels drawn', int((want != undrawn[b]).any(axis=2).sum()), 'differing', int((want != got[b]).any(axis=2).sum()))
        assert np.array_equal(got[b], want), b
        changed += int((want != undrawn[b]).sum())
        ids = rows[:, 6].astype(np.int64)
        assert np.array_equal(drawn['class_counts'][b].cpu().numpy(), np.bincount(ids, minlength=kw['num_det'])), b
        if _freetype():
            from PIL import ImageFont
            pil = DC.draw_pil(undrawn[b], rows, ImageFont.load_default(style.font_size_for(H)), style.thickness_for(b, H, W, (320, 320)), names=style.class_names,
                              colors=style.colors, skip_ids=skip_ids)
            assert np.array_equal(got[b], pil), b
    assert changed > 0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        quiet = P.detect_frames(*args, dtype=torch.float32, draw=style)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert all(np.array_equal(v.cpu().numpy(), w) for v, w in zip(quiet['overlay'], got))
