"""Seeded cases for tests/test_draw.py and tests/golden/gen_draw_golden.py, and the drawing rules of achelous.py:400-433 restated in numpy.

`draw_numpy` is an INDEPENDENT restatement (ring by ring, rectangle by rectangle, Python's own '{:.2f}'), not the kernel's closed forms, and `draw_pil` the same rules
handed to PIL's ImageDraw; gen_draw_golden.py asserts that both equal what the reference's own statements leave on every case before it writes the fixture, so a test
may use any of them as truth."""
import zlib

import numpy as np

NAMES = ('boat', 'sailor', 'buoy')
SKIP = ('sailor',)
COLORS = ((255, 0, 0), (0, 255, 0), (0, 0, 255))          # class_colors(3), spelled out (tests/test_draw.py holds the function to the reference's expression)
INPUT_SHAPE = (70, 70)                                    # (W + H) // 70: thickness 1, 3 and 5 for the three sizes below
SHAPES3 = [(37, 53), (96, 128), (150, 200)]               # (H, W): odd widths, widths that are no multiple of 4, several tiles both ways, partial edge tiles
MAX_DET = 12
SCORES = (0.0, 0.125, 0.995, 1.0, 0.005, 0.375)           # float32(0.995) lies above 0.995 -> '1.00'; 0.125 and 0.375 are exact ties -> '0.12', '0.38'


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(xx / 9.0)[..., None] * np.cos(yy[..., None] / 7.0 + np.arange(3))
    return np.clip(base + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)


def random_rows(h, w, n, seed, ids=(0, 2, 0, 2, 1)):
    """n detections (y1, x1, y2, x2, obj, cls, id): centres anywhere in the frame, a quarter reaching past an edge, fractional coordinates"""
    rng = np.random.default_rng(seed)
    cy, cx = rng.uniform(0, h, n), rng.uniform(0, w, n)
    hh, ww = rng.uniform(2, 0.7 * h, n), rng.uniform(2, 0.7 * w, n)
    rows = np.stack([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2, rng.uniform(0.3, 1, n), rng.uniform(0.3, 1, n),
                     np.array([ids[i % len(ids)] for i in range(n)], dtype=np.float64)], axis=1)
    return rows.astype(np.float32)


def _pad(rows, fill=0.0):
    out = np.full((MAX_DET, 7), fill, np.float32)
    out[:len(rows)] = rows
    return out


def _case(shapes, rows, counts, seed, thickness=None, font_size=None, dev_counts=None):
    """rows: per frame [MAX_DET, 7]; counts: how many the truth draws; dev_counts: what the device is told (default the same)"""
    return dict(shapes=list(shapes), images=[image(h, w, seed + i) for i, (h, w) in enumerate(shapes)], rows=np.stack(rows).astype(np.float32),
                counts=list(counts), dev_counts=list(counts if dev_counts is None else dev_counts), thickness=thickness, font_size=font_size)


def make_case(name):
    H, W = 150, 200
    if name == 'three':
        # ONE call: three sizes, thickness 1, 2 and 5 given per frame, counts 0 / 1 / MAX_DET, the reference's font sizes 1, 3 and 5; the count-0 frame's rows are real
        # boxes that must not be drawn
        rows = [random_rows(h, w, MAX_DET, 100 + i) for i, (h, w) in enumerate(SHAPES3)]
        return _case(SHAPES3, rows, (0, 1, MAX_DET), 10, thickness=(1, 2, 5))
    if name == 'rule':
        # thickness and font size by the reference's own rules: (W + H) // 70 = 1, 3, 5
        rows = [random_rows(h, w, MAX_DET, 200 + i) for i, (h, w) in enumerate(SHAPES3)]
        return _case(SHAPES3, rows, (5, MAX_DET, 7), 20)
    if name == 'overlap':
        # the same overlapping boxes in both orders, with a 12-pixel font: plates and anti-aliased text over each other
        r = np.array([[20 + 6 * i, 10 + 9 * i, 60 + 6 * i, 70 + 9 * i, 0.9 - 0.07 * i, 0.8, (0, 2)[i % 2]] for i in range(6)], np.float32)
        return _case([(96, 128), (96, 128)], [_pad(r), _pad(r[::-1])], (6, 6), 30, font_size=12)
    if name == 'edges':
        r = np.array([[-20.5, -30.2, 40.7, 50.1, 0.9, 0.9, 0],          # past the top and the left, negative coordinates; the label goes inside
                      [100.3, 150.9, 400.0, 900.0, 0.8, 0.9, 2],        # past the bottom and the right: bottom == H, right == W
                      [60.0, 80.0, 90.0, 86.9, 0.7, 0.9, 0],            # 6 wide with thickness 5: rings 4 is skipped
                      [70.0, 120.0, 74.5, 160.0, 0.7, 0.8, 2],          # 4 high: ring 2 has height 0 (ImageDraw also paints the row below at its ends), rings 3, 4 skipped
                      [30.0, 100.0, 55.0, 100.9, 0.6, 0.9, 0],          # left == right
                      [40.2, 110.0, 40.9, 140.0, 0.6, 0.8, 2],          # top == bottom
                      [3.0, 60.0, 30.0, 95.0, 0.5, 0.9, 2],             # at the top: no room above, the label goes inside
                      [120.0, 190.0, 140.0, 260.0, 0.5, 0.8, 0],        # the plate and the text run past the right edge
                      [60.0, 300.0, 90.0, 400.0, 0.5, 0.7, 2],          # wholly right of the image: no ring; left >= W, so nothing of the plate either
                      [149.0, 20.0, 170.0, 60.0, 0.4, 0.9, 0]], np.float32)   # top on the last row
        return _case([(H, W)], [_pad(r)], (len(r),), 40, thickness=(5,), font_size=12)
    if name == 'overflow':
        # a 20-pixel font on a 37 x 53 frame: labels wider than the frame and, placed inside a box at the top, taller than what is left below
        r = np.array([[18.0, 5.0, 30.0, 40.0, 0.9, 0.9, 0], [2.0, 30.0, 36.0, 52.0, 0.8, 0.9, 2], [30.0, 0.0, 37.0, 53.0, 0.5, 0.5, 0]], np.float32)
        return _case([(37, 53)], [_pad(r)], (3,), 50, thickness=(2,), font_size=20)
    if name == 'scores':
        r = np.array([[8 + 14 * i, 6 + 3 * i, 20 + 14 * i, 120 - 5 * i, s, 1.0, (0, 2)[i % 2]] for i, s in enumerate(SCORES)], np.float32)
        return _case([(96, 128)], [_pad(r)], (len(SCORES),), 60, thickness=(1,), font_size=12)
    if name == 'skips':
        # frame 0: a skipped class, ids -1 and num_classes, a NaN and an inf coordinate between drawn rows; the rows past count hold NaN and 1e30
        good = random_rows(96, 128, 8, 70, ids=(0, 2))
        a = good.copy()
        a[1, 6] = 1                      # 'sailor'
        a[2, 6] = -1
        a[3, 6] = len(NAMES)
        a[4, 1] = np.nan
        a[5, 2] = np.inf
        a = _pad(a, np.nan)
        a[10:] = 1e30
        # frame 1: the device is told count = 50 with max_det = 12: clamped, all twelve rows are drawn
        b = random_rows(96, 128, MAX_DET, 71, ids=(0, 2))
        return _case([(96, 128), (96, 128)], [a, b], (8, MAX_DET), 80, thickness=(2, 2), font_size=12, dev_counts=(8, 50))
    raise KeyError(name)


CASES = ('three', 'rule', 'overlap', 'edges', 'overflow', 'scores', 'skips')
COLOR_COUNTS = (1, 3, 7, 20)              # class counts whose reference colour tables the fixture records
FONT_SIZES = (1, 3, 5, 12, 20)            # 1, 3, 5: floor(0.03 H + 0.5) of the three heights; 12 and 20 given


def checksum(case):
    c = 0
    for im in case['images']:
        c = zlib.crc32(im.tobytes(), c)
    c = zlib.crc32(np.nan_to_num(case['rows'], nan=-7.0, posinf=-8.0).tobytes(), c)
    return zlib.crc32(np.asarray(case['counts'] + case['dev_counts'], np.int64).tobytes(), c)


def expected(fx, case, name, b):
    """PIL's image of frame b from the fixture `fx` (a dict of draw.npz's arrays): the stored changed pixels over the regenerated background"""
    img = case['images'][b]
    mask = np.unpackbits(fx[f'{name}/{b}/changed'])[:img.shape[0] * img.shape[1]].reshape(img.shape[:2]).astype(bool)
    return np.where(mask[..., None], fx[f'{name}/{b}'], img)


def font_size_of(case, b):
    return int(np.floor(3e-2 * case['shapes'][b][0] + 0.5)) if case['font_size'] is None else case['font_size']


def thickness_of(case, b):
    h, w = case['shapes'][b]
    return int(max((w + h) // np.mean(INPUT_SHAPE), 1)) if case['thickness'] is None else case['thickness'][b]


# ------------------------------------------------------------------------------------------------------------------ the rules, in numpy
def label_index(score):
    """hundredths of '{:.2f}'.format(score) for a float32 score, clamped to 0..100"""
    return int(min(max(round(float('{:.2f}'.format(score)) * 100), 0), 100))


def _fill(out, x0, y0, x1, y1, colour):
    """[x0, x1] x [y0, y1], both ends inclusive, clipped to the image"""
    H, W = out.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    if x0 <= x1 and y0 <= y1:
        out[y0:y1 + 1, x0:x1 + 1] = colour


def kept(row, num_classes, skip_ids):
    """the class id of a row that is drawn, else None"""
    cid = row[6]
    if not (cid > -1 and cid < num_classes):
        return None
    c = int(cid)
    return None if c in skip_ids or not np.isfinite(row[:6]).all() else c


def draw_numpy(img, rows, table, blob, thickness, colors=COLORS, skip_ids=(1,), ink=(0, 0, 0)):
    """img [H, W, 3] uint8; rows [n, 7] float32 (only the rows to draw); table / blob: the LabelAtlas arrays of the frame's font size"""
    out = img.copy()
    H, W = out.shape[:2]
    for row in np.asarray(rows, np.float32):
        c = kept(row, len(colors), skip_ids)
        if c is None:
            continue
        fl = [int(np.clip(np.floor(v), -2 ** 24, 2 ** 24)) for v in row[:4]]
        top, left, bottom, right = max(0, fl[0]), max(0, fl[1]), min(H, fl[2]), min(W, fl[3])
        off, mw, mh, ox, oy, lw, lh = (int(v) for v in table[c * 101 + label_index(np.float32(row[4]) * np.float32(row[5]))])
        org_x, org_y = (left, top - lh) if top - lh >= 0 else (left, top + 1)
        for i in range(thickness):
            x0, y0, x1, y1 = left + i, top + i, right - i, bottom - i
            if x1 < x0 or y1 < y0:
                continue                                   # current Pillow raises here; the reference's Pillow drew nothing visible
            _fill(out, x0, y0, x1, y0, colors[c])
            _fill(out, x0, y1, x1, y1, colors[c])
            _fill(out, x0, y0, x0, y1, colors[c])
            _fill(out, x1, y0, x1, y1, colors[c])
            if y0 == y1:                                   # ImageDraw's vertical strokes run from y0 + 1 to y1: a height-0 outline also paints the row below at its ends
                _fill(out, x0, y0 + 1, x0, y0 + 1, colors[c])
                _fill(out, x1, y0 + 1, x1, y0 + 1, colors[c])
        _fill(out, org_x, org_y, org_x + lw, org_y + lh, colors[c])
        mask = blob[off:off + mw * mh].reshape(mh, mw).astype(np.int64)
        for my in range(mh):
            y = org_y + oy + my
            if not 0 <= y < H:
                continue
            for mx in range(mw):
                x = org_x + ox + mx
                if 0 <= x < W:
                    a = mask[my, mx]
                    for ch in range(3):
                        t1, t2 = int(out[y, x, ch]) * (255 - a) + 128, ink[ch] * a + 128
                        out[y, x, ch] = (((t1 >> 8) + t1) >> 8) + (((t2 >> 8) + t2) >> 8)
    return out


def draw_pil(img, rows, font, thickness, names=NAMES, colors=COLORS, skip_ids=(1,), ink=(0, 0, 0)):
    """the same rules with PIL doing the painting: `font` an ImageFont; crossed rings are left out (current Pillow raises on them)"""
    from PIL import Image, ImageDraw
    canvas = Image.fromarray(img)
    pen = ImageDraw.Draw(canvas)
    H, W = img.shape[:2]
    for row in np.asarray(rows, np.float32):
        c = kept(row, len(names), skip_ids)
        if c is None:
            continue
        y0, x0, y1, x1 = (int(np.clip(np.floor(v), -2 ** 24, 2 ** 24)) for v in row[:4])
        y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, H), min(x1, W)
        text = f'{names[c]} {np.float32(row[4]) * np.float32(row[5]):.2f}'
        tw, th = pen.textbbox((0, 0), text, font=font)[2:]
        at = (x0, y0 - th) if y0 >= th else (x0, y0 + 1)
        fill = tuple(int(v) for v in colors[c])
        for i in range(thickness):
            if x1 - i >= x0 + i and y1 - i >= y0 + i:
                pen.rectangle((x0 + i, y0 + i, x1 - i, y1 - i), outline=fill)
        pen.rectangle((at[0], at[1], at[0] + tw, at[1] + th), fill=fill)
        pen.text(at, text, fill=tuple(ink), font=font)
    return np.array(canvas)
