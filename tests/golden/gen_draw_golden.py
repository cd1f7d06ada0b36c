"""Writes tests/golden/draw.npz: what the reference's own drawing statements leave on every case of tests/draw_cases.py, the label atlases the cases need, the
reference's box colours for a few class counts, and a checksum of each case's inputs.

    python tests/golden/gen_draw_golden.py

Runs ONLY where the reference exists (ACHELOUS_REFERENCE, default /root/reference) and Pillow has FreeType.  Nothing of the reference's text is stored: the drawing
loop (achelous.py, from `for i, c in list(enumerate(top_label)):` to `del draw`) and the colour lines (from `hsv_tuples =` to the second `self.colors =`) are read from
the checkout and EXECUTED here, with three adaptations to today's Pillow and to a font-less setting: `draw.textsize(label, font)` becomes `draw.textbbox((0, 0), label,
font)[2:4]` (what the removed call returned), the `ImageDraw.Draw` the loop makes skips a rectangle whose corners have crossed (current Pillow raises there), and the
font is ImageFont.load_default(size).  Rows the reference never meets (a class id outside the class list, a non-finite number) are taken out before the loop runs.

Before anything is written it asserts, on every frame of every case, that the numpy restatement `draw_cases.draw_numpy` — fed with the atlas arrays
`achelous_amd.prepost.LabelAtlas` built — and the project's own PIL driver `draw_cases.draw_pil` equal the reference's image byte for byte."""
import colorsys
import contextlib
import io
import os
import sys
import types

import numpy as np
from PIL import Image, ImageDraw, ImageFont

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import draw_cases as DC                                    # noqa: E402
from achelous_amd.prepost import LabelAtlas                # noqa: E402

REF = os.environ.get('ACHELOUS_REFERENCE', '/root/reference')


def _lines(first, last):
    """the reference's lines up to the first that starts with `last`, from the nearest line before it that starts with `first`, dedented"""
    with open(os.path.join(REF, 'achelous.py'), encoding='utf-8') as f:
        src = f.read().split('\n')
    b = next(i for i, ln in enumerate(src) if ln.strip().startswith(last))
    a = max(i for i in range(b) if src[i].strip().startswith(first))
    n = len(src[a]) - len(src[a].lstrip())
    assert all(not ln[:n].strip() for ln in src[a:b + 1])
    return '\n'.join(ln[n:] for ln in src[a:b + 1])


class _Draw(ImageDraw.ImageDraw):
    def rectangle(self, xy, *args, **kw):
        x0, y0, x1, y1 = xy if len(xy) == 4 else (*xy[0], *xy[1])
        if x1 >= x0 and y1 >= y0:
            super().rectangle(xy, *args, **kw)


def reference_colors(n):
    me = types.SimpleNamespace(num_classes=n)
    code = _lines('hsv_tuples =', 'self.colors = list(map(lambda x: (int(')
    assert code.count('\n') == 2, code
    exec(compile(code, 'achelous.py', 'exec'), {'colorsys': colorsys, 'self': me})
    return np.array(me.colors, dtype=np.uint8).reshape(n, 3)


_LOOP = None


def reference_draw(img, rows, font, thickness):
    global _LOOP
    if _LOOP is None:
        code = _lines('for i, c in list(enumerate(top_label)):', 'del draw')
        assert code.count('draw.textsize(label, font)') == 1
        _LOOP = compile(code.replace('draw.textsize(label, font)', 'draw.textbbox((0, 0), label, font)[2:4]'), 'achelous.py', 'exec')
    rows = np.asarray([r for r in np.asarray(rows, np.float32) if DC.kept(r, len(DC.NAMES), ()) is not None], np.float32).reshape(-1, 7)
    me = types.SimpleNamespace(class_names=list(DC.NAMES), colors=[tuple(int(v) for v in c) for c in reference_colors(len(DC.NAMES))])
    ns = {'np': np, 'self': me, 'image': Image.fromarray(img), 'font': font, 'thickness': thickness, 'ImageDraw': types.SimpleNamespace(Draw=_Draw),
          'top_label': np.array(rows[:, 6], dtype='int32'), 'top_conf': rows[:, 4] * rows[:, 5], 'top_boxes': rows[:, :4]}
    with contextlib.redirect_stdout(io.StringIO()):
        exec(_LOOP, ns)
    return np.array(ns['image'])


def main():
    out = {}
    for n in DC.COLOR_COUNTS:
        out[f'colors/{n}'] = reference_colors(n)
    assert [tuple(int(v) for v in c) for c in out['colors/3']] == list(DC.COLORS)
    atlases = {s: LabelAtlas(DC.NAMES, s) for s in DC.FONT_SIZES}
    for s, a in atlases.items():
        out[f'atlas/{s}/table'], out[f'atlas/{s}/blob'] = a.table, a.blob
    changed = 0
    for name in DC.CASES:
        case = DC.make_case(name)
        out[f'{name}/checksum'] = np.array([DC.checksum(case)], np.int64)
        for b, img in enumerate(case['images']):
            size, thick = DC.font_size_of(case, b), DC.thickness_of(case, b)
            rows = case['rows'][b, :case['counts'][b]]
            want = reference_draw(img, rows, ImageFont.load_default(size), thick)
            bad = [int((want != got).any(axis=2).sum()) for got in (DC.draw_numpy(img, rows, atlases[size].table, atlases[size].blob, thick),
                                                                    DC.draw_pil(img, rows, ImageFont.load_default(size), thick))]
            mask = (want != img).any(axis=2)                # the background is noise: only the changed pixels are stored (draw_cases.expected puts them back)
            print(f'{name}[{b}] {img.shape[0]} x {img.shape[1]} font {size} thickness {thick}: {int(mask.sum())} pixels changed, {bad[0]} differ from numpy, {bad[1]} from draw_pil')
            assert bad == [0, 0], (name, b, bad)
            changed += int(mask.sum())
            out[f'{name}/{b}'], out[f'{name}/{b}/changed'] = want * mask[..., None], np.packbits(mask)
    path = os.path.join(HERE, 'draw.npz')
    np.savez_compressed(path, **out)
    print(f'{changed} pixels changed in all, 0 differing; {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
