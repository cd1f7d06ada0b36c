#!/usr/bin/env python3
"""tests/golden/heatmap.npz: what the reference's heat-map mode computes on the cases of tests/heatmap_cases.py.

The mask loop of achelous.detect_heatmap (achelous.py:457-459 the sigmoid, 539-546 the loop over the three outputs) is read out of the reference's SOURCE — achelous.py
imports cv2, which is not installed where the fixtures are made, so the module is parsed, not imported — and the statements themselves are executed, with `cv2.resize`
bound to `oracle.prepost.resize_linear` (OpenCV's INTER_LINEAR restated).  Stored per case: the logits (int8 eighths; 'nd1' reads the first two channels of 'nd7'), the reference's float32 scores (what it hands
to cv2.resize), per frame the mask, (lo, hi) and the colour pictures `matplotlib.cm.jet(Normalize(lo, hi)(mask), bytes=True)` blended over the base image with a real
`PIL.Image.blend` for every alpha of heatmap_cases.ALPHAS (asserted equal to the restatement on every case, stored for heatmap_cases.COLOUR_CASE); once: the base images, matplotlib's jet table, and
    e_ref = the largest |float32 score - float64 score| over every cell of every case, both from the reference's own expression,
the unit of the score tolerance in tests/test_heatmap.py.  The generator also asserts what that test relies on: the reference's float32 mask differs from the mask of
the float64 evaluation only where the float64 value of resize * 255 lies within 255 * 4 * e_ref of an integer, by exactly 1, on at most 1 % of a frame's pixels.

    python tests/golden/gen_heatmap_golden.py <directory of the reference checkout>"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import heatmap_cases as HC                    # noqa: E402
from oracle.prepost import resize_linear      # noqa: E402


def mask_statements(path):
    """the nested `sigmoid` and the statements from `mask = np.zeros(...)` to the end of the `for sub_output in outputs` loop of detect_heatmap, compiled"""
    tree = ast.parse(open(path, encoding='utf-8').read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == 'detect_heatmap')
    sig = next(n for n in fn.body if isinstance(n, ast.FunctionDef) and n.name == 'sigmoid')
    first = next(i for i, n in enumerate(fn.body) if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', None) == 'mask')
    loop = next(i for i, n in enumerate(fn.body) if isinstance(n, ast.For) and getattr(n.iter, 'id', None) == 'outputs')
    assert loop == first + 1, 'achelous.py: the mask loop no longer follows the mask'
    mod = ast.Module(body=[sig, fn.body[first], fn.body[loop]], type_ignores=[])
    return compile(ast.fix_missing_locations(mod), path, 'exec'), (sig.lineno, fn.body[first].lineno, fn.body[loop].end_lineno)


class _Image:
    def __init__(self, H, W):
        self.size = (W, H)


class _Cv2:
    """cv2 for the executed statements: resize = oracle.prepost.resize_linear (float64 inputs, of the error analysis, through heatmap_cases' float64 form); keeps what it was given"""

    def __init__(self, R):
        self.R, self.seen = R, []

    def resize(self, score, size):
        self.seen.append(score)
        W, H = size
        if score.dtype == np.float32:
            return resize_linear(score[..., None], H, W)[..., 0]
        return HC.resize_level(score, H, W, self.R // score.shape[0], (0, 0, self.R, self.R), np.float64)


def run_reference(code, dets, b, R, H, W):
    """the statements on frame b of `dets`; returns (mask float64 [H, W], the score maps cv2.resize was given)"""
    cv2 = _Cv2(R)
    ns = {'np': np, 'cv2': cv2, 'image': _Image(H, W), 'outputs': [d[b:b + 1] for d in dets]}
    exec(code, ns)
    return ns['mask'], cv2.seen


if __name__ == '__main__':
    import matplotlib
    from matplotlib import cm
    from matplotlib.colors import Normalize
    from PIL import Image
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ACHELOUS_REFERENCE', '')
    code, lines = mask_statements(os.path.join(ref, 'achelous.py'))
    out = {'source_lines': np.asarray(lines, np.int32), 'jet': cm.jet(np.arange(256), bytes=True)[:, :3].astype(np.uint8)}
    for b in range(len(HC.SHAPES)):
        out[f'base/{b}'] = HC.make_base(b)
    runs, e_ref = {}, 0.0
    for name, c in HC.CASES.items():
        R = c['R']
        eighths = HC.make_case(name)
        if name != 'nd1':
            out[f'{name}/logits8'] = eighths
        d32, d64 = HC.det_maps(eighths, R, np.float32), HC.det_maps(eighths, R, np.float64)
        s32 = np.zeros((len(c['frames']), sum(HC.cells(R))), np.float32)
        rng_ = np.zeros((len(c['frames']), 2), np.int32)
        for i, fb in enumerate(c['frames']):
            H, W = HC.SHAPES[fb]
            m32, seen32 = run_reference(code, d32, i, R, H, W)
            m64, seen64 = run_reference(code, d64, i, R, H, W)
            assert all(s.dtype == np.float32 for s in seen32) and all(s.dtype == np.float64 for s in seen64)
            s32[i] = np.concatenate([s.reshape(-1) for s in seen32])
            s64 = np.concatenate([s.reshape(-1) for s in seen64])
            e_ref = max(e_ref, float(np.abs(s32[i].astype(np.float64) - s64).max()))
            mask = m32.astype(np.uint8)
            assert np.array_equal(mask, m32) and np.array_equal(mask, HC.mask_from_scores(s32[i], R, H, W)), 'the restatement is not the reference'
            lo, hi = int(mask.min()), int(mask.max())
            out[f'{name}/mask/{i}'], rng_[i] = mask, (lo, hi)
            rgb = cm.jet(Normalize(lo, hi)(m32), bytes=True)[..., :3]           # the float64 mask, as the reference hands it to imshow
            assert np.array_equal(rgb, out['jet'][HC.colour_index(mask, lo, hi)])
            for alpha in HC.ALPHAS:
                pic = np.asarray(Image.blend(Image.fromarray(out[f'base/{fb}']), Image.fromarray(np.ascontiguousarray(rgb)), alpha))
                assert np.array_equal(pic, HC.colour(mask, lo, hi, out[f'base/{fb}'], out['jet'], alpha))
                if name == HC.COLOUR_CASE:                                       # (the assertion above holds every case; one case's pictures are stored)
                    out[f'{name}/colour/{alpha}/{i}'] = pic
            runs[(name, i)] = (m32, m64, HC.level_values(s64, R, H, W, None, np.float64))
        out[f'{name}/scores'], out[f'{name}/range'] = s32, rng_
    out['e_ref'] = np.asarray([e_ref], np.float64)
    for (name, i), (m32, m64, v64) in runs.items():
        diff = m32 != m64
        near = (np.abs(v64 - np.round(v64)) <= 255 * 4 * e_ref).any(0)
        assert np.all(np.abs(m32 - m64)[diff] == 1) and np.all(near[diff]) and diff.sum() <= 0.01 * diff.size, (name, i, int(diff.sum()))
    path = os.path.join(HERE, 'heatmap.npz')
    np.savez_compressed(path, **out)
    print('wrote heatmap.npz:', os.path.getsize(path), 'bytes; e_ref', e_ref, '; matplotlib', matplotlib.__version__, '; source lines', lines)
