#!/usr/bin/env python3
"""tests/golden/scatter.npz: what the reference's point-class scatter computes on the cases of tests/scatter_cases.py.

The statements of achelous.detect_image that make the table (achelous.py:262-268: the arg-max of the point head, the concatenation of u, v, rcs and class, np.unique)
are read out of the reference's SOURCE — achelous.py imports cv2, which is not installed where the fixtures are made, so the module is parsed, not imported — and the
statements themselves are executed, per frame of every case, on the case's (u, v, rcs) columns at the sampled rows and on logits whose arg-max is the case's classes.
The samples our rule drops (a non-finite u, v or s, a class outside [0, num_classes), an index outside the cloud) are taken out first: the reference has no rule for
them.  Stored per case and frame: the rows; for the cases drawn with the default colours also `matplotlib.cm.viridis(Normalize(c.min(), c.max())(c), bytes=True)` of
the rows' classes.  Once: matplotlib's 256-entry viridis table, and the colours matplotlib gives every class c of every range 0 <= lo <= c <= hi <= 16.

    python tests/golden/gen_scatter_golden.py <directory of the reference checkout>"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import scatter_cases as SC                    # noqa: E402

NAMES = ('output_seg_pc_cls', 'output_seg_pc_collections')


def table_statements(path):
    """the assignments to output_seg_pc_cls and output_seg_pc_collections in detect_image, in source order, compiled"""
    tree = ast.parse(open(path, encoding='utf-8').read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == 'detect_image')
    body = sorted((n for n in ast.walk(fn) if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', None) in NAMES), key=lambda n: n.lineno)
    assert [n.targets[0].id for n in body] == [NAMES[0], NAMES[1], NAMES[1]], 'achelous.py: the point-class table is no longer made by three statements'
    return compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, 'exec'), (body[0].lineno, body[-1].end_lineno)


def run_reference(code, kept, num_classes):
    """the statements on the kept samples [M, 4] = (u, v, s, c)"""
    import torch
    logits = torch.full((len(kept), num_classes), -1.0)
    logits[torch.arange(len(kept)), torch.from_numpy(kept[:, 3].astype(np.int64))] = 1.0
    ns = {'np': np, 'torch': torch, 'output_seg_pc': logits, 'radar_pc_u': kept[:, 0:1], 'radar_pc_v': kept[:, 1:2], 'radar_pc_power': kept[:, 2:3]}
    exec(code, ns)
    return ns['output_seg_pc_collections']


if __name__ == '__main__':
    import matplotlib
    from matplotlib import cm
    from matplotlib.colors import Normalize
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ACHELOUS_REFERENCE', '')
    code, lines = table_statements(os.path.join(ref, 'achelous.py'))
    out = {'source_lines': np.asarray(lines, np.int32), 'viridis': cm.viridis(np.arange(256), bytes=True)[:, :3].astype(np.uint8)}
    rule = np.zeros((17, 17, 17, 3), np.uint8)
    for lo in range(17):
        for hi in range(lo, 17):
            c = np.arange(lo, hi + 1, dtype=np.float64)
            rule[lo, hi, lo:hi + 1] = cm.viridis(Normalize(lo, hi)(c), bytes=True)[:, :3]
            assert np.array_equal(rule[lo, hi, lo:hi + 1], out['viridis'][SC.colour_index(c, lo, hi)]), (lo, hi)
    out['index_rule'] = rule
    for name in SC.CASE_NAMES:
        c = SC.case(name)
        for i in range(len(c['frames'])):
            kept = SC.gather(c['clouds'][i], c['indices'][i], c['classes'][i], SC.NUM_CLASSES, c['columns'] or (2, 3, 4))
            rows = run_reference(code, kept, SC.NUM_CLASSES) if len(kept) else np.zeros((0, 4))
            assert rows.dtype == np.float64 and np.array_equal(rows, SC.unique_rows(kept)), 'the restatement is not the reference'
            out[f'{name}/rows/{i}'] = rows
            if name in SC.FIXTURE_COLOUR_CASES and len(rows):
                k = rows[:, 3]
                out[f'{name}/colours/{i}'] = cm.viridis(Normalize(k.min(), k.max())(k), bytes=True)[:, :3].astype(np.uint8)
    path = os.path.join(HERE, 'scatter.npz')
    np.savez_compressed(path, **out)
    print('wrote scatter.npz:', os.path.getsize(path), 'bytes; matplotlib', matplotlib.__version__, '; source lines', lines)
