#!/usr/bin/env python3
"""Generate tests/golden/radar_maps.npz by EXECUTING the loop cell of the reference's radar_feature_map_generate.ipynb (read-only) on the seeded clouds of
tests/radar_cases.py.

Runs ONLY where the reference exists (ACHELOUS_REFERENCE, default /root/reference).  Nothing of the notebook's text is stored: the fixture holds the checksum of
the inputs and the maps the cell wrote for them.  The cell is found by the name of its map variable and run in a namespace whose file I/O is replaced:
`pd.read_csv` hands out the case's clouds (the cell selects its five feature columns by name), `np.savez_compressed` collects the maps, `os.path.join` and
`tqdm` are inert, and `resolution` is the case's R (the notebook's own cell says 320).  Each case runs twice: on the float64 clouds, and on the clouds rounded
to float32 (what the kernel computes from a float32 upload).
ASSERTED here, not stored: the restatement of tests/radar_cases.py gives the same maps, bit for bit, NaN for NaN.
"""
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('ACHELOUS_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'tests')]

import radar_cases as RC                                                    # noqa: E402


def _loop_cell():
    with open(os.path.join(REF, 'radar_feature_map_generate.ipynb')) as f:
        nb = json.load(f)
    cells = [''.join(c['source']) for c in nb['cells'] if c['cell_type'] == 'code']
    loop = [s for s in cells if 'example_radar_map' in s and 'for ' in s]
    assert len(loop) == 1, 'the notebook no longer has exactly one rasterising cell'
    return loop[0]


def run_notebook(clouds, R):
    """the notebook's cell on `clouds` (float64 [n, 5] in its feature order) -> list of float64 [3, R, R]"""
    saved = {}

    class Frame:
        def __init__(self, a):
            self.a = a

        def __getitem__(self, cols):
            assert list(cols) == RC.FEATURES
            return self

        def to_numpy(self):
            return self.a

    class Numpy:
        def __getattr__(self, k):
            return getattr(np, k)

        def savez_compressed(self, path, arr):
            saved[int(path.split('/')[-1][:-4])] = np.array(arr)

    ns = dict(pd=types.SimpleNamespace(read_csv=lambda path: Frame(clouds[int(path.split('/')[-1][:-4])])), np=Numpy(),
              os=types.SimpleNamespace(path=types.SimpleNamespace(join=lambda a, b: a + '/' + b)), tqdm=lambda x: x, radar_root='in', save_radar_map_root='out',
              radar_files=['%d.csv' % i for i in range(len(clouds))], features_list=list(RC.FEATURES), resolution=R)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        exec(compile(_loop_cell(), 'radar_feature_map_generate.ipynb', 'exec'), ns)
    return [saved[i] for i in range(len(clouds))]


def main():
    out = {}
    for name, cfg in RC.CASES.items():
        clouds = RC.make_clouds(name)
        out[f'{name}/checksum'] = np.array([RC.checksum(clouds)])
        cols = list(RC.map_columns(name))
        for tag, dtype in (('f64', np.float64), ('f32', np.float32)):
            _, truth_from = RC.as_input(clouds, dtype)
            maps = np.stack(run_notebook([c[:, cols] for c in truth_from], cfg['R']))
            assert maps.shape == (len(clouds), 3, cfg['R'], cfg['R']) and maps.dtype == np.float64
            assert np.array_equal(maps, RC.rasterise_batch(truth_from, cfg['R'], cols), equal_nan=True), (name, tag)
            out[f'{name}/{tag}/maps'] = maps
            print(name, tag, 'non-zero cells per frame', [int((m != 0).sum()) for m in maps])
    path = os.path.join(HERE, 'radar_maps.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
