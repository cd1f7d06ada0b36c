#!/usr/bin/env python3
"""Generate tests/golden/data.npz by IMPORTING the reference's dataset and collate function (read-only) on the CPU.

Runs ONLY where the reference exists (ACHELOUS_REFERENCE, default /root/reference).  Nothing of the reference's program text is stored: the fixture holds the checksum
of the seeded inputs of tests/data_cases.py and what `utils.dataloader.YoloDataset` + `yolo_dataset_collate_all` return for them.
  * The inputs are written to a temporary folder as the files the dataset reads: PNG images, label PNGs (one frame has no water-line map: the dataset's own
    fallback runs), `.npz` radar maps, `.csv` point clouds.
  * `cv2` and `albumentations` are imported by utils/dataloader.py at module level and never used on its live path; neither is installed, so empty stand-ins are
    placed in `sys.modules` (the albumentations one accepts the three module-level `Compose(...)` constructions).
  * `np.random.choice` is wrapped to record the point indices the dataset draws.  The dataset also shuffles the boxes: the tests compare them as a multiset.
Also recorded: PIL's own `resize` + `paste` for the general placements of tests/data_cases.py (which the reference never uses).
ASSERTED here, not stored: the NEAREST restatement of tests/data_cases.py equals PIL on in, out < 200, 1920 and 1080 to every third width below 700, 300 .. 4200 to
320, and on 2-D `L` images; the radar maps pass through as their float32 cast; the `.csv` round trip keeps every bit of the clouds.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('ACHELOUS_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'tests'), REPO, REF]

import data_cases as DC                                                     # noqa: E402


def _reference():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    alb = types.ModuleType('albumentations')
    for name in ('Compose', 'RandomRain', 'RandomSunFlare', 'RandomFog'):
        setattr(alb, name, lambda *a, **k: None)
    sys.modules.setdefault('albumentations', alb)
    import matplotlib
    matplotlib.use('Agg')
    from utils import dataloader as DL                                      # the reference (never copied)
    return DL


def check_nearest():
    from PIL import Image

    def pil_index(n_in, n_out):
        src = Image.fromarray(np.arange(n_in, dtype=np.int32).reshape(1, n_in))
        return np.array(src.resize((n_out, 1), Image.NEAREST)).reshape(-1)
    pairs = [(i, o) for i in range(1, 200) for o in range(1, 200)]
    pairs += [(i, o) for i in (1920, 1080) for o in range(1, 700, 3)] + [(i, 320) for i in range(300, 4201)]
    bad = [(i, o) for i, o in pairs if not np.array_equal(pil_index(i, o), DC.nearest_index(i, o))]
    assert not bad, bad[:5]
    closed = sum(not np.array_equal(np.floor((np.arange(o) + 0.5) * i / o).astype(np.int64), DC.nearest_index(i, o)) for i, o in pairs)
    rng = np.random.default_rng(1)
    for h, w, nh, nw in ((2, 7, 7, 2), (135, 240, 54, 96), (200, 90, 96, 43), (3, 5, 57, 96), (17, 33, 90, 200)):
        m = rng.integers(0, 256, (h, w)).astype(np.uint8)
        assert np.array_equal(np.array(Image.fromarray(m).resize((nw, nh), Image.NEAREST)), DC.nearest_resize(m, nw, nh)), (h, w, nh, nw)
    print(f'NEAREST: {len(pairs)} (in, out) pairs equal PIL; floor((x + 0.5) * in / out) differs on {closed} of them')


def run_batch(DL, name, out):
    from PIL import Image
    import pandas as pd
    cfg = DC.BATCHES[name]
    R = cfg['R']
    frames = [DC.make_frame(name, i) for i in range(len(cfg['frames']))]
    out[f'{name}/checksum'] = np.array([DC.checksum(frames)])
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {k: os.path.join(tmp, k) for k in ('img', 'seg', 'wl', 'radar', 'pc')}
        for d in dirs.values():
            os.makedirs(d)
        lines = []
        for i, f in enumerate(frames):
            stem = f'f{i}'
            Image.fromarray(f['image']).save(os.path.join(dirs['img'], stem + '.png'))
            Image.fromarray(f['png']).save(os.path.join(dirs['seg'], stem + '.png'))
            if f['png_w'] is not None:
                Image.fromarray(f['png_w']).save(os.path.join(dirs['wl'], stem + '.png'))
            np.savez(os.path.join(dirs['radar'], stem + '.npz'), f['radar'])
            df = pd.DataFrame(f['points'], columns=DC.FEATURES)
            df['label'] = f['point_labels']
            path = os.path.join(dirs['pc'], stem + '.csv')
            df.to_csv(path)
            assert np.array_equal(np.asarray(pd.read_csv(path, index_col=0)[DC.FEATURES]), f['points'])
            lines.append(' '.join([os.path.join(dirs['img'], stem + '.png')] + [','.join(str(int(v)) for v in b) for b in f['boxes']]))
        ds = DL.YoloDataset(lines, [R, R], 7, DC.NUM_SEG, 1, dirs['radar'], False, False, 0.0, 0.0, dirs['seg'], dirs['wl'], dirs['pc'], False, DC.FEATURES,
                            is_radar_pc_seg=True, radar_pc_num=DC.NUM_POINTS)
        drawn = []
        choice = np.random.choice

        def recording(*a, **k):
            r = choice(*a, **k)
            drawn.append(np.array(r))
            return r
        np.random.seed(7)
        np.random.choice = recording
        try:
            items = [ds[i] for i in range(len(frames))]
        finally:
            np.random.choice = choice
        images, bboxes, radars, pngs, pngs_w, _, _, pc, pc_labels = DL.yolo_dataset_collate_all(items)
    B = len(frames)
    assert np.array_equal(radars.numpy(), np.stack([f['radar'] for f in frames]).astype(np.float32))
    assert len(drawn) == B and int(pngs.max()) == DC.NUM_SEG and int(pngs_w.max()) == 2
    G = max(1, max(int(b.shape[0]) for b in bboxes))
    boxes = np.zeros((B, G, 5), np.float32)
    for b, t in enumerate(bboxes):
        if t.shape[0]:
            boxes[b, :t.shape[0]] = t.numpy()
    out[f'{name}/images'] = images.numpy()
    out[f'{name}/png'] = pngs.numpy().astype(np.uint8)
    out[f'{name}/png_w'] = pngs_w.numpy().astype(np.uint8)
    out[f'{name}/boxes'] = boxes
    out[f'{name}/counts'] = np.array([int(b.shape[0]) for b in bboxes], np.int32)
    out[f'{name}/points'] = pc.numpy()
    out[f'{name}/pc_labels'] = pc_labels.numpy().astype(np.int16)
    out[f'{name}/indices'] = np.stack(drawn).astype(np.int16)
    print(name, 'images', tuple(images.shape), 'boxes kept', out[f'{name}/counts'].tolist(), 'of', [len(f['boxes']) for f in frames],
          'frames without a water-line map:', [i for i, f in enumerate(frames) if f['png_w'] is None])


def run_placements(out):
    frames = [DC.make_frame('r96', i) for i in DC.PLACEMENT_FRAMES]
    res = [DC.pil_frame(f['image'], f['png'], f['png_w'], 96, DC.NUM_SEG, p) for f, p in zip(frames, DC.PLACEMENTS)]
    out['place/canvas'] = np.stack([r[0] for r in res])
    out['place/png'] = np.stack([r[2] for r in res])
    out['place/png_w'] = np.stack([r[3] for r in res])
    assert (out['place/canvas'][3] == 128).all() and not out['place/png'][3].any()          # the window wholly outside the canvas


def main():
    check_nearest()
    DL = _reference()
    out = {}
    for name in DC.BATCHES:
        run_batch(DL, name, out)
    run_placements(out)
    path = os.path.join(HERE, 'data.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
