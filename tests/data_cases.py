"""Inputs and host restatements shared by tests/test_data.py, tests/golden/gen_data_golden.py and profiles/scripts/data_timing.py.

The inputs are seeded and regenerated wherever they are needed; tests/golden/data.npz stores their checksum and what the reference's dataset + collate computed on
them.  The restatements here are independent of achelous_amd/data.py: `nearest_index` (Pillow's NEAREST rule; the generator checks it against PIL itself) and
`pil_frame` (the reference's per-frame host path with PIL, for the general-placement fixtures and the host leg of the timing script)."""
import numpy as np

FEATURES = ['x', 'y', 'z', 'comp_velocity', 'rcs']
NUM_SEG = 9
NUM_POINTS = 64

# (H, W) of every frame; the label maps have the image's size.  `w_map`: the frame has a water-line map.  Boxes: x1, y1, x2, y2, class in original pixels.
BATCHES = {
    'r96': dict(R=96, frames=[
        # 135 x 240 -> nw 96, nh 54, dx 0, dy 21 (x scale 0.4): corners past the image / negative, zero width, widths that truncate to exactly 1 (dropped) and 2 (kept)
        dict(hw=(135, 240), w_map=True, cloud=700,
             boxes=[(-20, -10, 100, 60, 0), (200, 100, 300, 180, 1), (50, 20, 50, 90, 2), (10, 10, 13, 100, 3), (10, 10, 15, 100, 4), (30, 40, 200, 44, 5), (5, 5, 235, 130, 6)]),
        # 200 x 90 portrait -> nw 43, nh 96, dx 26, dy 0; no water-line map
        dict(hw=(200, 90), w_map=False, cloud=3, boxes=[(-60, -5, 30, 50, 1), (10, 20, 80, 190, 0), (85, 150, 140, 260, 2), (40, 40, 41, 100, 3)]),
        # 40 x 30 up-scale -> nw 72, nh 96, dx 12
        dict(hw=(40, 30), w_map=True, cloud=40, boxes=[(0, 0, 30, 40, 6), (3, 4, 4, 30, 5), (29, 0, 30, 40, 4)]),
        # 3 x 5 tiny -> nw 96, nh 57; no boxes
        dict(hw=(3, 5), w_map=True, cloud=17, boxes=[]),
    ]),
    'r64': dict(R=64, frames=[dict(hw=(64, 64), w_map=True, cloud=64, boxes=[(0, 0, 64, 64, 0), (10, 12, 11, 40, 1), (62, 60, 70, 70, 2)])]),
}

# general placements (nw, nh, dx, dy) at R = 96 on the r96 frames + one more: dx < 0, overhang right / bottom, nw > R, wholly outside, nw == iw
PLACEMENTS = [(80, 50, -30, -7), (60, 70, 50, 60), (130, 150, -20, -30), (20, 30, 96, 10), (90, 200, 3, -100)]
PLACEMENT_FRAMES = [0, 1, 2, 3, 1]


def make_frame(batch, index):
    """seeded image [H, W, 3], label maps [H, W] (values above the class counts, 255 among them; None without a water-line map), cloud [n, 5] float64, point labels,
    radar map [3, R, R] float64"""
    cfg = BATCHES[batch]
    f = cfg['frames'][index]
    H, W = f['hw']
    rng = np.random.default_rng([sorted(BATCHES).index(batch), index, 20])
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 11 + 90) % 256, (xx * yy + 31) % 256], -1)
    image = np.clip(base + rng.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)
    image.reshape(-1)[:4] = (0, 255, 0, 255)
    png = rng.integers(0, NUM_SEG + 4, (H, W)).astype(np.uint8)
    png.reshape(-1)[::5] = 255
    png_w = rng.integers(0, 5, (H, W)).astype(np.uint8)
    png_w.reshape(-1)[::7] = 255
    cloud = rng.normal(size=(f['cloud'], len(FEATURES))) * np.array([30.0, 8.0, 2.0, 5.0, 12.0])
    cloud = np.round(cloud * 64) / 64                    # exact in binary and short in decimal: a .csv round trip keeps every bit
    plab = rng.integers(0, 8, f['cloud'])
    radar = rng.random((3, cfg['R'], cfg['R']))
    return dict(image=image, png=png, png_w=png_w if f['w_map'] else None, boxes=np.array(f['boxes'], np.int64).reshape(-1, 5), points=cloud, point_labels=plab, radar=radar)


def checksum(frames):
    s = 0.0
    for f in frames:
        for k in ('image', 'png', 'png_w', 'points', 'point_labels', 'radar'):
            if f[k] is not None:
                a = np.asarray(f[k], np.float64).reshape(-1)
                s += float((a * (np.arange(a.size) % 251 + 1)).sum())
    return s


def nearest_index(in_size, out_size):
    """PIL Image.NEAREST along one axis: a running sum in double, truncated per sample"""
    a = in_size / out_size
    xx = 0.5 * a
    out = []
    for _ in range(out_size):
        out.append(int(xx))
        xx += a
    return np.array(out, np.int64)


def nearest_resize(m, nw, nh):
    return m[nearest_index(m.shape[0], nh)][:, nearest_index(m.shape[1], nw)]


def paste(canvas, src, dx, dy):
    """Image.paste's clipping in numpy"""
    R = canvas.shape[0]
    nh, nw = src.shape[:2]
    x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + nw, R), min(dy + nh, R)
    if x0 < x1 and y0 < y1:
        canvas[y0:y1, x0:x1] = src[y0 - dy:y1 - dy, x0 - dx:x1 - dx]
    return canvas


def letterbox(iw, ih, R):
    scale = min(R / iw, R / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return nw, nh, (R - nw) // 2, (R - nh) // 2


def pil_frame(image, png, png_w, R, num_seg, placement=None):
    """the host path per frame with PIL: (canvas uint8 [R, R, 3], normalised fp32 [3, R, R], png [R, R], png_w [R, R])"""
    from PIL import Image
    ih, iw = image.shape[:2]
    nw, nh, dx, dy = placement or letterbox(iw, ih, R)
    canvas = Image.new('RGB', (R, R), (128, 128, 128))
    canvas.paste(Image.fromarray(image).resize((nw, nh), Image.BICUBIC), (dx, dy))
    canvas = np.array(canvas)
    x = np.array(canvas, dtype=np.float64)
    x /= 255.0
    x -= np.array([0.485, 0.456, 0.406])
    x /= np.array([0.229, 0.224, 0.225])
    outs = []
    for m, n in ((png, num_seg), (png_w, 2)):
        lab = Image.new('L', (R, R), 0)
        if m is not None:
            lab.paste(Image.fromarray(m).resize((nw, nh), Image.NEAREST), (dx, dy))
        lab = np.array(lab)
        lab[lab >= n] = n
        outs.append(lab)
    return canvas, np.transpose(x, (2, 0, 1)).astype(np.float32), outs[0], outs[1]
