"""The cases of tests/test_scatter.py and the point-class scatter restated in numpy and PIL (achelous_amd/csrc/k_scatter.h, prepost.scatter_points_frames; the
reference's achelous.py:261-271).

Inputs.  Frames (1, 1), (7, 9), (37, 53), (96, 131), (1, 300), (130, 70): widths that are no multiple of 4, more than one tile across and down.  Clouds are built from an
integer hash (no numpy random stream), on a grid of eighths, so float32 and float64 clouds hold the same values; special rows are written into fixed places: duplicates
of a row under another row number, -0.0 against 0.0, negative coordinates, NaN and +-inf in each of u, v, s, u = +-1e300, s = 0 and s < 0.  Indices are sampled with
replacement, one of them equal to n; classes include -1 and num_classes.

Oracle (independent of the kernel): rows by np.unique(axis=0) after the stated filter; coverage by the float64 expression dx * dx + dy * dy <= min(k * s, max_radius^2)
with s > 0, in numpy; colour by the integer index rule; paint by real PIL, row after row: Image.blend(img, solid colour, alpha) copied in under the row's mask."""
import numpy as np

SHAPES = ((1, 1), (7, 9), (37, 53), (96, 131), (1, 300), (130, 70))
NUM_CLASSES = 9
SENTINEL = 0xA5


def hashed(seed, n, top):
    """n integers in [0, top) from an integer hash of (seed, position): the same on every numpy"""
    x = np.arange(n, dtype=np.uint64) + np.full(n, seed, np.uint64) * np.uint64(0x9E3779B97F4A7C15)           # (array arithmetic wraps modulo 2^64)
    for _ in range(2):
        x ^= x >> np.uint64(31)
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(29)
        x = x * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(32)
    return (x % np.uint64(top)).astype(np.int64)


def make_base(b):
    """the image under the discs for frame b of SHAPES: every byte value reachable, from the hash"""
    H, W = SHAPES[b]
    return hashed(500 + b, H * W * 3, 256).astype(np.uint8).reshape(H, W, 3)


def _cloud(seed, n, H, W, F, cols, dtype, smax=1600, margin=10):
    """[n, F]: u in [-margin, W + margin), v in [-margin, H + margin) in eighths, s in [0, smax / 4) in quarters, the other columns noise; cols = (rcs, u, v)"""
    c = (hashed(seed, n * F, 4096).reshape(n, F) / 16.0).astype(np.float64)
    c[:, cols[1]] = hashed(seed + 1, n, 8 * (W + 2 * margin)) / 8.0 - margin
    c[:, cols[2]] = hashed(seed + 2, n, 8 * (H + 2 * margin)) / 8.0 - margin
    c[:, cols[0]] = hashed(seed + 3, n, smax) / 4.0
    return c.astype(dtype)


def _special(c, cols, W, H):
    """fixed places of a cloud of at least 40 rows get the rows that can go wrong"""
    r, u, v = cols
    c[1] = c[0]                                              # equal rows from different cloud rows
    c[2, [u, v, r]] = c[0, [u, v, r]]                        # ... and when only the other columns differ
    c[3, u], c[4, u] = c[5, u], c[5, u]                      # ties in u broken by v
    c[4, v] = c[5, v]                                        # ... then by s
    c[4, r] = c[5, r] + 1
    c[6, u], c[7, u] = 0.0, -0.0                             # -0.0 against 0.0: one row
    c[7, [v, r]] = c[6, [v, r]]
    c[8, u], c[8, v] = -3.5, -2.25                           # negative coordinates, still touching the frame
    c[8, r] = 400.0
    c[9, u], c[10, v], c[11, r] = np.nan, np.nan, np.nan
    c[12, u], c[13, v], c[14, r] = np.inf, np.inf, np.inf
    c[15, u], c[16, v], c[17, r] = -np.inf, -np.inf, -np.inf
    if c.dtype == np.float64:
        c[18, u], c[19, u], c[20, v] = 1e300, -1e300, 1e300
    else:
        c[18, u], c[19, u], c[20, v] = 3e38, -3e38, 3e38
    c[21, r], c[22, r] = 0.0, -4.0                           # s = 0 and s < 0: in the rows, cover nothing
    c[21, [u, v]] = (2.0, 0.0)                               # (s = 0 with its centre exactly on a pixel)
    c[23, [u, v, r]] = (W / 2.0, H / 2.0, 4.0 * 1e6)         # covers a lot: clamped by max_radius
    return c


def _case(name):
    F5, F4 = (2, 3, 4), (0, 3, 1)                            # (rcs, u, v): the default columns of a 5-column cloud; a 4-column cloud with its own
    if name in ('mix64', 'lo3', 'fixed', 'palette', 'mix64_f32'):
        frames, N, dtype, cols, F = (0, 1, 2, 3, 4, 5), 64, np.float32 if name == 'mix64_f32' else np.float64, F5, 5
        clouds, idx, cls = [], [], []
        for i, b in enumerate(frames):
            H, W = SHAPES[b]
            n = 48
            c = _special(_cloud(10 + i, n, H, W, F, cols, dtype), cols, W, H)
            if b == 0:
                c[:, cols[1]] = np.nan                       # a frame whose rows are all dropped
            j = hashed(40 + i, N, n)                         # with replacement: repeats
            j[:24] = np.arange(24)                           # every special row is sampled
            j[24:28] = (0, 0, 5, 5)                          # the same cloud row twice with one class and with two
            j[30] = n                                        # an index equal to n
            k = hashed(60 + i, N, NUM_CLASSES)
            k[24], k[25], k[26], k[27] = 2, 2, 1, 6
            k[7] = k[6]                                      # (the -0.0 row and the 0.0 row have one class)
            k[31], k[32] = -1, NUM_CLASSES
            if name == 'lo3':
                k = np.where((k >= 0) & (k < NUM_CLASSES), 3 + k % 5, k)
            clouds.append(c); idx.append(j); cls.append(k)
        style = {'fixed': dict(class_range=(2, 5)), 'palette': dict(colors=hashed(77, NUM_CLASSES * 3, 256).astype(np.uint8).reshape(-1, 3))}.get(name, {})
        return dict(frames=frames, N=N, clouds=clouds, indices=np.stack(idx), classes=np.stack(cls), style=style, columns=None)
    if name in ('mix5', 'one'):
        frames, N = (0, 1, 2, 3, 4, 5), 5 if name == 'mix5' else 1
        clouds, idx, cls = [], [], []
        for i, b in enumerate(frames):
            H, W = SHAPES[b]
            c = _cloud(100 + i, 7, H, W, 4, F4, np.float32, smax=400, margin=2)
            c[0, [F4[1], F4[2], F4[0]]] = (0.0, 0.0, 16.0)   # the (1, 1) frame is painted too
            clouds.append(c); idx.append(np.arange(N) * 3 % 7); cls.append(hashed(120 + i, N, NUM_CLASSES))
        return dict(frames=frames, N=N, clouds=clouds, indices=np.stack(idx), classes=np.stack(cls), style=dict(columns=F4), columns=F4)
    if name == 'identical':                                  # all rows identical: one row, one class, hi == lo
        frames, N = (1, 2), 64
        clouds = [np.tile(np.array([[1.0, 2.0, 36.0, 3.0, 4.0]]), (3, 1)) for _ in frames]
        return dict(frames=frames, N=N, clouds=clouds, indices=hashed(7, 2 * N, 3).reshape(2, N), classes=np.full((2, N), 4), style={}, columns=None)
    if name.startswith('order'):                             # 300 distinct rows that all cover pixel (4, 3): the order decides every byte
        frames, N = (1, 2), 300
        alpha = float(name[5:])
        clouds = []
        for i, b in enumerate(frames):
            c = np.zeros((N, 5))
            c[:, 3] = 4.0 + (hashed(200 + i, N, 17) - 8) / 8.0
            c[:, 4] = 3.0 + (hashed(210 + i, N, 17) - 8) / 8.0
            c[:, 2] = 36.0 + np.arange(N)                    # distinct
            clouds.append(c)
        return dict(frames=frames, N=N, clouds=clouds, indices=np.tile(np.arange(N)[::-1], (2, 1)),
                    classes=hashed(230, 2 * N, NUM_CLASSES).reshape(2, N), style=dict(alpha=alpha), columns=None)
    if name in ('geom', 'geom_r6'):
        frames, N = (3, 5, 2), 64
        clouds = []
        for i, b in enumerate(frames):
            H, W = SHAPES[b]
            c = _cloud(300 + i, N, H, W, 5, F5, np.float64, smax=200, margin=4)
            g = [(-40.0, -40.0, 100.0),                      # wholly outside
                 (W + 30.0, H / 2.0, 400.0),                 # wholly outside, to the right
                 (0.0, H / 2.0, 900.0),                      # half outside
                 (W - 1.0, H - 1.0, 256.0),                  # a quarter inside
                 (W / 2.0, H / 2.0, 4.0 * 65536.0),          # the whole frame (max_radius 256)
                 (10.0, 10.0, 20.0),                         # centre on a pixel, r2 = 5 exactly: the (1, 2) neighbours lie ON the circle
                 (20.0, 5.0, 4.0),                           # r2 = 1: the four neighbours
                 (63.5, 15.5, 36.0), (64.0, 16.0, 16.0),     # tile corners for every tile height the kernel may be built with
                 (63.5, 31.5, 36.0), (64.0, 64.0, 64.0), (63.75, 63.25, 100.0),
                 (30.0, 8.0, 0.0), (31.0, 8.0, -9.0),        # s = 0 on a pixel centre, s < 0
                 (5.25, 7.125, 2.0)]                         # smaller than a pixel's reach: may cover nothing
            for j, (u, v, s) in enumerate(g):
                c[j, [3, 4, 2]] = (u, v, s)
            clouds.append(c)
        style = dict(max_radius=256) if name == 'geom' else dict(max_radius=6, size_scale=1.5)
        return dict(frames=frames, N=N, clouds=clouds, indices=np.tile(np.arange(N), (3, 1)), classes=hashed(330, 3 * N, NUM_CLASSES).reshape(3, N), style=style, columns=None)
    if name == 'big4096':                                    # the largest N: eight sort slots per thread, sixteen chunks in the tile kernel
        frames, N, n = (2,), 4096, 3000
        H, W = SHAPES[2]
        c = _cloud(400, n, H, W, 5, F5, np.float32, smax=64, margin=6)
        return dict(frames=frames, N=N, clouds=[c], indices=hashed(401, N, n).reshape(1, N), classes=hashed(402, N, NUM_CLASSES).reshape(1, N), style={}, columns=None)
    raise KeyError(name)


CASE_NAMES = ('mix64', 'mix64_f32', 'lo3', 'fixed', 'palette', 'mix5', 'one', 'identical', 'order0.98', 'order0.5', 'order1.0', 'order0.0', 'geom', 'geom_r6', 'big4096')
FIXTURE_COLOUR_CASES = ('mix64', 'lo3', 'identical', 'geom', 'mix5')        # default colours: the fixture holds matplotlib's
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _case(name)
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------------ the oracle
def gather(cloud, idx, cls, num_classes, cols):
    """the kept samples of one frame as float64 [M, 4] = (u, v, s, c), unsorted: the stated filter"""
    n = cloud.shape[0]
    ok = (idx >= 0) & (idx < n) & (cls >= 0) & (cls < num_classes)
    safe = np.where(ok, idx, 0)
    if n == 0:
        return np.zeros((0, 4))
    r, cu, cv = cols
    u, v, s = (cloud[safe, k].astype(np.float64) for k in (cu, cv, r))
    ok &= np.isfinite(u) & np.isfinite(v) & np.isfinite(s)
    return np.stack([u, v, s, cls.astype(np.float64)], axis=1)[ok]


def unique_rows(t):
    return np.unique(t, axis=0) if len(t) else np.zeros((0, 4))


def colour_index(c, lo, hi):
    c = np.asarray(c, dtype=np.int64)
    return np.zeros_like(c) if hi == lo else np.minimum(((c - lo) * 256) // (hi - lo), 255)


def row_colours(rows, table, class_range=None, colors=None):
    """uint8 [M, 3] and the (lo, hi) of the rows' classes"""
    if not len(rows):
        return np.zeros((0, 3), np.uint8), (0, 0)
    c = rows[:, 3].astype(np.int64)
    lo, hi = int(c.min()), int(c.max())
    if colors is not None:
        return np.asarray(colors)[c], (lo, hi)
    if class_range is not None:
        return table[colour_index(np.clip(c, class_range[0], class_range[1]), class_range[0], class_range[1])], (lo, hi)
    return table[colour_index(c, lo, hi)], (lo, hi)


def coverage(u, v, s, H, W, size_scale, max_radius):
    """bool [H, W]: the float64 expression, every operation one rounded numpy operation"""
    if not s > 0:
        return np.zeros((H, W), bool)
    k = size_scale * size_scale / 4.0
    r2 = min(k * s, float(max_radius) * float(max_radius))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(over='ignore'):
        dx, dy = xx - u, yy - v
        return dx * dx + dy * dy <= r2


def paint(img, rows, colours, alpha, size_scale, max_radius):
    """the rows in order over `img` (uint8 [H, W, 3]) with real PIL blends; returns the new image and the union of the masks"""
    from PIL import Image
    H, W, _ = img.shape
    out, union = img.copy(), np.zeros((H, W), bool)
    for (u, v, s, _), col in zip(rows, colours):
        m = coverage(u, v, s, H, W, size_scale, max_radius)
        if not m.any():
            continue
        blended = np.asarray(Image.blend(Image.fromarray(out), Image.new('RGB', (W, H), tuple(int(x) for x in col)), alpha))
        out[m] = blended[m]
        union |= m
    return out, union


def oracle(name, table, frames=None):
    """per frame of the case (or of `frames`, positions in the case): dict(rows, count, range, image, union)"""
    c = case(name)
    st = dict(alpha=0.98, size_scale=1.0, max_radius=64)
    st.update({k: v for k, v in c['style'].items() if k in st})
    cols = c['columns'] or (2, 3, 4)
    res = []
    for i in (range(len(c['frames'])) if frames is None else frames):
        rows = unique_rows(gather(c['clouds'][i], c['indices'][i], c['classes'][i], NUM_CLASSES, cols))
        colours, rng = row_colours(rows, table, c['style'].get('class_range'), c['style'].get('colors'))
        img, union = paint(make_base(c['frames'][i]), rows, colours, st['alpha'], st['size_scale'], st['max_radius'])
        res.append(dict(rows=rows, count=len(rows), range=rng, colours=colours, image=img, union=union))
    return res
