"""The cases of tests/test_heatmap.py and the heat-map mode restated in numpy (achelous_amd/csrc/k_heatmap.h; the reference's achelous.detect_heatmap, achelous.py:451-555).

Inputs.  One batch of six frames — (1, 1), (3, 2) with W < 4, (7, 9) a down-scale below the 10 x 10 level, (37, 53) with W % 4 != 0, (96, 131) more than one column
tile, (1, 300) — on detection maps at R = 320 with num_det 1 ('nd1') and 7 ('nd7'), and one frame at R = 416 ('r416': A = 3549 cells, next to the LDS bound of 4096).
The logits are smooth seeded fields quantised to eighths inside (-16, 16), so one set of values is exact in fp32, bf16 and fp16; the box channels 0..3 are not read and
hold zeros.  tests/golden/gen_heatmap_golden.py records what the reference's own statements give on them in tests/golden/heatmap.npz, together with the logits (as
int8 eighths), so `make_case` here is only run by the generator; the tests read the fixture.

Restatement.  `scores` (any float type), `mask_from_scores` (the resize with the window's scale and offset per axis; float32 as the kernel and cv2 compute it, or
float64 for the error analysis), `colour` (Normalize + 256-entry colour map + Image.blend)."""
import numpy as np

SHAPES = ((1, 1), (3, 2), (7, 9), (37, 53), (96, 131), (1, 300))
CASES = {'nd1': dict(R=320, num_det=1, frames=(0, 1, 2, 3, 4, 5), seed=12),           # (the objectness and the first class of 'nd7')
         'nd7': dict(R=320, num_det=7, frames=(0, 1, 2, 3, 4, 5), seed=12),
         'r416': dict(R=416, num_det=1, frames=(3,), seed=13)}
ALPHAS = (0.5, 0.3)
COLOUR_CASE = 'nd7'           # the case whose colour pictures the fixture stores
STRIDES = (8, 16, 32)


def cells(R):
    return [(R // s) ** 2 for s in STRIDES]


def letterbox_window(h, w, R):
    scale = min(R / w, R / h)
    nw, nh = max(1, int(w * scale)), max(1, int(h * scale))
    return (R - nh) // 2, (R - nw) // 2, nh, nw


def make_base(b):
    """the image under the colour for frame b: smooth, every byte value reachable, seeded"""
    H, W = SHAPES[b]
    rng = np.random.default_rng(100 + b)
    yy, xx = np.mgrid[0:H, 0:W]
    ph = rng.uniform(0, 6.28, 3)
    img = 127.5 + 127.5 * np.sin(xx[..., None] / 9.0 + yy[..., None] / 5.0 + ph)
    img[::3, ::5] = rng.integers(0, 256, img[::3, ::5].shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def make_case(name):
    """logits as int8 eighths [B, 1 + num_det, A]: channel 0 the objectness, then the classes; level-major cells"""
    c = CASES[name]
    if name == 'nd1':
        return np.ascontiguousarray(make_case('nd7')[:, :2])
    R, nd, B = c['R'], c['num_det'], len(c['frames'])
    rng = np.random.default_rng(c['seed'])
    out = np.zeros((B, 1 + nd, sum(cells(R))), np.int8)
    for b in range(B):
        floor = -9.0 if b % 3 else -1.0                                  # every third frame has a warm background: lo > 0
        blobs = [(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.03, 0.25), rng.uniform(4, 12)) for _ in range(4)]
        at = 0
        for s in STRIDES:
            n = R // s
            yy, xx = (np.mgrid[0:n, 0:n] + 0.5) / n
            for ch in range(1 + nd):
                v = np.full((n, n), floor + 0.4 * ch)
                for k, (cy, cx, sig, amp) in enumerate(blobs):
                    if ch == 0 or (k + ch) % 3 != 0:
                        v = v + amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig * sig)) * (1.0 - 0.07 * ch)
                v = v + 0.5 * np.sin(37.0 * xx * (1 + ch) + 11.0 * yy * yy * (b + 1))            # fine structure without the entropy of noise: the fixture stores these
                out[b, ch, at:at + n * n] = np.clip(np.round(v * 8), -127, 127).reshape(-1)
            at += n * n
    return out


def det_maps(eighths, R, dtype=np.float32):
    """the three det tensors [B, 5 + num_det, n, n] of a case's logits (box channels zero)"""
    B, C, _ = eighths.shape
    maps, at = [], 0
    for s in STRIDES:
        n = R // s
        m = np.zeros((B, 4 + C, n, n), dtype)
        m[:, 4:] = (eighths[:, :, at:at + n * n].astype(np.float64) / 8.0).reshape(B, C, n, n)
        maps.append(m)
        at += n * n
    return maps


def scores(dets, dtype=np.float32):
    """[B, A] level-major: max_c sigmoid(cls) * sigmoid(obj), the reference's expression (achelous.py:457-459, 543) in `dtype`; a cell with a NaN logit scores 0"""
    out = []
    with np.errstate(over='ignore', invalid='ignore'):
        for d in dets:
            x = np.asarray(d).astype(dtype)
            sig = lambda v: 1.0 / (1.0 + np.exp(-v))
            s = np.max(sig(x[:, 5:]), 1) * sig(x[:, 4])
            s = np.where(np.isnan(x[:, 4:]).any(1), 0, s).astype(dtype)
            out.append(s.reshape(len(x), -1))
    return np.concatenate(out, 1)


def _axis(n_dst, scale, off, n_src):
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale + off - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = (f - i.astype(np.float32)).astype(np.float32)
    lo, hi = i < 0, i >= n_src - 1
    i = np.where(lo, 0, np.where(hi, n_src - 1, i))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    return i, np.minimum(i + 1, n_src - 1), f


def resize_level(src, H, W, stride, window, dtype=np.float32):
    """the level's map [n, n] stretched to [H, W]: sc = nw / (W * stride), off = x0 / stride per axis, clamps to the whole map, horizontal then vertical blend in `dtype`
    (float32: every operation rounded on its own, as the kernel)"""
    y0, x0, nh, nw = window
    n = src.shape[0]
    src = src.astype(dtype)
    iy, iy1, fy = _axis(H, float(nh) / (float(H) * float(stride)), float(y0) / float(stride), n)
    ix, ix1, fx = _axis(W, float(nw) / (float(W) * float(stride)), float(x0) / float(stride), n)
    fxc, fyc, one = fx[None, :].astype(dtype), fy[:, None].astype(dtype), dtype(1)
    top = src[iy][:, ix] * (one - fxc) + src[iy][:, ix1] * fxc
    bot = src[iy1][:, ix] * (one - fxc) + src[iy1][:, ix1] * fxc
    return (top * (one - fyc) + bot * fyc).astype(dtype)


def level_values(score_row, R, H, W, window=None, dtype=np.float32):
    """[3, H, W]: resize_l * 255 of the three levels"""
    window = (0, 0, R, R) if window is None else window
    out, at = [], 0
    for s in STRIDES:
        n = R // s
        out.append(resize_level(np.asarray(score_row[at:at + n * n]).reshape(n, n), H, W, s, window, dtype) * dtype(255))
        at += n * n
    return np.stack(out)


def mask_from_scores(score_row, R, H, W, window=None):
    """uint8 [H, W]: max_l uint8(trunc(resize_l * 255)) from one frame's float32 scores [A]"""
    return level_values(np.asarray(score_row, np.float32), R, H, W, window).astype(np.uint8).max(0)


def colour_index(m, lo, hi):
    """the colour-map entry of mask value m: Normalize(lo, hi) in float64, times 256, truncated, 256 -> 255; a flat mask takes entry 0"""
    m = np.asarray(m, np.float64)
    if hi == lo:
        return np.zeros(m.shape, np.int64)
    return np.minimum(((m - float(lo)) / float(hi - lo) * 256.0).astype(np.int64), 255)


def colour(mask, lo, hi, base, cmap, alpha):
    """uint8 [H, W, 3]: Image.blend(base, cmap[colour_index(mask)], alpha) = (uint8)(a + alpha * (b - a)) in float32, every operation rounded"""
    rgb = np.asarray(cmap)[colour_index(mask, lo, hi)].astype(np.float32)
    a = base.astype(np.float32)
    return (a + (np.float32(alpha) * (rgb - a)).astype(np.float32)).astype(np.float32).astype(np.uint8)
