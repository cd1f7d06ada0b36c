"""Training batches assembled on the device from ragged frames (csrc/k_data.h, csrc/k_radarmap.h; C ABI `ach_data_letterbox_batch`, `ach_data_labels_batch`,
`ach_data_radar_maps`, `ach_data_radar_points`).

The live path of the reference's `YoloDataset.__getitem__` / `get_random_data` + `yolo_dataset_collate_all` (utils/dataloader.py:87-148, 153-233, 517-550) for B decoded
frames of different sizes at once, producing what `GraphedTrainStep` / `MultiTaskLoss.forward(outputs, boxes, counts, png, png_w, pc_labels)` and the network take:

    images  [B, 3, R, R] fp32 / bf16 / fp16   PIL BICUBIC resize to (nw, nh) pasted at (dx, dy) on a (128, 128, 128) canvas, ((v / 255) - mean) / std in float64
                                              rounded once to fp32 (a 768-entry table), then one RNE rounding to a 16-bit type; `torch.uint8`: the bytes, [B, R, R, 3]
    png, png_w [B, R, R] uint8 / int64        PIL NEAREST resize, pasted on zeros, min(v, num_classes_seg) / min(v, 2); a frame without a water-line map: zeros
    boxes [B, G, 5] fp32, counts [B] int32    the reference's integer box arithmetic in numpy on the host (a handful of numbers), packed as `losses.pack_labels` packs
    points [B, D, N], pc_labels [B, N] int64  N rows sampled with replacement on the host, then the existing `prepost.normalize_points`
    radar   [B, C, R, R] fp32                 passes through; or, for frames that carry a raw `cloud` [n, F], rasterised on the device by the rule of the reference's
                                              radar_feature_map_generate.ipynb (`radar_maps_batch`), with `points` / `pc_labels` gathered from the same upload
                                              (`radar_points_batch`): one launch each

Per batch: two image launches, one label launch, one point launch, whatever B is; three host-to-device copies (image arena, label arena, one buffer with the frame
tables, the coefficient / index tables, the value table, boxes, points and radar maps) from reusable pinned memory, none back.  Placement defaults to the
reference's letterbox; a caller may pass any `(nw, nh, dx, dy)` per frame (scale / position jitter): the paste clips as `Image.paste` does.  Not covered: flips, the
HSV jitter / mosaic / mixup of the reference's unreachable code, image decoding, the float one-hot targets (the losses take integer maps).
No torch-op or CPU fallback: without the HIP library these raise.
"""
import collections
import ctypes

import numpy as np
import torch

from . import prepost as _pp
from .losses import pack_labels
from ._native import lib as _lib, check as _check, ptr as _p, stream as _stream, stateless_handle

TABLE_COLS = 16          # DATA_TABLE_COLS of k_data.h
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_OUT_KIND = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.uint8: 3}
_LABEL_KIND = {torch.int64: 0, torch.uint8: 2}
_ERRORS = {-1: ValueError, -2: NotImplementedError}

Batch = collections.namedtuple('Batch', 'images radar points boxes counts png png_w pc_labels')
Arena = collections.namedtuple('Arena', 'data frames')          # data: 1-D uint8 tensor on the device; frames: per frame (byte offset, H, W, pitch) or None
Clouds = collections.namedtuple('Clouds', 'data frames')        # data: 1-D float32 / float64 tensor on the device; frames: per frame (element offset, n, F, row stride)
RADAR_TABLE_COLS = 16    # k_radarmap.h
MAP_COLUMNS = (0, 1, 2, 3, 4)          # the notebook's feature order: range, doppler, rcs, u, v
CELL = (6.0, 3.375)                    # 1920 / 320 and 1080 / 320 pixels per cell: the notebook's constants, whatever the resolution
_IN_KIND = {torch.float32: 0, torch.float64: 1}


# ------------------------------------------------------------------------------------------------------------------ host rules
def value_table():
    """[3, 256] fp32: ((v / 255) - mean) / std in float64, rounded once (utils/dataloader.py:105 with utils_seg/utils.py:40-44, then FloatTensor)"""
    v = np.arange(256, dtype=np.float64)
    return np.stack([(v / 255.0 - m) / s for m, s in zip(MEAN, STD)]).astype(np.float32)


_NEAREST, _BICUBIC = {}, {}


def nearest_index(in_size, out_size):
    """Source index of every output sample of PIL's Image.NEAREST resize along one axis: Pillow's running sum in double (a = in / out; xx = a / 2; index =
    int(xx); xx += a), which `floor((x + 0.5) * in / out)` does not reproduce.  -1: past the axis (left zero).  int32 [out_size], cached."""
    key = (int(in_size), int(out_size))
    if key not in _NEAREST:
        a = key[0] / key[1]
        xx = 0.5 * a
        idx = np.empty(key[1], np.int32)
        for x in range(key[1]):
            i = int(xx)
            idx[x] = i if i < key[0] else -1
            xx += a
        _NEAREST[key] = idx
    return _NEAREST[key]


def _bicubic_tables(in_size, out_size):
    key = (int(in_size), int(out_size))
    if key not in _BICUBIC:
        b, k, ks = _pp._pil_coeffs(key[0], key[1], 'cpu')
        assert int(k.abs().max()) < 1 << 23                  # the kernels multiply taps as 24-bit integers (k_data.h tap_mul)
        _BICUBIC[key] = (b.numpy().reshape(-1), k.numpy().reshape(-1), int(ks))
    return _BICUBIC[key]


def default_placement(iw, ih, resolution):
    """the reference's letterbox (utils/dataloader.py:178-182): (nw, nh, dx, dy)"""
    R = int(resolution)
    scale = min(R / iw, R / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return nw, nh, (R - nw) // 2, (R - nh) // 2


def adjust_boxes(boxes, iw, ih, placement, resolution):
    """utils/dataloader.py:219-228 and :108-110 for one frame: integer corners (x1, y1, x2, y2, class) of the original image -> float64 [n, 5] (cx, cy, w, h, class)
    on the canvas.  The scaled corners are truncated toward zero when they are stored back into the integer array; input order is kept."""
    box = np.array(boxes, dtype=np.int64).reshape(-1, 5)
    nw, nh, dx, dy = (int(v) for v in placement)
    R = int(resolution)
    if len(box):
        box[:, [0, 2]] = box[:, [0, 2]] * nw / iw + dx
        box[:, [1, 3]] = box[:, [1, 3]] * nh / ih + dy
        box[:, 0:2] = np.maximum(box[:, 0:2], 0)
        box[:, 2:4] = np.minimum(box[:, 2:4], R)
        box = box[(box[:, 2] - box[:, 0] > 1) & (box[:, 3] - box[:, 1] > 1)]
    out = box.astype(np.float64)
    if len(out):
        out[:, 2:4] -= out[:, 0:2]
        out[:, 0:2] += out[:, 2:4] / 2
    return out


def sample_points(clouds, labels, num_points, indices=None, rng=None):
    """utils/dataloader.py:137-140: `num_points` rows with replacement from each ragged cloud [n_i, D] -> (fp32 [B, N, D], int64 [B, N], the indices [B, N])."""
    N = int(num_points)
    if indices is None and rng is None:
        raise ValueError("sample_points: pass `indices` [B, N] or a numpy.random.Generator as `rng`")
    pts, lab, used = [], [], []
    for b, cloud in enumerate(clouds):
        c = np.asarray(cloud)
        if c.ndim != 2 or c.shape[0] == 0:
            raise ValueError(f"sample_points: frame {b} has an empty point cloud")
        idx = np.asarray(indices[b], dtype=np.int64) if indices is not None else rng.choice(c.shape[0], N, replace=True)
        if idx.shape != (N,) or idx.min() < 0 or idx.max() >= c.shape[0]:
            raise ValueError(f"sample_points: frame {b} needs {N} indices below {c.shape[0]}")
        pts.append(c[idx].astype(np.float32))
        lab.append(np.asarray(labels[b])[idx].astype(np.int64))
        used.append(idx)
    return np.stack(pts), np.stack(lab), np.stack(used)


# ------------------------------------------------------------------------------------------------------------------ staging
def _host_array(a, channels):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    want = 3 if channels == 3 else 2
    if a.dtype != np.uint8 or a.ndim != want or (channels == 3 and a.shape[2] != 3) or a.size == 0:
        raise TypeError("frames are CPU uint8 arrays / tensors: images [H, W, 3], label maps [H, W]")
    return a


class _Pinned:
    """Reusable pinned staging memory per device.  A buffer is written again only after the copy that read it has completed (an event QUERY, never a wait); while
    it is in flight another buffer is taken, so nothing here synchronises."""

    def __init__(self, device):
        self.device, self.slots = device, {}

    def take(self, name, nbytes):
        if self.device.type != 'cuda':
            return [torch.empty(max(nbytes, 16), dtype=torch.uint8), None]
        ring = self.slots.setdefault(name, [])
        for slot in ring:
            if slot[0].numel() >= nbytes and (slot[1] is None or slot[1].query()):
                return slot
        ring[:] = [s for s in ring if s[0].numel() >= nbytes][-3:]
        slot = [torch.empty(max(16, nbytes + nbytes // 8), dtype=torch.uint8, pin_memory=True), None]
        ring.append(slot)
        return slot

    def upload(self, slot, nbytes):
        if self.device.type != 'cuda':
            return slot[0][:nbytes]
        dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        dev.copy_(slot[0][:nbytes], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        return dev


_PINNED = {}


def _pinned(device):
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if device not in _PINNED:
        _PINNED[device] = _Pinned(device)
    return _PINNED[device]


def pack_arena(frames, channels=3, device='cuda', name=None):
    """A list of CPU uint8 arrays / tensors (None: the frame has no such map) -> `Arena`: packed into reusable pinned memory, 16-byte aligned frames, ONE copy."""
    pin = _pinned(device)
    arrs = [None if f is None else _host_array(f, channels) for f in frames]
    offs, total = [], 0
    for a in arrs:
        offs.append(total)
        if a is not None:
            total += (a.size + 15) // 16 * 16
    total = max(total, 16)
    slot = pin.take(name or f'arena{channels}', total)
    host = slot[0].numpy()
    for a, o in zip(arrs, offs):
        if a is not None:
            np.copyto(host[o:o + a.size].reshape(a.shape), a)
    data = pin.upload(slot, total)
    return Arena(data, [None if a is None else (o, a.shape[0], a.shape[1], a.shape[1] * channels) for a, o in zip(arrs, offs)])


class _Meta:
    """Everything small a batch needs on the device, in ONE pinned buffer and one non-blocking copy: frame tables, coefficient / index tables (each distinct
    (in, out) pair once), the value table, boxes, points, radar maps."""

    def __init__(self, device, name='meta'):
        self.pin, self.parts, self.nbytes, self.name = _pinned(device), [], 0, name          # a `_Meta` kept across batches needs a `name` of its own
        self.tabs, self.tab_at, self.tab_len = [], {}, 0
        self.slot = self.dev = None

    def add(self, arr):
        arr = np.ascontiguousarray(arr)
        off = self.nbytes
        self.parts.append((off, arr))
        self.nbytes += (arr.nbytes + 15) // 16 * 16
        return (off, arr.dtype, arr.shape)

    def table(self, key, arr):
        if key not in self.tab_at:
            self.tab_at[key] = self.tab_len
            self.tabs.append(np.ascontiguousarray(arr, dtype=np.int32).reshape(-1))
            self.tab_len += self.tabs[-1].size
        return self.tab_at[key]

    def commit(self):
        self.tabs_ref = self.add(np.concatenate(self.tabs) if self.tabs else np.zeros(1, np.int32))
        self.slot = self.pin.take(self.name, self.nbytes)
        host = self.slot[0].numpy()
        for off, arr in self.parts:
            host[off:off + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        self.dev = self.pin.upload(self.slot, self.nbytes)

    def host_ptr(self, ref):
        return ctypes.c_void_p(self.slot[0].data_ptr() + ref[0])

    def dev_ptr(self, ref):
        return ctypes.c_void_p(self.dev.data_ptr() + ref[0])

    def tensor(self, ref):
        off, dtype, shape = ref
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.dev[off:off + n].view(getattr(torch, np.dtype(dtype).name)).view(shape)


def _as_arena(frames, channels, device, name):
    return frames if isinstance(frames, Arena) else pack_arena(frames, channels, device, name)


def _placements(frames, placements, R):
    if placements is None:
        return [default_placement(f[2], f[1], R) for f in frames]
    out = [tuple(int(v) for v in p) for p in placements]
    if len(out) != len(frames) or any(len(p) != 4 or p[0] < 1 or p[1] < 1 for p in out):
        raise ValueError("placements: one (nw, nh, dx, dy) per frame with nw, nh >= 1")
    return out


# ------------------------------------------------------------------------------------------------------------------ the two launches
def _plan_images(meta, arena, places, R):
    R4 = (R + 3) // 4 * 4
    table = np.zeros((len(arena.frames), TABLE_COLS), np.int64)
    mid = 0
    for b, (fr, (nw, nh, dx, dy)) in enumerate(zip(arena.frames, places)):
        off, H, W, pitch = fr
        hb, hk, hks = _bicubic_tables(W, nw)
        vb, vk, vks = _bicubic_tables(H, nh)
        table[b] = (off, H, W, pitch, nw, nh, dx, dy, meta.table(('hb', W, nw), hb), meta.table(('hk', W, nw), hk), hks,
                    meta.table(('hb', H, nh), vb), meta.table(('hk', H, nh), vk), vks, mid, 0)
        y0, y1 = min(max(dy, 0), R), min(max(dy + nh, 0), R)
        if y0 < y1 and min(max(dx, 0), R) < min(max(dx + nw, 0), R):
            rows = int(vb[2 * (y1 - 1 - dy)] + vb[2 * (y1 - 1 - dy) + 1] - vb[2 * (y0 - dy)])
            mid += rows * 3 * R4
    return meta.add(table), max(mid, 16)


def _launch_images(meta, arena, ref, mid_bytes, lut_ref, R, dtype):
    data = arena.data
    lib = _lib(data)
    B = len(arena.frames)
    mid = torch.empty(mid_bytes, dtype=torch.uint8, device=data.device)
    out = torch.empty((B, R, R, 3) if dtype == torch.uint8 else (B, 3, R, R), dtype=dtype, device=data.device)
    _check(lib, lib.lib.ach_data_letterbox_batch(_p(data), data.numel(), meta.host_ptr(ref), meta.dev_ptr(ref), meta.host_ptr(meta.tabs_ref), meta.dev_ptr(meta.tabs_ref),
                                                 meta.tab_len, meta.dev_ptr(lut_ref), B, R, _p(mid), mid_bytes, _p(out), _OUT_KIND[dtype], _stream(data)), _ERRORS, 'data kernel')
    return out


def _plan_labels(meta, arena, arena_w, places, R):
    """both maps of a frame live in ONE arena: `arena.frames` then `arena_w.frames` index the same `data`"""
    B = len(arena.frames)
    table = np.zeros((B, TABLE_COLS), np.int64)
    for b, (nw, nh, dx, dy) in enumerate(places):
        table[b, :4] = (nw, nh, dx, dy)
        for m, fr in enumerate((arena.frames[b], arena_w.frames[b])):
            if fr is None:
                table[b, 4 + 6 * m] = -1
                continue
            off, H, W, pitch = fr
            table[b, 4 + 6 * m:10 + 6 * m] = (off, H, W, pitch, meta.table(('nn', W, nw), nearest_index(W, nw)), meta.table(('nn', H, nh), nearest_index(H, nh)))
    return meta.add(table)


def _launch_labels(meta, data, ref, B, R, num_classes_seg, label_dtype):
    lib = _lib(data)
    png = torch.empty(B, R, R, dtype=label_dtype, device=data.device)
    png_w = torch.empty(B, R, R, dtype=label_dtype, device=data.device)
    _check(lib, lib.lib.ach_data_labels_batch(_p(data), data.numel(), meta.host_ptr(ref), meta.dev_ptr(ref), meta.host_ptr(meta.tabs_ref), meta.dev_ptr(meta.tabs_ref),
                                              meta.tab_len, B, R, int(num_classes_seg), _p(png), _p(png_w), _LABEL_KIND[label_dtype], _stream(data)), _ERRORS, 'data kernel')
    return png, png_w


def _pack_label_arena(png, png_w, device):
    n = len(png)
    both = pack_arena(list(png) + list(png_w), 1, device, 'labels')
    if any(f is None for f in both.frames[:n]):
        raise ValueError("every frame needs a semantic label map (only the water-line map may be missing)")
    return Arena(both.data, both.frames[:n]), Arena(both.data, both.frames[n:])


def _image_dtype(dtype):
    if dtype not in _OUT_KIND:
        raise TypeError(f"images are float32, bfloat16, float16 or uint8 (the bytes, HWC), got {dtype}")
    return dtype


def letterbox_batch(images, resolution, placements=None, dtype=torch.float32, device='cuda'):
    """`images`: a list of CPU uint8 [H, W, 3] arrays / tensors of any sizes, or an `Arena` already on the device -> [B, 3, R, R] `dtype` (torch.uint8: [B, R, R, 3],
    byte for byte `prepost.resize_image`).  Two launches for the whole batch."""
    R = int(resolution)
    arena = _as_arena(images, 3, device, 'images')
    places = _placements(arena.frames, placements, R)
    meta = _Meta(arena.data.device)
    ref, mid_bytes = _plan_images(meta, arena, places, R)
    lut = meta.add(value_table())
    meta.commit()
    return _launch_images(meta, arena, ref, mid_bytes, lut, R, _image_dtype(dtype))


def labels_batch(png, png_w, resolution, num_classes_seg, placements=None, label_dtype=torch.uint8, device='cuda'):
    """`png`, `png_w`: lists of CPU uint8 [H, W] label maps (`png_w[b]` may be None), or two `Arena`s over one device buffer -> (png, png_w) [B, R, R] `label_dtype`
    (uint8 or int64).  One launch.  Default placement: the reference's letterbox of the semantic map's size."""
    if label_dtype not in _LABEL_KIND:
        raise TypeError(f"label maps are uint8 or int64, got {label_dtype}")
    R = int(resolution)
    a, aw = (png, png_w) if isinstance(png, Arena) else _pack_label_arena(png, png_w, device)
    places = _placements(a.frames, placements, R)
    meta = _Meta(a.data.device)
    ref = _plan_labels(meta, a, aw, places, R)
    meta.commit()
    return _launch_labels(meta, a.data, ref, len(a.frames), R, num_classes_seg, label_dtype)


# ------------------------------------------------------------------------------------------------------------------ radar clouds (csrc/k_radarmap.h)
def pack_clouds(clouds, device='cuda', name='clouds'):
    """B host arrays [n_i, F_i] (all float32 or all float64; n_i may be 0) -> `Clouds`: packed into reusable pinned memory, 16-byte aligned frames, ONE copy."""
    arrs = []
    for b, c in enumerate(clouds):
        a = c.numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
        if a.ndim != 2 or a.shape[1] < 1 or a.dtype not in (np.float32, np.float64):
            raise TypeError(f"pack_clouds: frame {b}: clouds are CPU float32 / float64 arrays [n, F]")
        arrs.append(a)
    if not arrs or any(a.dtype != arrs[0].dtype for a in arrs):
        raise TypeError("pack_clouds: at least one cloud, all of one dtype")
    item = arrs[0].dtype.itemsize
    step = 16 // item
    offs, total = [], 0
    for a in arrs:
        offs.append(total)
        total += (a.size + step - 1) // step * step
    total = max(total, step)
    pin = _pinned(device)
    slot = pin.take(name, total * item)
    host = slot[0].numpy()[:total * item].view(arrs[0].dtype)
    for a, o in zip(arrs, offs):
        np.copyto(host[o:o + a.size].reshape(a.shape), a)
    data = pin.upload(slot, total * item).view(torch.float32 if item == 4 else torch.float64)
    return Clouds(data, [(o, a.shape[0], a.shape[1], a.shape[1]) for a, o in zip(arrs, offs)])


def _as_clouds(clouds, device, name='clouds'):
    return clouds if isinstance(clouds, Clouds) else pack_clouds(clouds, device, name)


def _plan_clouds(meta, packed, columns):
    cols = tuple(int(c) for c in columns)
    if len(cols) != 5:
        raise ValueError("columns: the five column indices of range, doppler, rcs, u, v")
    table = np.zeros((len(packed.frames), RADAR_TABLE_COLS), np.int64)
    for b, fr in enumerate(packed.frames):
        table[b, :4] = fr
        table[b, 4:9] = cols
    return meta.add(table)


def _launch_radar_maps(meta, packed, ref, R, cell, normalize, dtype):
    data = packed.data
    lib = _lib(data)
    B = len(packed.frames)
    raw = torch.empty(B, 3, R, R, dtype=torch.float32, device=data.device)
    out = partial = None
    if normalize:
        if dtype not in _OUT_KIND or dtype == torch.uint8:
            raise TypeError(f"the normalised radar map is float32, bfloat16 or float16, got {dtype}")
        out = torch.empty(B, 3, R, R, dtype=dtype, device=data.device)
        partial = torch.empty(2 * B * R, dtype=torch.float32, device=data.device)          # per frame one (min, max) per band of rows: at most R bands
    _check(lib, lib.lib.ach_data_radar_maps(_p(data), data.numel(), _IN_KIND[data.dtype], meta.host_ptr(ref), meta.dev_ptr(ref), B, R, float(cell[0]), float(cell[1]),
                                            _p(raw), _p(partial), partial.numel() if normalize else 0, _p(out), _OUT_KIND[dtype] if normalize else 0, _stream(data)),
           _ERRORS, 'radar kernel')
    return out if normalize else raw


def radar_maps_batch(clouds, resolution, columns=MAP_COLUMNS, cell=CELL, normalize=False, dtype=torch.float32, device='cuda'):
    """`clouds`: a list of CPU float32 / float64 arrays [n_i, F] (any n_i, 0 included), or `Clouds` already on the device -> the radar map [B, 3, R, R] the reference
    generates offline (radar_feature_map_generate.ipynb), EXACTLY: per channel (range, doppler, rcs = `columns[:3]`) and point in row order, x = int(u / cell[0]),
    y = int(v / cell[1]) in float64 with Python's truncation and negative-index wrap, the notebook's one-cell shift of a point that meets an occupied cell, later
    points overwriting earlier ones, the value rounded once to fp32.  normalize=False: that raw map, fp32 (what the reference trains on), one launch.
    normalize=True: `prepost.preprocess_input_radar(raw, dtype)` of it, the same bits, with the extrema taken in the rasterising pass: two launches."""
    R = int(resolution)
    packed = _as_clouds(clouds, device)
    meta = _Meta(packed.data.device, 'radar')
    ref = _plan_clouds(meta, packed, columns)
    meta.commit()
    return _launch_radar_maps(meta, packed, ref, R, cell, bool(normalize), dtype)


def draw_indices(counts, num_points, indices=None, rng=None):
    """utils/dataloader.py:137: `num_points` row indices with replacement per cloud of `counts[b]` rows, the caller's or drawn from `rng` -> int64 [B, N]"""
    N = int(num_points)
    if indices is None and rng is None:
        raise ValueError("pass `indices` [B, N] or a numpy.random.Generator as `rng`")
    out = np.empty((len(counts), N), np.int64)
    for b, n in enumerate(counts):
        if n < 1:
            raise ValueError(f"frame {b} has an empty point cloud")
        idx = np.asarray(indices[b], dtype=np.int64) if indices is not None else rng.choice(n, N, replace=True)
        if idx.shape != (N,) or idx.min() < 0 or idx.max() >= n:
            raise ValueError(f"frame {b} needs {N} indices below {n}")
        out[b] = idx
    return out


def _launch_radar_points(meta, packed, ref, iref, columns, label_column, N, dtype):
    data = packed.data
    lib = _lib(data)
    B = len(packed.frames)
    cols = np.ascontiguousarray([int(c) for c in columns], dtype=np.int32)
    if dtype not in _OUT_KIND or dtype == torch.uint8:
        raise TypeError(f"points are float32, bfloat16 or float16, got {dtype}")
    points = torch.empty(B, cols.size, N, dtype=dtype, device=data.device)
    labels = torch.empty(B, N, dtype=torch.int64, device=data.device) if label_column is not None else None
    _check(lib, lib.lib.ach_data_radar_points(_p(data), data.numel(), _IN_KIND[data.dtype], meta.host_ptr(ref), meta.dev_ptr(ref), meta.host_ptr(iref), meta.dev_ptr(iref),
                                              ctypes.c_void_p(cols.ctypes.data), cols.size, -1 if label_column is None else int(label_column), B, N, _p(points),
                                              _OUT_KIND[dtype], _p(labels), _stream(data)), _ERRORS, 'radar kernel')
    return points, labels


def radar_points_batch(clouds, columns, label_column=None, num_points=512, indices=None, rng=None, dtype=torch.float32, device='cuda'):
    """The PointNet input from the same clouds (utils/dataloader.py:137-141): `num_points` rows per frame by `indices` [B, N] (or drawn with replacement from `rng`),
    the D columns `columns`, each divided by its L2 norm over the sampled rows (sklearn normalize(axis=0); fp32 arithmetic on the fp32-rounded values, as
    `prepost.normalize_points`) -> (points [B, D, N] `dtype`, labels [B, N] int64 from `label_column`, or None).  One launch; the indices travel with the table."""
    packed = _as_clouds(clouds, device)
    idx = draw_indices([f[1] for f in packed.frames], num_points, indices, rng)
    meta = _Meta(packed.data.device, 'radar')
    ref = _plan_clouds(meta, packed, (0,) * 5)
    iref = meta.add(idx)
    meta.commit()
    return _launch_radar_points(meta, packed, ref, iref, columns, label_column, int(num_points), dtype)


def _normalize_points(points, dtype):
    lib = getattr(_lib, 'test_library', None)
    if lib is None:
        return _pp.normalize_points(points, dtype)
    B, N, D = points.shape                               # tests: the same kernel under the emulation library
    out = torch.empty(B, D, N, dtype=dtype, device=points.device)
    stateless_handle(1, 32, dtype, lib).normalize_points(B, N, D, points.contiguous(), out)
    return out


class TrainBatcher:
    """`TrainBatcher(resolution, num_classes_seg, num_points)(frames)` -> `Batch(images, radar, points, boxes, counts, png, png_w, pc_labels)` on `device`.

    `frames`: a list of dicts with `image` [H, W, 3] uint8, `png` [H, W] uint8, optionally `png_w` [H, W] uint8 (absent / None: zeros), `boxes` [n, 5] integers
    (x1, y1, x2, y2, class) in pixels of the original image, `radar` [C, R, R], and `points` [n, D] with `point_labels` [n] (all frames or none).  `placements`: one
    (nw, nh, dx, dy) per frame instead of the reference's letterbox.  Points are sampled with the caller's `indices` [B, N] or drawn from `rng`
    (a numpy.random.Generator).  `max_boxes` fixes G (a captured graph needs fixed shapes); more surviving boxes than that is `pack_labels`' error.

    Frames with a `cloud` key (all frames or none) carry the raw radar points instead of `radar` / `points` / `point_labels`: `cloud` [n, F] float32 / float64 and
    `cloud_columns`, a dict with 'map' (the columns of range, doppler, rcs, u, v; default 0..4) and optionally 'points' (the PointNet columns) with 'label' (the label
    column), the same for every frame.  `radar` is then the raw map of `radar_maps_batch` (cell size `cell`), `points` / `pc_labels` come from `radar_points_batch`:
    one upload of the clouds, one launch each."""

    def __init__(self, resolution, num_classes_seg, num_points=512, dtype=torch.float32, label_dtype=torch.uint8, max_boxes=None, device='cuda', cell=CELL):
        if label_dtype not in _LABEL_KIND:
            raise TypeError(f"label maps are uint8 or int64, got {label_dtype}")
        self.R, self.num_classes_seg, self.num_points = int(resolution), int(num_classes_seg), int(num_points)
        self.dtype, self.label_dtype, self.max_boxes, self.device = _image_dtype(dtype), label_dtype, max_boxes, device
        self.point_dtype = torch.float32 if dtype == torch.uint8 else dtype
        self.cell = (float(cell[0]), float(cell[1]))

    def __call__(self, frames, placements=None, indices=None, rng=None):
        R, B = self.R, len(frames)
        if B == 0:
            raise ValueError("TrainBatcher: an empty batch")
        arena = pack_arena([f['image'] for f in frames], 3, self.device, 'images')
        la, law = _pack_label_arena([f['png'] for f in frames], [f.get('png_w') for f in frames], self.device)
        places = _placements(arena.frames, placements, R)
        meta = _Meta(arena.data.device)
        iref, mid_bytes = _plan_images(meta, arena, places, R)
        lref = _plan_labels(meta, la, law, places, R)
        lut = meta.add(value_table())
        per = [torch.from_numpy(adjust_boxes(f.get('boxes', ()), fr[2], fr[1], p, R)) for f, fr, p in zip(frames, arena.frames, places)]
        boxes, counts = pack_labels(per, self.max_boxes, device='cpu')
        bref, cref = meta.add(boxes.numpy()), meta.add(counts.numpy())
        pref = plref = rref = None
        if any(f.get('cloud') is not None for f in frames):
            return self._cloud_batch(frames, indices, rng, meta, arena, la, iref, mid_bytes, lref, lut, bref, cref)
        if any(f.get('points') is not None for f in frames):
            pts, plab, _ = sample_points([f.get('points', ()) for f in frames], [f.get('point_labels') for f in frames], self.num_points, indices, rng)
            pref, plref = meta.add(pts), meta.add(plab)
        if any(f.get('radar') is not None for f in frames):
            rref = meta.add(np.stack([np.asarray(f['radar']) for f in frames]).astype(np.float32))
        meta.commit()
        images = _launch_images(meta, arena, iref, mid_bytes, lut, R, self.dtype)
        png, png_w = _launch_labels(meta, la.data, lref, B, R, self.num_classes_seg, self.label_dtype)
        points = _normalize_points(meta.tensor(pref), self.point_dtype) if pref is not None else None
        return Batch(images, meta.tensor(rref) if rref is not None else None, points, meta.tensor(bref), meta.tensor(cref), png, png_w,
                     meta.tensor(plref) if plref is not None else None)

    def _cloud_batch(self, frames, indices, rng, meta, arena, la, iref, mid_bytes, lref, lut, bref, cref):
        R, B = self.R, len(frames)
        if any(f.get('cloud') is None for f in frames) or any(f.get(k) is not None for f in frames for k in ('radar', 'points', 'point_labels')):
            raise ValueError("TrainBatcher: every frame carries a `cloud`, or none does; a `cloud` replaces `radar`, `points` and `point_labels`")
        cols = [dict(f.get('cloud_columns') or {}) for f in frames]
        if any(c != cols[0] for c in cols) or set(cols[0]) - {'map', 'points', 'label'} or ('label' in cols[0] and 'points' not in cols[0]):
            raise ValueError("TrainBatcher: `cloud_columns` is one dict for all frames with 'map', optionally 'points' and with it 'label'")
        packed = pack_clouds([f['cloud'] for f in frames], self.device)
        cref_ = _plan_clouds(meta, packed, cols[0].get('map', MAP_COLUMNS))
        xref = None
        if 'points' in cols[0]:
            xref = meta.add(draw_indices([f[1] for f in packed.frames], self.num_points, indices, rng))
        meta.commit()
        images = _launch_images(meta, arena, iref, mid_bytes, lut, R, self.dtype)
        png, png_w = _launch_labels(meta, la.data, lref, B, R, self.num_classes_seg, self.label_dtype)
        radar = _launch_radar_maps(meta, packed, cref_, R, self.cell, False, torch.float32)
        points = pc_labels = None
        if xref is not None:
            points, pc_labels = _launch_radar_points(meta, packed, cref_, xref, cols[0]['points'], cols[0].get('label'), self.num_points, self.point_dtype)
        return Batch(images, radar, points, meta.tensor(bref), meta.tensor(cref), png, png_w, pc_labels)
