"""Device-side counterparts of the reference's host pre / post-processing, batched.

    preprocess_input_radar(radar[B,C,R,R] fp32)      utils/utils.py:51-54   -> [B,C,R,R] dtype
    normalize_points(points[B,N,D] fp32)             achelous.py:240-243    -> [B,D,N]   dtype
    preprocess_input(images[B,R,R,3] uint8)          utils/utils.py:44-48   -> [B,3,R,R] dtype   (letterboxing stays on the host)
    seg_class_map(seg[B,C,R,R])                      achelous.py:283-296    -> uint8 [B,R,R]     (network resolution)
    seg_class_map_original(seg[B,C,R,R], (h, w))     achelous.py:283-318    -> uint8 [B,h,w]     softmax -> crop bars -> INTER_LINEAR -> argmax
    seg_maps_frames(se, lane, shapes, arena)         achelous.py:283-345    -> per-frame views   both class maps + the overlay image, ragged batch, one launch
    correct_boxes_frames(rows, cnt, (R, R), shapes)  utils_bbox.py:5-30     -> [B,max_det,7]     every frame's own (H, W)
    detect_frames(net, frames, radar, points)        achelous.py:190-345    camera bytes of B frames of different sizes -> boxes, class maps, overlays
    detect_frames_from_clouds(net, frames, clouds)   + radar_feature_map_generate.ipynb   the same from raw radar point clouds (data.radar_maps_batch / radar_points_batch)
    draw_detections_frames(arena, layout, boxes, ..) achelous.py:363-433    box rings, label plates and label text drawn in place on every frame, PIL's bytes (csrc/k_draw.h)
    heatmap_frames(det, shapes, base, layout, style) achelous.py:451-555    the heat-map mode: score mask at every frame's size, its range, the jet blend (csrc/k_heatmap.h)
    scatter_points_frames(arena, layout, shapes, ..) achelous.py:261-271    the radar point classes: unique (u, v, rcs, class) rows and their discs painted in place (csrc/k_scatter.h)
HIP kernels through the C ABI; no CPU fallback.
"""
import contextlib
import math

import numpy as np
import torch

from ._native import lib as _pass_lib, check as _check, ptr as _ptr, stream as _stream, stateless_handle, DTYPE_CODE as _DTYPE_CODE
from .postprocess import _handle

# `_pass_lib(t)` is `_native.lib` (tests set `_pass_lib.test_library`): it raises RuntimeError for a CPU tensor.  The single-shape entries below always run on the
# HIP library through `_handle`; they call it for that check alone (with a test library set a CPU tensor gets as far as `torch.cuda.device`, which refuses it).


def preprocess_input_radar(radar, dtype=torch.float32):
    _pass_lib(radar)
    r = radar.contiguous().float()
    B, C, R, _ = r.shape
    with torch.cuda.device(r.device):
        out = torch.empty(B, C, R, R, dtype=dtype, device=r.device)
        _handle(1, R, dtype).preprocess_radar(B, C, r, out, torch.cuda.current_stream().cuda_stream)
    return out


def normalize_points(points, dtype=torch.float32):
    _pass_lib(points)
    p = points.contiguous().float()
    B, N, D = p.shape
    with torch.cuda.device(p.device):
        out = torch.empty(B, D, N, dtype=dtype, device=p.device)
        _handle(1, 320, dtype).normalize_points(B, N, D, p, out, torch.cuda.current_stream().cuda_stream)
    return out


def preprocess_input(images_u8, dtype=torch.float32):
    _pass_lib(images_u8)
    x = images_u8.contiguous()
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.shape[1] != x.shape[2]:
        raise ValueError("expected uint8 images [B,R,R,3]")
    B, R = x.shape[0], x.shape[1]
    with torch.cuda.device(x.device):
        out = torch.empty(B, 3, R, R, dtype=dtype, device=x.device)
        _handle(1, R, dtype).preprocess_image(B, x, out, torch.cuda.current_stream().cuda_stream)
    return out


def seg_class_map(seg):
    _pass_lib(seg)
    s = seg.contiguous()
    B, C, R, _ = s.shape
    with torch.cuda.device(s.device):
        out = torch.empty(B, R, R, dtype=torch.uint8, device=s.device)
        _handle(1, R, s.dtype).seg_argmax(B, C, s, out, torch.cuda.current_stream().cuda_stream)
    return out


def seg_class_map_original(seg, image_shape):
    """The class map at the ORIGINAL image size exactly as the reference's detect_image builds it (achelous.py:283-318): softmax over
    the classes, the letterbox's grey bars cropped (utils_seg/utils.py:19-31), cv2.resize(..., INTER_LINEAR) to `image_shape` = (h, w),
    argmax.  All frames of the batch share `image_shape`."""
    _pass_lib(seg)
    s = seg.contiguous()
    B, C, R, _ = s.shape
    oh, ow = int(image_shape[0]), int(image_shape[1])
    with torch.cuda.device(s.device):
        ws = torch.empty(B * C * R * R, dtype=torch.float32, device=s.device)
        out = torch.empty(B, oh, ow, dtype=torch.uint8, device=s.device)
        _handle(1, R, s.dtype).seg_resize_argmax(B, C, s, oh, ow, ws, out, torch.cuda.current_stream().cuda_stream)
    return out


# ------------------------------------------------------------------------------------------------- letterbox resize (utils/utils.py:20-33)
def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_COEFFS = {}


def _pil_coeffs(in_size, out_size, device):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) for Image.BICUBIC over the whole axis: per output
    sample the first source index, the tap count and the taps as 22-bit fixed point — double precision and C truncation on the host (a
    few hundred numbers), integer arithmetic on the device.  Cached per (sizes, device)."""
    key = (in_size, out_size, str(device))
    if key not in _COEFFS:
        scale = filterscale = in_size / out_size
        filterscale = max(filterscale, 1.0)
        support = 2.0 * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        bounds, kk = [], []
        for xx in range(out_size):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            count = min(int(center + support + 0.5), in_size) - xmin
            w = [_bicubic((x + xmin - center + 0.5) / filterscale) for x in range(count)]
            ww = sum(w)
            row = [0] * ksize
            for x in range(count):
                v = w[x] / ww if ww != 0.0 else w[x]
                row[x] = int(v * (1 << 22) - 0.5) if v < 0 else int(v * (1 << 22) + 0.5)
            bounds.append((xmin, count))
            kk.append(row)
        _COEFFS[key] = (torch.tensor(bounds, dtype=torch.int32, device=device), torch.tensor(kk, dtype=torch.int32, device=device), ksize)
    return _COEFFS[key]


def _resample(lib, src, out_h, out_w, dst=None):
    """PIL.Image.resize((out_w, out_h), BICUBIC) of an HWC uint8 tensor; `dst` (a window of a larger canvas) receives the last pass."""
    H, W, C = src.shape
    stream = _stream(src)

    def run(s, oh, ow, vertical, d):
        b, k, ks = _pil_coeffs(s.shape[0] if vertical else s.shape[1], oh if vertical else ow, s.device)
        _check(lib, lib.lib.ach_resample_pass_u8(s.data_ptr(), d.data_ptr(), b.data_ptr(), k.data_ptr(), ks, s.shape[0], s.shape[1], oh, ow, C, int(vertical),
                                                 s.stride(0), d.stride(0), stream), what='resample pass')
        return d

    cur = src
    if W != out_w:
        last = H == out_h
        cur = run(cur, H, out_w, False, dst if (last and dst is not None) else torch.empty(H, out_w, C, dtype=torch.uint8, device=src.device))
    if H != out_h:
        cur = run(cur, out_h, out_w, True, dst if dst is not None else torch.empty(out_h, out_w, C, dtype=torch.uint8, device=src.device))
    if dst is not None and cur is not dst:
        dst.copy_(cur)                                   # neither axis changed: the paste is a copy
        cur = dst
    return cur


def resize_image(image_u8, size, letterbox_image=True):
    """The reference's `resize_image(image, size, letterbox_image)` (utils/utils.py:20-33) on the device, BIT-EXACT against PIL: `image_u8`
    [H, W, 3] uint8 (HWC, what `np.array(PIL image)` gives), `size` = (w, h).  letterbox: aspect-preserving Image.BICUBIC resize pasted
    centred on a (128, 128, 128) canvas; otherwise a plain BICUBIC resize.  Returns [h, w, 3] uint8; feed it to `preprocess_input`."""
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise TypeError("resize_image expects an HWC uint8 image [H, W, 3]")
    img = image_u8.contiguous()
    lib = _pass_lib(img)
    ih, iw = img.shape[0], img.shape[1]
    w, h = int(size[0]), int(size[1])
    if not letterbox_image:
        return _resample(lib, img, h, w)
    scale = min(w / iw, h / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    canvas = torch.full((h, w, 3), 128, dtype=torch.uint8, device=img.device)
    y0, x0 = (h - nh) // 2, (w - nw) // 2
    _resample(lib, img, nh, nw, dst=canvas[y0:y0 + nh, x0:x0 + nw])
    return canvas


# ------------------------------------------------------------------------------------------------- camera bytes -> results, on the device
def detect_frame(net, image_u8, radar_map, points, conf_thres=0.5, nms_thres=0.4, letterbox_image=True, max_det=100, dtype=torch.bfloat16):
    """The arithmetic of the reference's `detect_image` (achelous.py:190-330) for one frame without its file I/O and plotting, every stage a
    device kernel: letterbox resize (PIL BICUBIC, bit-exact) -> mean / std + HWC -> CHW, radar min-max, point normalisation -> forward +
    decode + NMS (`forward_detect`) -> boxes back to the original image's pixels, both class maps at the original size (softmax -> crop ->
    INTER_LINEAR -> argmax), the per-point class.

    image_u8 [H, W, 3] uint8, radar_map [3, R, R] float, points [N, pc_channels] float (rows = points), all on the GPU.
    Returns dict(boxes [K, 7] = (y1, x1, y2, x2 in image pixels, obj, class conf, class id), semantic [H, W] uint8, waterline [H, W] uint8,
    point_class [N] int64)."""
    from .postprocess import correct_boxes_device
    R = net.resolution
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    dt = dtype
    x = preprocess_input(resize_image(image_u8, (R, R), letterbox_image).unsqueeze(0), dt)
    xr = preprocess_input_radar(radar_map.unsqueeze(0), dt)
    xp = normalize_points(points.unsqueeze(0), dt)
    (det, se, lane, pc), (rows, idx, cnt) = net.forward_detect(x, xr, xp, conf_thres, nms_thres, max_det)
    boxes = correct_boxes_device(rows, cnt, (R, R), (H, W), letterbox_image)
    sem, wl = seg_class_map_original(se, (H, W)), seg_class_map_original(lane, (H, W))
    return {'boxes': boxes[0, :int(cnt[0])], 'semantic': sem[0], 'waterline': wl[0], 'point_class': pc[0].float().argmax(-1)}


# ------------------------------------------------------------------------------------------------- a ragged batch: class maps, overlays, boxes (csrc/k_serve.h)
# the reference's two colour lists for up to 21 classes (achelous.py:135-142; the water-line list is the same list reversed)
PALETTE_SEG = ((0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (128, 0, 128), (0, 128, 128), (128, 128, 128), (64, 0, 0), (192, 0, 0), (64, 128, 0),
               (192, 128, 0), (64, 0, 128), (192, 0, 128), (64, 128, 128), (192, 128, 128), (0, 64, 0), (128, 64, 0), (0, 192, 0), (128, 192, 0), (0, 64, 128),
               (128, 64, 12))
PALETTE_LINE = tuple(reversed(PALETTE_SEG))
SERVE_TABLE_COLS = 16        # k_serve.h
_SERVE_OUTPUTS = ('semantic', 'waterline', 'overlay')


def _frames_handle(t, R, dtype):
    """the engine handle whose kernels serve tensors like `t` (tests: the emulation library through `_pass_lib.test_library`)"""
    _pass_lib(t)
    return stateless_handle(1, R, dtype, getattr(_pass_lib, 'test_library', None))


def _frame_shapes(shapes, B):
    out = [(int(s[0]), int(s[1])) for s in shapes]
    if len(out) != B:
        raise ValueError(f"shapes: one (H, W) per frame expected, got {len(out)} for a batch of {B}")
    if any(h < 1 or w < 1 for h, w in out):
        raise ValueError("shapes: H and W are at least 1")
    return out


def letterbox_window(h, w, R):
    """(y0, x0, nh, nw): the part of the R x R network map the letterbox of an (h, w) frame fills (utils_seg/utils.py:19-31, as `seg_class_map_original` crops it)"""
    scale = min(R / w, R / h)
    nw, nh = max(1, int(w * scale)), max(1, int(h * scale))
    return (R - nh) // 2, (R - nw) // 2, nh, nw


def brightness_table(factor):
    """ImageEnhance.Brightness(image).enhance(factor) per byte: Image.blend(black, image, factor) = factor * v in float32, <= 0 -> 0, >= 255 -> 255, else truncated"""
    t = np.float32(factor) * np.arange(256, dtype=np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def frames_layout(shapes):
    """Where `seg_maps_frames` puts every frame in its output arenas: (map offsets, map pitches, map bytes, overlay offsets, overlay pitches, overlay bytes).
    Pitches are rounded up to 16 bytes, so frame starts are 16-byte aligned."""
    moff, mp, ooff, op, mt, ot = [], [], [], [], 0, 0
    for h, w in shapes:
        mp.append((w + 15) // 16 * 16)
        op.append((3 * w + 15) // 16 * 16)
        moff.append(mt)
        ooff.append(ot)
        mt += h * mp[-1]
        ot += h * op[-1]
    return moff, mp, mt, ooff, op, ot


def _seg_maps_plan(se, lane, shapes, arena=None, palette_se=PALETTE_SEG, palette_line=PALETTE_LINE, keep_classes=None, blend=(0.45, 0.3), brightness=1.3,
                   want=_SERVE_OUTPUTS, windows=None, workspaces=None, out=None, meta_name='serve'):
    """everything `seg_maps_frames` does on the host (checks, frame table, constants, one upload, arenas); returns the launch as a callable.  A caller that keeps the
    callable and launches it again later passes a `meta_name` of its own: the pinned copy of the tables, which every launch re-checks, is reused per name"""
    from . import data as _data
    s, ln = se.contiguous(), lane.contiguous()
    B, C, R, _ = s.shape
    if ln.shape != (B, 2, R, R) or ln.dtype != s.dtype or s.shape[3] != R:
        raise ValueError("seg_maps_frames: se [B, C, R, R] and lane [B, 2, R, R] of one dtype expected")
    shapes = _frame_shapes(shapes, B)
    want = tuple(w for w in _SERVE_OUTPUTS if w in want and (w != 'overlay' or arena is not None))
    if not want or any(w not in _SERVE_OUTPUTS for w in want):
        raise ValueError(f"seg_maps_frames: `want` names some of {_SERVE_OUTPUTS} (the overlay needs `arena`)")
    wins = [letterbox_window(h, w, R) for h, w in shapes] if windows is None else [tuple(int(v) for v in w) for w in windows]
    if len(wins) != B:
        raise ValueError("seg_maps_frames: one window per frame")
    moff, mp, mbytes, ooff, op, obytes = frames_layout(shapes)
    table = np.zeros((B, SERVE_TABLE_COLS), np.int64)
    for b, ((h, w), win) in enumerate(zip(shapes, wins)):
        table[b, 1:3] = (h, w)
        table[b, 4:8] = win
        table[b, 8:13] = (moff[b], moff[b], mp[b], ooff[b], op[b])
    meta = _data._Meta(s.device, meta_name)
    consts = None
    n_se = n_line = 0
    if 'overlay' in want:
        if len(arena.frames) != B or any(f is None or (f[1], f[2]) != sh for f, sh in zip(arena.frames, shapes)):
            raise ValueError("seg_maps_frames: `arena` holds one image per frame, of the sizes in `shapes`")
        for b, f in enumerate(arena.frames):
            table[b, 0], table[b, 3] = f[0], f[3]
        pal = [np.asarray(p, dtype=np.uint8).reshape(-1, 3) for p in (palette_se, palette_line)]
        if any(len(p) < 1 or len(p) > 256 for p in pal):
            raise ValueError("seg_maps_frames: a palette holds 1..256 colours")
        n_se, n_line = len(pal[0]), len(pal[1])
        c = np.zeros(2304, np.uint8)
        c[0:3 * n_se], c[768:768 + 3 * n_line] = pal[0].reshape(-1), pal[1].reshape(-1)
        ident = np.arange(256, dtype=np.uint8)
        c[1536:1792] = ident if keep_classes is None else np.where(np.isin(ident, np.asarray(keep_classes, dtype=np.int64)), ident, 0)
        c[1792:2048] = ident
        if brightness is not None:
            c[2048:2304] = brightness_table(brightness)
        consts = meta.add(c)
    tref = meta.add(table)
    meta.commit()
    dev = s.device
    sizes = {'semantic': mbytes, 'waterline': mbytes, 'overlay': obytes}
    arenas = {}
    for name in want:
        a = (out or {}).get(name)
        if a is None:
            a = torch.empty(max(sizes[name], 16), dtype=torch.uint8, device=dev)
        elif a.dtype != torch.uint8 or a.dim() != 1 or not a.is_contiguous() or a.device != dev or a.numel() < sizes[name]:
            raise ValueError(f"seg_maps_frames: out[{name!r}] is a contiguous 1-D uint8 tensor of at least {sizes[name]} bytes on the inputs' device")
        arenas[name] = a
    if workspaces is None:
        workspaces = (torch.empty(B * C * R * R, dtype=torch.float32, device=dev), torch.empty(B * 2 * R * R, dtype=torch.float32, device=dev))
    ws_se, ws_line = workspaces
    if ws_se.dtype != torch.float32 or ws_line.dtype != torch.float32 or ws_se.numel() < B * C * R * R or ws_line.numel() < B * 2 * R * R or ws_se.device != dev or ws_line.device != dev:
        raise ValueError("seg_maps_frames: workspaces are fp32 tensors of B * C * R * R and B * 2 * R * R elements on the inputs' device")
    h = _frames_handle(s, R, s.dtype)
    addr = lambda ref: (meta.host_ptr(ref).value, meta.dev_ptr(ref).value) if ref is not None else (None, None)
    nbytes = lambda name: arenas[name].numel() if name in arenas else 0
    ctx = torch.cuda.device(dev) if s.is_cuda else contextlib.nullcontext()

    def run():
        with ctx:
            h.seg_overlay_frames(B, C, s, ln, ws_se, ws_line, arena.data if 'overlay' in want else None, arena.data.numel() if 'overlay' in want else 0,
                                 *addr(tref), *addr(consts), n_se, n_line, blend[0], blend[1], brightness is not None, arenas.get('semantic'), nbytes('semantic'),
                                 arenas.get('waterline'), nbytes('waterline'), arenas.get('overlay'), nbytes('overlay'), _stream(s).value)
        res = {'arenas': arenas}
        for name in want:
            a = arenas[name]
            if name == 'overlay':
                res[name] = [torch.as_strided(a, (hh, ww, 3), (op[b], 3, 1), ooff[b]) for b, (hh, ww) in enumerate(shapes)]
            else:
                res[name] = [torch.as_strided(a, (hh, ww), (mp[b], 1), moff[b]) for b, (hh, ww) in enumerate(shapes)]
        return res
    return run



def seg_maps_frames(se, lane, shapes, arena=None, palette_se=PALETTE_SEG, palette_line=PALETTE_LINE, keep_classes=None, blend=(0.45, 0.3), brightness=1.3,
                    want=_SERVE_OUTPUTS, windows=None, workspaces=None, out=None):
    """What the reference's detect_image computes from the two segmentation outputs (achelous.py:283-345), for B frames of DIFFERENT sizes in one launch behind
    the two softmax launches: `se` [B, C, R, R], `lane` [B, 2, R, R], `shapes` one (H, W) per frame.

    semantic / waterline: the class map at the frame's own size, exactly `seg_class_map_original` per frame (the arg-max itself; `keep_classes` does not touch it).
    overlay: [H, W, 3] uint8 = Brightness(blend(blend(image, palette_se[class'], blend[0]), palette_line[line class], blend[1])).enhance(brightness), PIL's
    arithmetic byte for byte; class' = class if class in `keep_classes` else 0 (achelous.py:297 is keep_classes=(0, 8); None keeps all); brightness None: no
    enhancement.  Needs `arena`, the `data.Arena` the frames were uploaded in (`data.pack_arena`); with arena=None only the class maps are produced.

    Returns a dict of lists of per-frame VIEWS into one packed arena per output (row pitch rounded up to 16 bytes: the views are strided, nothing is copied), and
    under 'arenas' the arenas themselves.  `windows`: per frame (y0, x0, nh, nw) of the network map instead of the letterbox's window.  `workspaces`: the two fp32
    probability buffers (B * C * R * R and B * 2 * R * R) to use; `out`: dict name -> 1-D uint8 tensor to use as that output's arena (`frames_layout`).
    No host read, no synchronisation."""
    return _seg_maps_plan(se, lane, shapes, arena, palette_se, palette_line, keep_classes, blend, brightness, want, windows, workspaces, out)()


def correct_boxes_frames(rows, cnt, input_shape, shapes, letterbox_image):
    """`postprocess.correct_boxes_device` for a ragged batch: kept rows [B, max_det, 7] -> (y1, x1, y2, x2) in pixels of EACH frame's own image, `shapes` one (H, W)
    per frame; rows past cnt[b] are zero.  One launch; the shapes travel in one non-blocking copy."""
    from . import data as _data
    R = int(input_shape[0])
    if int(input_shape[1]) != R:
        raise ValueError("square network input expected")
    rows = rows.contiguous()
    B, max_det, _ = rows.shape
    shapes = _frame_shapes(shapes, B)
    meta = _data._Meta(rows.device, 'serve_boxes')
    ref = meta.add(np.asarray(shapes, dtype=np.int32))
    meta.commit()
    out = torch.empty_like(rows)
    h = _frames_handle(rows, R, torch.float32)
    ctx = torch.cuda.device(rows.device) if rows.is_cuda else contextlib.nullcontext()
    with ctx:
        h.correct_boxes_frames(B, max_det, rows, cnt.contiguous(), meta.host_ptr(ref).value, meta.dev_ptr(ref).value, letterbox_image, out, _stream(rows).value)
    return out


# ------------------------------------------------------------------------------------------------- boxes, plates and labels on the frames (csrc/k_draw.h)
DRAW_TABLE_COLS, DRAW_LABEL_COLS, DRAW_REC, DRAW_SCORES = 8, 7, 16, 101        # k_draw.h
DRAW_STYLE_BYTES, DRAW_STYLE_SKIP, DRAW_STYLE_INK = 1028, 768, 1024
_DRAW_ERRORS = {-1: ValueError, -2: NotImplementedError}


def class_colors(n):
    """the reference's box colours (achelous.py:130-132): the HSV wheel in n steps, truncated to bytes; uint8 [n, 3]"""
    import colorsys
    return np.array([[int(v * 255) for v in colorsys.hsv_to_rgb(x / n, 1., 1.)] for x in range(n)], dtype=np.uint8).reshape(n, 3)


def _core_bytes(core):
    """the rows of an 'L' ImagingCore (what font.getmask2 returns) as uint8 [h, w]"""
    w, h = core.size
    return np.frombuffer(bytes(core), dtype=np.uint8).reshape(h, w) if w and h else np.zeros((h, w), np.uint8)


class LabelAtlas:
    """Every label the drawing can need at ONE font size, rendered once on the host with PIL: for class c and hundredths k the text '{name} {k / 100:.2f}' as the
    8-bit coverage mask `font.getmask2(label, 'L', anchor='la')` returns, packed into one uint8 `blob`, and `table` int32 [num_classes * 101, 7] = (byte offset, mask w,
    mask h, ox, oy, label_w, label_h): (ox, oy) is where ImageDraw.text puts the mask relative to the text origin, (label_w, label_h) = textbbox((0, 0), label, font)[2:4]
    (what the removed `textsize` returned).  `font`: None = ImageFont.load_default(size), a path for ImageFont.truetype, or a callable size -> ImageFont.
    `LabelAtlas.get` caches per (names, font, size); `from_arrays` builds one from stored arrays without PIL and puts it in that cache."""
    _cache = {}

    def __init__(self, class_names, font_size, font=None, _arrays=None):
        self.class_names, self.font_size, self.font = tuple(str(n) for n in class_names), int(font_size), font
        if _arrays is None:
            from PIL import Image, ImageDraw, ImageFont
            fnt = font(self.font_size) if callable(font) else ImageFont.load_default(self.font_size) if font is None else ImageFont.truetype(font, self.font_size)
            draw = ImageDraw.Draw(Image.new('RGB', (1, 1)))
            table, masks, off = np.zeros((len(self.class_names) * DRAW_SCORES, DRAW_LABEL_COLS), np.int32), [], 0
            for c, name in enumerate(self.class_names):
                for k in range(DRAW_SCORES):
                    label = '{} {:.2f}'.format(name, k / 100)
                    core, (ox, oy) = fnt.getmask2(label, 'L', anchor='la')
                    m = _core_bytes(core)
                    lw, lh = draw.textbbox((0, 0), label, font=fnt)[2:4]
                    table[c * DRAW_SCORES + k] = (off, m.shape[1], m.shape[0], ox, oy, lw, lh)
                    masks.append(m.reshape(-1))
                    off += m.size
            _arrays = (table, np.concatenate(masks) if off else np.zeros(0, np.uint8))
        self.table = np.ascontiguousarray(_arrays[0], dtype=np.int32).reshape(-1, DRAW_LABEL_COLS)
        self.blob = np.ascontiguousarray(_arrays[1], dtype=np.uint8).reshape(-1)
        if len(self.table) != len(self.class_names) * DRAW_SCORES:
            raise ValueError("LabelAtlas: the table holds 101 labels per class, 7 numbers each")

    @classmethod
    def from_arrays(cls, class_names, font_size, table, blob, font=None):
        a = cls(class_names, font_size, font, _arrays=(table, blob))
        cls._cache[(a.class_names, font, a.font_size)] = a
        for key in [k for k in _DRAW_ATLASES if k[:2] == (a.class_names, font) and a.font_size in k[2]]:
            del _DRAW_ATLASES[key]                           # device copies that hold the arrays this call replaces
        return a

    @classmethod
    def get(cls, class_names, font_size, font=None):
        key = (tuple(str(n) for n in class_names), font, int(font_size))
        if key not in cls._cache:
            cls._cache[key] = cls(class_names, font_size, font)
        return cls._cache[key]


class DrawStyle:
    """How `draw_detections_frames` draws: `class_names` (the label texts; their number is num_classes, at most 256), `colors` uint8 [num_classes, 3] (None: the
    reference's `class_colors`), `skip`: class names or ids that are not drawn (the reference skips 'sailor'), `font` as `LabelAtlas` takes it, `ink` the text colour.
    `font_size` / `thickness`: None = the reference's rules per frame, floor(0.03 H + 0.5) and max((W + H) // mean(input_shape), 1); a number fixes it for every frame (`thickness` may also be one number per frame)."""

    def __init__(self, class_names, colors=None, skip=(), font=None, ink=(0, 0, 0), font_size=None, thickness=None):
        self.class_names = tuple(str(n) for n in class_names)
        n = len(self.class_names)
        if not 1 <= n <= 256:
            raise ValueError("DrawStyle: 1..256 class names")
        self.colors = class_colors(n) if colors is None else np.asarray(colors, dtype=np.uint8).reshape(n, 3)
        self.skip = tuple(sorted(self.class_names.index(k) if isinstance(k, str) else int(k) for k in skip))
        if any(k < 0 or k >= n for k in self.skip):
            raise ValueError("DrawStyle: `skip` names classes of `class_names`")
        self.font, self.ink, self.font_size, self.thickness = font, tuple(int(v) for v in ink), font_size, thickness
        b = np.zeros(DRAW_STYLE_BYTES, np.uint8)
        b[:3 * n] = self.colors.reshape(-1)
        b[[DRAW_STYLE_SKIP + k for k in self.skip]] = 1
        b[DRAW_STYLE_INK:DRAW_STYLE_INK + 3] = self.ink
        self.bytes = b

    def font_size_for(self, h):
        return int(np.floor(3e-2 * h + 0.5)) if self.font_size is None else int(self.font_size)

    def thickness_for(self, b, h, w, input_shape):
        if self.thickness is None:
            return int(max((w + h) // np.mean(input_shape), 1))
        if not hasattr(self.thickness, '__len__'):
            return int(self.thickness)
        if b >= len(self.thickness):
            raise ValueError(f"DrawStyle: `thickness` holds {len(self.thickness)} values for a batch with a frame {b}")
        return int(self.thickness[b])


_DRAW_ATLASES = {}                 # insertion-ordered; at most _DRAW_ATLASES_MAX entries, the oldest dropped first
_DRAW_ATLASES_MAX = 16


def _device_atlases(style, sizes, device):
    """the atlases of the font sizes one call needs, concatenated: (host label table, its device copy, device blob, {size: first entry}); cached per (names, font, sizes,
    device), so only the first call with a new set of sizes renders and uploads anything.  The cache is bounded: a stream of ever new sets of frame heights keeps the 16
    newest sets and uploads again for an older one; `LabelAtlas.from_arrays` drops the entries that hold the arrays it replaces."""
    key = (style.class_names, style.font, sizes, str(device))
    if key not in _DRAW_ATLASES:
        while len(_DRAW_ATLASES) >= _DRAW_ATLASES_MAX:
            del _DRAW_ATLASES[next(iter(_DRAW_ATLASES))]
        tables, blobs, base, off = [], [], {}, 0
        for size in sizes:
            a = LabelAtlas.get(style.class_names, size, style.font)
            t = a.table.copy()
            t[:, 0] += off
            base[size] = sum(len(x) for x in tables)
            tables.append(t)
            blobs.append(a.blob)
            off += a.blob.size
        host = np.ascontiguousarray(np.concatenate(tables))
        blob = np.concatenate(blobs + [np.zeros(16, np.uint8)])
        _DRAW_ATLASES[key] = (host, torch.from_numpy(host).to(device), torch.from_numpy(blob).to(device), base, off)
    return _DRAW_ATLASES[key]


def draw_detections_frames(arena, layout, boxes, count, shapes, style, input_shape, class_counts=None):
    """The drawing the reference's detect_image ends with (achelous.py:400-433), for B frames of different sizes, IN PLACE and byte for byte PIL's: per kept detection
    `boxes[b, j]`, j < count[b], in that order — later drawing overwrites earlier — `thickness` one-pixel rings of the box in the class colour, the filled label plate
    above the box (inside it when there is no room) and the label '{name} {obj * cls:.2f}' in `style.ink`.  Rows whose class is in `style.skip`, whose id is outside
    [0, num_classes) or that hold a non-finite number are not drawn.

    arena: 1-D uint8 tensor of packed HWC frames; layout: (byte offsets, pitches) per frame, or what `frames_layout(shapes)` returns (its overlay part is used) — offsets
    and pitches are multiples of 4, as `seg_maps_frames` lays its overlay arena out.  boxes [B, max_det, 7] fp32 and count [B] int32 as `correct_boxes_frames` returns
    them, `shapes` one (H, W) per frame, `style` a `DrawStyle`, `input_shape` the network's (R, R).  class_counts: optional int32 [B, num_classes] tensor that receives
    the number of kept rows per class id (the reference's count=True tally; skipped classes count, rows past count[b] do not).
    Two launches whatever B is; the per-frame table travels in one non-blocking copy; no host read, no synchronisation.  Returns the per-frame [H, W, 3] views.
    Not covered: crop=True (data-dependent output sizes), file output (the scatter of the point classes is `scatter_points_frames`)."""
    from . import data as _data
    lib = _pass_lib(arena)
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise ValueError("draw_detections_frames: `arena` is a contiguous 1-D uint8 tensor")
    if boxes.dtype != torch.float32 or boxes.dim() != 3 or boxes.shape[2] != 7 or count.dtype != torch.int32 or count.numel() != boxes.shape[0]:
        raise ValueError("draw_detections_frames: boxes [B, max_det, 7] float32 and count [B] int32 expected")
    if boxes.device != arena.device or count.device != arena.device:
        raise ValueError("draw_detections_frames: boxes, count and the arena live on one device")
    boxes, count = boxes.contiguous(), count.contiguous()
    B, max_det, _ = boxes.shape
    shapes = _frame_shapes(shapes, B)
    offs, pitches = (layout[3], layout[4]) if len(layout) == 6 else layout
    if len(offs) != B or len(pitches) != B:
        raise ValueError("draw_detections_frames: one offset and one pitch per frame")
    nc = len(style.class_names)
    if class_counts is not None and (class_counts.dtype != torch.int32 or tuple(class_counts.shape) != (B, nc) or not class_counts.is_contiguous() or class_counts.device != arena.device):
        raise ValueError("draw_detections_frames: class_counts is a contiguous int32 [B, num_classes] tensor on the arena's device")
    sizes = [style.font_size_for(h) for h, w in shapes]
    labels_host, labels_dev, blob_dev, base, blob_bytes = _device_atlases(style, tuple(sorted(set(sizes))), arena.device)
    table = np.zeros((B, DRAW_TABLE_COLS), np.int64)
    for b, (h, w) in enumerate(shapes):
        table[b, :6] = (int(offs[b]), h, w, int(pitches[b]), style.thickness_for(b, h, w, input_shape), base[sizes[b]])
    meta = _data._Meta(arena.device, 'serve_draw')
    tref, sref = meta.add(table), meta.add(style.bytes)
    meta.commit()
    recs = torch.empty(B * max_det * DRAW_REC, dtype=torch.int32, device=arena.device)
    ctx = torch.cuda.device(arena.device) if arena.is_cuda else contextlib.nullcontext()
    with ctx:
        _check(lib, lib.lib.ach_draw_detections_frames(_ptr(arena), arena.numel(), meta.host_ptr(tref), meta.dev_ptr(tref), B, _ptr(boxes), _ptr(count), max_det, nc,
                                                       labels_host.ctypes.data, _ptr(labels_dev), len(labels_host), _ptr(blob_dev), blob_bytes, meta.dev_ptr(sref),
                                                       _ptr(recs), _ptr(class_counts), _stream(arena)), _DRAW_ERRORS, 'draw kernels')
    return [torch.as_strided(arena, (h, w, 3), (int(pitches[b]), 3, 1), int(offs[b])) for b, (h, w) in enumerate(shapes)]


# ------------------------------------------------------------------------------------------------- the heat-map mode (csrc/k_heatmap.h)
HEAT_TABLE_COLS = 16        # k_heatmap.h


class HeatmapStyle:
    """How `heatmap_frames` colours: `alpha` of the colour over the base image (the reference's 0.5), `cmap` uint8 [256, 3] (None: matplotlib's jet, shipped as a table:
    `colormaps.JET`), `window`: 'full' stretches every level's whole map over the frame as the reference does, 'letterbox' only the part the frame's letterbox fills,
    `over` (read by `detect_frames`): 'frame' colours the camera frame as the reference does, 'overlay' the segmentation overlay."""

    def __init__(self, alpha=0.5, cmap=None, window='full', over='frame'):
        from .colormaps import JET
        self.alpha = float(alpha)
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError("HeatmapStyle: alpha lies in [0, 1]")
        c = JET if cmap is None else np.asarray(cmap)
        if c.dtype != np.uint8 or c.shape != (256, 3):
            raise ValueError("HeatmapStyle: `cmap` is a uint8 [256, 3] table")
        if window not in ('full', 'letterbox') or over not in ('frame', 'overlay'):
            raise ValueError("HeatmapStyle: window is 'full' or 'letterbox', over is 'frame' or 'overlay'")
        self.cmap, self.window, self.over = np.ascontiguousarray(c), window, over


def heatmap_frames(det, shapes, base, layout=None, style=None, input_shape=None, letterbox_image=True, out=None, inplace=False):
    """The reference's heat-map mode (achelous.detect_heatmap, achelous.py:451-555) for B frames of different sizes, from the detection maps `det` = (det3, det4, det5)
    [B, 5 + num_det, R/s, R/s] (s = 8, 16, 32; fp32, bf16 or fp16) that `forward_detect` returns, in three launches whatever B is:

    heat_mask: per frame the uint8 [H, W] mask max_l uint8(trunc(cv2.resize(max_c sigmoid(cls) * sigmoid(obj), (W, H)) * 255)) — the reference's arithmetic
    (achelous.py:457-459, 539-546; INTER_LINEAR as `oracle/prepost.py:resize_linear` restates it, float32, never contracted).  A cell with a NaN logit scores 0.
    heat_range: int32 [B, 2] = (lo, hi), the mask's minimum and maximum, which is what matplotlib's Normalize scales the colour map by.
    heatmap: per frame uint8 [H, W, 3] = Image.blend(base, cmap[min(int((m - lo) / (hi - lo) * 256), 255)], alpha), entry 0 on a flat mask: the colour is byte for byte
    `matplotlib.cm.jet(Normalize(lo, hi)(mask), bytes=True)`, the compositing is PIL's `Image.blend`, at the frame's own size.  matplotlib's Agg compositing and its
    resampling to the figure's size (achelous.py:548-553) are NOT reproduced.

    style.window: 'full' is the reference, which stretches the whole map over the frame even when the frame was letterboxed; 'letterbox' (with letterbox_image=True)
    stretches the window `letterbox_window` gives instead, so that the heat lies on what it belongs to.  The interpolation still clamps at the map's edge, not the
    window's, so up to half a cell of the grey bars' score bleeds in at the window's edge.

    base: the image under the colour — a `data.Arena` (layout: None) or a 1-D uint8 tensor of packed HWC frames with `layout` = (byte offsets, pitches) per frame or
    what `frames_layout(shapes)` returns (its overlay part); None: mask and range only (two launches).  The coloured frames go to an arena of their own laid out by
    `frames_layout` (`out`: a 1-D uint8 tensor to use), or with inplace=True over `base` itself (its offsets and pitches are then multiples of 16, as an overlay
    arena's are).  input_shape: the network's (R, R), default 8 x det3's size.  Returns dict(heat_mask, heat_range, heatmap (with a base), scores float32 [B, A]
    level-major, arenas).  One non-blocking copy for the tables; no host read, no synchronisation."""
    from . import data as _data
    from .engine import NativeEngine
    style = HeatmapStyle() if style is None else style
    if len(det) != 3 or any(d.dim() != 4 or d.dtype != det[0].dtype or d.device != det[0].device or d.shape[:2] != det[0].shape[:2] for d in det):
        raise ValueError("heatmap_frames: det = (det3, det4, det5), [B, 5 + num_det, R/s, R/s] of one dtype on one device")
    det = [d.contiguous() for d in det]
    lib = _pass_lib(det[0])
    if det[0].dtype not in _DTYPE_CODE:
        raise TypeError(f"heatmap_frames: float32, bfloat16 or float16 detection maps, got {det[0].dtype}")
    B, C = int(det[0].shape[0]), int(det[0].shape[1])
    R = 8 * int(det[0].shape[2]) if input_shape is None else int(input_shape[0])
    if C < 6 or (input_shape is not None and int(input_shape[1]) != R) or any(tuple(d.shape[2:]) != (R // s, R // s) for d, s in zip(det, (8, 16, 32))):
        raise ValueError("heatmap_frames: det maps of [B, 5 + num_det, R/8 | R/16 | R/32 squared] for a square input_shape (R, R) expected")
    shapes = _frame_shapes(shapes, B)
    dev = det[0].device
    A = (R // 8) ** 2 + (R // 16) ** 2 + (R // 32) ** 2
    moff, mp, mbytes, ooff, op, obytes = frames_layout(shapes)
    table = np.zeros((B, HEAT_TABLE_COLS), np.int64)
    for b, (h, w) in enumerate(shapes):
        table[b, 1:3] = (h, w)
        table[b, 4:8] = letterbox_window(h, w, R) if (style.window == 'letterbox' and letterbox_image) else (0, 0, R, R)
        table[b, 8:12] = (moff[b], mp[b], ooff[b], op[b])
    base_t = None
    if base is not None:
        if isinstance(base, _data.Arena):
            if len(base.frames) != B or any(f is None or (f[1], f[2]) != sh for f, sh in zip(base.frames, shapes)):
                raise ValueError("heatmap_frames: `base` holds one image per frame, of the sizes in `shapes`")
            base_t, boffs, bpitches = base.data, [f[0] for f in base.frames], [f[3] for f in base.frames]
        else:
            if layout is None:
                raise ValueError("heatmap_frames: a tensor `base` needs its `layout`")
            base_t = base
            boffs, bpitches = (layout[3], layout[4]) if len(layout) == 6 else layout
        if base_t.dtype != torch.uint8 or base_t.dim() != 1 or not base_t.is_contiguous() or base_t.device != dev:
            raise ValueError("heatmap_frames: `base` is a contiguous 1-D uint8 tensor on the det maps' device")
        if len(boffs) != B or len(bpitches) != B:
            raise ValueError("heatmap_frames: one offset and one pitch per frame")
        for b in range(B):
            table[b, 0], table[b, 3] = int(boffs[b]), int(bpitches[b])
        if inplace:
            table[:, 10], table[:, 11] = table[:, 0], table[:, 3]
    elif inplace or out is not None:
        raise ValueError("heatmap_frames: `out` / inplace need a `base`")
    meta = _data._Meta(dev, 'serve_heat')
    tref, cref = meta.add(table), meta.add(style.cmap)
    meta.commit()
    scores = torch.empty(B, A, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 2, dtype=torch.int32, device=dev)
    mask = torch.empty(max(mbytes, 16), dtype=torch.uint8, device=dev)
    out_t = None
    if base_t is not None:
        if inplace:
            if out is not None:
                raise ValueError("heatmap_frames: inplace=True writes over `base`; no `out`")
            out_t = base_t
        elif out is None:
            out_t = torch.empty(max(obytes, 16), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev or out.numel() < obytes:
            raise ValueError(f"heatmap_frames: `out` is a contiguous 1-D uint8 tensor of at least {obytes} bytes on the det maps' device")
        else:
            out_t = out
    ctx = torch.cuda.device(dev) if det[0].is_cuda else contextlib.nullcontext()
    with ctx:
        NativeEngine.heatmap_frames(lib, _DTYPE_CODE[det[0].dtype], R, C - 5, B, det[0], det[1], det[2], scores, base_t, 0 if base_t is None else base_t.numel(),
                                    meta.host_ptr(tref).value, meta.dev_ptr(tref).value, meta.dev_ptr(cref).value, style.alpha, mask, mask.numel(), stats, out_t,
                                    0 if out_t is None else out_t.numel(), _stream(det[0]).value)
    res = {'heat_mask': [torch.as_strided(mask, (h, w), (mp[b], 1), moff[b]) for b, (h, w) in enumerate(shapes)],
           'heat_range': torch.stack((255 - stats[:, 1], stats[:, 0]), dim=1), 'scores': scores, 'arenas': {'heat_mask': mask}}
    if out_t is not None:
        res['heatmap'] = [torch.as_strided(out_t, (h, w, 3), (int(table[b, 11]), 3, 1), int(table[b, 10])) for b, (h, w) in enumerate(shapes)]
        res['arenas']['heatmap'] = out_t
    return res


# ------------------------------------------------------------------------------------------------- the point classes on the frames (csrc/k_scatter.h)
SCATTER_TABLE_COLS, SCATTER_MAX_POINTS = 16, 4096        # k_scatter.h


class ScatterStyle:
    """How `scatter_points_frames` paints: `cmap` uint8 [256, 3] (None: matplotlib's default viridis, shipped as `colormaps.VIRIDIS`), normalised per frame to the
    smallest and largest class among the frame's rows as matplotlib's `c=` does; `class_range` = (lo, hi) fixes that range for every frame, so that a class keeps its
    colour from frame to frame (ids outside it clamp to its ends); `colors` uint8 [num_classes, 3] replaces the map by a per-class palette.  `alpha` of a disc over what
    lies under it (the reference's 0.98).  A row's disc has the diameter size_scale * sqrt(s) pixels, its radius at most `max_radius` (1..256) pixels.  `columns`: the
    cloud's columns of (rcs, u, v) — None: `data.MAP_COLUMNS[2:5]`, or the serving call's `columns`."""

    def __init__(self, cmap=None, colors=None, class_range=None, alpha=0.98, size_scale=1.0, max_radius=64, columns=None):
        from .colormaps import VIRIDIS
        self.alpha, self.size_scale, self.max_radius = float(alpha), float(size_scale), int(max_radius)
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError("ScatterStyle: alpha lies in [0, 1]")
        if not 1 <= self.max_radius <= 256 or self.max_radius != max_radius:
            raise ValueError("ScatterStyle: max_radius is an integer in 1..256")
        self.k = self.size_scale * self.size_scale / 4.0
        if not (self.size_scale > 0 and math.isfinite(self.k) and self.k > 0):
            raise ValueError("ScatterStyle: size_scale is above 0")
        c = VIRIDIS if cmap is None else np.asarray(cmap)
        if c.dtype != np.uint8 or c.shape != (256, 3):
            raise ValueError("ScatterStyle: `cmap` is a uint8 [256, 3] table")
        self.cmap = np.ascontiguousarray(c)
        self.colors = None
        if colors is not None:
            p = np.asarray(colors)
            if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= 256:
                raise ValueError("ScatterStyle: `colors` is a uint8 [num_classes, 3] palette of at most 256 classes")
            self.colors = np.ascontiguousarray(p)
        self.class_range = None
        if class_range is not None:
            lo, hi = (int(v) for v in class_range)
            if not 0 <= lo <= hi <= 255:
                raise ValueError("ScatterStyle: class_range = (lo, hi) with 0 <= lo <= hi <= 255")
            self.class_range = (lo, hi)
        self.columns = None if columns is None else tuple(int(c) for c in columns)
        if self.columns is not None and len(self.columns) != 3:
            raise ValueError("ScatterStyle: `columns` are the cloud's three columns of rcs, u, v")

    def table(self, num_classes):
        """(the 768 colour bytes, colour mode of k_scatter.h, lo, hi)"""
        if self.colors is not None:
            if len(self.colors) < num_classes:
                raise ValueError(f"ScatterStyle: `colors` holds {len(self.colors)} colours for {num_classes} classes")
            t = np.zeros((256, 3), np.uint8)
            t[:len(self.colors)] = self.colors
            return t, 2, 0, 0
        return (self.cmap, 0, 0, 0) if self.class_range is None else (self.cmap, 1, self.class_range[0], self.class_range[1])


def scatter_points_frames(arena, layout, shapes, points, point_class, num_classes, style=None, indices=None, _columns=None):
    """The reference's picture of the radar point classes (achelous.py:261-271) for B frames of different sizes, IN PLACE on a packed HWC uint8 arena, in two launches
    whatever B is.  For frame b and sample j < N: (u, v, s) = the cloud's u, v and rcs columns at row indices[b, j], as float64; c = point_class[b, j].

    point_rows: float64 [B, N, 4], the reference's `output_seg_pc_collections` = np.unique(concat[u, v, rcs, class], axis=0): the samples sorted ascending by
    (u, v, s, c) by value, equal rows once, rows past point_count[b] zero.  A sample leaves when u, v or s is not finite, when its class is outside [0, num_classes)
    (our rule: the reference would hand NaN to matplotlib) or when its index is outside its cloud.  point_count: int32 [B].
    point_class_range: int32 [B, 2], the smallest and largest class among a frame's rows, (0, 0) without one: what matplotlib's `c=` normalises the colour map by.
    Colour: style.cmap[0] when hi == lo, else style.cmap[min((c - lo) * 256 // (hi - lo), 255)] — byte for byte cm.viridis(Normalize(lo, hi)(c), bytes=True); or over
    style.class_range, or style.colors[c].
    Geometry (our rule — the reference's marker size is in points of a figure whose scale to image pixels it never fixes): a pixel has its centre at integer
    coordinates, as imshow places it, and a row covers pixel (x, y) iff s > 0 and (x - u)^2 + (y - v)^2 <= min(size_scale^2 / 4 * s, max_radius^2), in float64, every
    operation rounded once: a disc of diameter size_scale * sqrt(s) pixels.  No anti-aliasing: matplotlib's Agg edges are NOT reproduced, nor its figure or file output.
    Paint: the rows in their sorted order, later over earlier, every covered pixel = Image.blend(pixel, colour, style.alpha) per covering row (PIL's arithmetic).  A
    byte no disc covers is not written.

    arena: 1-D uint8 tensor of packed HWC frames; layout: (byte offsets, pitches) per frame, or what `frames_layout(shapes)` returns (its overlay part) — multiples of 4.
    points: a `data.Clouds`, a list of host clouds [n_i, F] (uploaded once; the columns are style.columns), or a dense device tensor [B, N, 3] = (u, v, s) float32 /
    float64.  point_class: [B, N] integer tensor on the arena's device.  indices: [B, N] (host array or device tensor), None: sample j is row j.  N is at most 4096.
    The table, the colours and host indices travel in one non-blocking copy; no host read, no synchronisation.
    Returns dict(frames: the per-frame [H, W, 3] views, point_rows, point_count, point_class_range)."""
    from . import data as _data
    style = ScatterStyle() if style is None else style
    lib = _pass_lib(arena)
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise ValueError("scatter_points_frames: `arena` is a contiguous 1-D uint8 tensor")
    dev = arena.device
    if point_class.dim() != 2 or point_class.dtype.is_floating_point or point_class.device != dev:
        raise ValueError("scatter_points_frames: point_class is an integer tensor [B, N] on the arena's device")
    B, N = (int(v) for v in point_class.shape)
    if not 1 <= N <= SCATTER_MAX_POINTS:
        raise ValueError(f"scatter_points_frames: 1..{SCATTER_MAX_POINTS} points per frame, got {N}")
    cls = point_class.to(torch.int64).contiguous()
    shapes = _frame_shapes(shapes, B)
    offs, pitches = (layout[3], layout[4]) if len(layout) == 6 else layout
    if len(offs) != B or len(pitches) != B:
        raise ValueError("scatter_points_frames: one offset and one pitch per frame")
    table = np.zeros((B, SCATTER_TABLE_COLS), np.int64)
    if isinstance(points, torch.Tensor):
        if tuple(points.shape) != (B, N, 3) or points.dtype not in (torch.float32, torch.float64) or points.device != dev:
            raise ValueError("scatter_points_frames: dense points are a float32 / float64 tensor [B, N, 3] = (u, v, size) on the arena's device")
        cloud = points.contiguous()
        for b in range(B):
            table[b, 4:11] = (b * N * 3, N, 3, 3, 0, 1, 2)
    else:
        packed = _data._as_clouds(points, dev, 'scatter_clouds')
        cloud = packed.data
        if len(packed.frames) != B or cloud.device != dev:
            raise ValueError(f"scatter_points_frames: one cloud per frame on the arena's device expected, got {len(packed.frames)} for {B} frames")
        rcs, cu, cv = _columns or style.columns or _data.MAP_COLUMNS[2:5]
        for b, fr in enumerate(packed.frames):
            table[b, 4:11] = tuple(fr) + (cu, cv, rcs)
    for b, (h, w) in enumerate(shapes):
        table[b, :4] = (int(offs[b]), h, w, int(pitches[b]))
    colours, mode, lo, hi = style.table(int(num_classes))
    meta = _data._Meta(dev, 'serve_scatter')
    tref, cref, iref = meta.add(table), meta.add(colours), None
    idx_dev = None
    if isinstance(indices, torch.Tensor) and indices.device.type != 'cpu':
        if tuple(indices.shape) != (B, N) or indices.device != dev:
            raise ValueError("scatter_points_frames: indices are [B, N] on the arena's device or on the host")
        idx_dev = indices.to(torch.int64).contiguous()
    elif indices is not None:
        idx = np.ascontiguousarray(indices.numpy() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64)
        if idx.shape != (B, N):
            raise ValueError(f"scatter_points_frames: indices are [B, N] = [{B}, {N}]")
        iref = meta.add(idx)
    meta.commit()
    rows = torch.empty(B, N, 4, dtype=torch.float64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    rng = torch.empty(B, 2, dtype=torch.int32, device=dev)
    discs = torch.empty(B * N * 4, dtype=torch.float64, device=dev)
    boxes = torch.empty(B * N * 4, dtype=torch.int32, device=dev)
    ctx = torch.cuda.device(dev) if arena.is_cuda else contextlib.nullcontext()
    with ctx:
        _check(lib, lib.lib.ach_scatter_points_frames(_ptr(arena), arena.numel(), meta.host_ptr(tref), meta.dev_ptr(tref), B, _ptr(cloud), cloud.numel(),
                                                      0 if cloud.dtype == torch.float32 else 1, _ptr(idx_dev) if iref is None else meta.dev_ptr(iref), _ptr(cls), N,
                                                      int(num_classes), meta.dev_ptr(cref), mode, lo, hi, style.alpha, style.k, style.max_radius, _ptr(rows), _ptr(count),
                                                      _ptr(rng), _ptr(discs), discs.numel() * 8, _ptr(boxes), boxes.numel() * 4, _stream(arena)),
               _DRAW_ERRORS, 'scatter kernels')
    return {'frames': [torch.as_strided(arena, (h, w, 3), (int(pitches[b]), 3, 1), int(offs[b])) for b, (h, w) in enumerate(shapes)],
            'point_rows': rows, 'point_count': count, 'point_class_range': rng}


def detect_frames(net, frames, radar_maps, points, conf_thres=0.5, nms_thres=0.4, letterbox_image=True, max_det=100, dtype=torch.bfloat16, overlay=True,
                  palette_se=PALETTE_SEG, palette_line=PALETTE_LINE, keep_classes=None, blend=(0.45, 0.3), brightness=1.3, draw=None, heatmap=None, scatter=None,
                  point_uvs=None):
    """`detect_frame` for B frames of DIFFERENT sizes: the arithmetic of the reference's detect_image (achelous.py:190-433) without its file I/O; the box drawing
    (achelous.py:363-433) is on with `draw`.

    frames: a list of CPU uint8 [H_i, W_i, 3] arrays / tensors, or a `data.Arena` already on the device; radar_maps [B, 3, R, R] float and points
    [B, N, pc_channels] float on the GPU.  One upload (`data.pack_arena`), the letterbox of all frames in two launches (`data.letterbox_batch`; with
    letterbox_image=False every frame is stretched over the whole input), the batched radar / point preparation, ONE `forward_detect`, one box-correction launch
    and one launch for both class maps and the overlay of every frame.  The launch count does not depend on B and nothing is read back or synchronised, so the
    boxes are NOT cut to their count here: the caller slices `boxes[b, :count[b]]` when it reads `count`.

    Returns dict(boxes [B, max_det, 7] = (y1, x1, y2, x2 in the frame's own pixels, obj, class conf, class id), rows past count[b] zero; count [B] int32;
    semantic, waterline: lists of [H_i, W_i] uint8 views; overlay: list of [H_i, W_i, 3] uint8 views (overlay=True; `seg_maps_frames`); point_class [B, N] int64).
    draw: None, or a `DrawStyle` — two more launches (`draw_detections_frames`) then draw every kept detection's box, plate and label on the overlay (overlay=True
    is required), and the result gains class_counts [B, num_classes] int32, the kept rows per class id.  With draw=None nothing changes.
    heatmap: None, or a `HeatmapStyle` — three more launches (`heatmap_frames`) on the det maps of the same `forward_detect`, and the result gains heat_mask,
    heat_range and heatmap; the colour goes over the camera frames (style.over = 'frame', the reference) or over the overlay as it is after the drawing ('overlay',
    needs overlay=True), into an arena of its own: every other key is what it is without `heatmap`, and with heatmap=None nothing changes.
    scatter: None, or a `ScatterStyle` — two more launches (`scatter_points_frames`) paint the radar point classes on the overlay (overlay=True is required) after the
    drawing and before a heat map with over='overlay', as the reference's scatter lies above the image with its boxes; `point_uvs` [B, N, 3] float32 / float64 on the
    device holds every point's (u, v, size) in the frame's own pixels.  The result gains point_rows, point_count and point_class_range; with scatter=None nothing changes."""
    from . import data as _data
    _need_overlay(draw, overlay, heatmap, scatter)
    if scatter is not None and point_uvs is None:
        raise ValueError("detect_frames: `scatter` needs `point_uvs` [B, N, 3] = (u, v, size)")
    R = net.resolution
    arena = _data._as_arena(frames, 3, radar_maps.device, 'images')
    B = len(arena.frames)
    x = _data.letterbox_batch(arena, R, None if letterbox_image else [(R, R, 0, 0)] * B, dtype)
    xr = preprocess_input_radar(radar_maps, dtype)
    xp = normalize_points(points, dtype)
    return _detect_prepared(net, arena, x, xr, xp, conf_thres, nms_thres, letterbox_image, max_det, overlay, palette_se, palette_line, keep_classes, blend, brightness, draw, heatmap,
                            scatter, (point_uvs, None, None))


def _need_overlay(draw, overlay, heatmap=None, scatter=None):
    if scatter is not None and not overlay:
        raise ValueError("detect_frames: `scatter` paints on the overlay, so it needs overlay=True")
    if draw is not None and not overlay:
        raise ValueError("detect_frames: `draw` draws on the overlay, so it needs overlay=True")
    if heatmap is not None and heatmap.over == 'overlay' and not overlay:
        raise ValueError("detect_frames: `heatmap` with over='overlay' colours the overlay, so it needs overlay=True")


def _detect_prepared(net, arena, x, xr, xp, conf_thres, nms_thres, letterbox_image, max_det, overlay, palette_se, palette_line, keep_classes, blend, brightness, draw=None, heatmap=None,
                     scatter=None, scatter_source=None):
    """`detect_frames` from the three prepared network inputs on; scatter_source: (points, indices, columns) as `scatter_points_frames` takes them"""
    R, B = net.resolution, len(arena.frames)
    shapes = [(f[1], f[2]) for f in arena.frames]
    (det, se, lane, pc), (rows, idx, cnt) = net.forward_detect(x, xr, xp, conf_thres, nms_thres, max_det)
    boxes = correct_boxes_frames(rows, cnt, (R, R), shapes, letterbox_image)
    maps = seg_maps_frames(se, lane, shapes, arena if overlay else None, palette_se, palette_line, keep_classes, blend, brightness,
                           windows=None if letterbox_image else [(0, 0, R, R)] * B)
    res = {'boxes': boxes, 'count': cnt, 'semantic': maps['semantic'], 'waterline': maps['waterline'], 'point_class': pc.float().argmax(-1)}
    if overlay:
        res['overlay'] = maps['overlay']
    if draw is not None:
        res['class_counts'] = torch.empty(B, len(draw.class_names), dtype=torch.int32, device=boxes.device)
        draw_detections_frames(maps['arenas']['overlay'], frames_layout(shapes), boxes, cnt, shapes, draw, (R, R), res['class_counts'])
    if scatter is not None:
        pts = scatter_points_frames(maps['arenas']['overlay'], frames_layout(shapes), shapes, scatter_source[0], res['point_class'], int(pc.shape[-1]), scatter,
                                    scatter_source[1], _columns=scatter_source[2])
        res.update({k: pts[k] for k in ('point_rows', 'point_count', 'point_class_range')})
    if heatmap is not None:
        under = (maps['arenas']['overlay'], frames_layout(shapes)) if heatmap.over == 'overlay' else (arena, None)
        heat = heatmap_frames(det, shapes, under[0], under[1], heatmap, (R, R), letterbox_image)
        res.update({k: heat[k] for k in ('heat_mask', 'heat_range', 'heatmap')})
    return res


def detect_frames_from_clouds(net, frames, clouds, indices=None, rng=None, num_points=512, columns=None, point_columns=None, cell=None, conf_thres=0.5, nms_thres=0.4,
                              letterbox_image=True, max_det=100, dtype=torch.bfloat16, overlay=True, palette_se=PALETTE_SEG, palette_line=PALETTE_LINE,
                              keep_classes=None, blend=(0.45, 0.3), brightness=1.3, device='cuda', draw=None, heatmap=None, scatter=None):
    """`detect_frames` from raw radar point clouds instead of ready radar maps and sampled points: `clouds` is a list of CPU float32 / float64 arrays [n_i, F] (or
    `data.Clouds` already on the device), uploaded once.  The normalised radar map is `data.radar_maps_batch(..., normalize=True)` (the reference's offline
    rasterisation, then its min-max scaling: `columns` = the columns of range, doppler, rcs, u, v, default 0..4; `cell` default (6.0, 3.375)); the points are
    `data.radar_points_batch`: `num_points` rows per frame by `indices` [B, N] or drawn from `rng`, the columns `point_columns` (default: the first
    `net.pc_channels`), normalised.  Two launches for the map and one for the points whatever B is, nothing read back; everything else and the result as `detect_frames`.
    scatter: None, or a `ScatterStyle` — the point classes painted on the overlay (`scatter_points_frames`, two more launches) from the packed clouds themselves: the
    rows the points were sampled by (`indices`, or the ones drawn from `rng`) and the rcs, u, v columns of `columns` (or style.columns)."""
    from . import data as _data
    _need_overlay(draw, overlay, heatmap, scatter)
    R = net.resolution
    packed = _data._as_clouds(clouds, device)
    arena = _data._as_arena(frames, 3, packed.data.device, 'images')
    B = len(arena.frames)
    if len(packed.frames) != B:
        raise ValueError(f"detect_frames_from_clouds: one cloud per frame expected, got {len(packed.frames)} for {B} frames")
    x = _data.letterbox_batch(arena, R, None if letterbox_image else [(R, R, 0, 0)] * B, dtype)
    xr = _data.radar_maps_batch(packed, R, _data.MAP_COLUMNS if columns is None else columns, _data.CELL if cell is None else cell, True, dtype)
    source = None
    if scatter is not None:                                              # the rows the points are sampled by, drawn here so that the scatter reads the same ones
        indices = _data.draw_indices([f[1] for f in packed.frames], num_points, indices, rng)
        source = (packed, indices, scatter.columns or tuple((_data.MAP_COLUMNS if columns is None else columns)[2:5]))
    xp, _ = _data.radar_points_batch(packed, tuple(range(net.pc_channels)) if point_columns is None else point_columns, None, num_points, indices, rng, dtype)
    return _detect_prepared(net, arena, x, xr, xp, conf_thres, nms_thres, letterbox_image, max_det, overlay, palette_se, palette_line, keep_classes, blend, brightness, draw, heatmap,
                            scatter, source)
