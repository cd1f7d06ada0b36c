"""ctypes binding of the C ABI in include/achelous.h (libachelous_hip.so).

PyTorch is plumbing here: it owns device memory and streams; tensors cross the boundary as raw
`data_ptr()`s.  The library is built in-tree by `make -C achelous_amd/csrc` (see __graft_entry__.build()).
There is NO fallback: if the HIP library cannot be loaded, or a tensor is not on a GPU, this raises.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIBRARY = os.path.join(_HERE, 'libachelous_hip.so')
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'achelous.h')

DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2      # include/achelous.h ACH_DTYPE_*: storage type of the activations (F16: inputs / outputs fp16, or bf16 with option io_bf16)
BACKBONES = {'en': 0, 'mv': 1, 'pf': 2, 'rv': 4}       # (3 is reserved for the reference's default 'ef' and refused)
PHIS = {'S0': 0, 'S1': 1, 'S2': 2}
NECKS = {'gdf': 0, 'cdf': 1}
PC_SEGS = {'pn': 0, 'pn2': 1, 'none': 2, 'pn2_msg': 3}     # 'none': Achelous3T (nets/Achelous.py:56-76), no point stream

_ERRORS = {-1: ValueError, -2: NotImplementedError, -3: KeyError, -4: RuntimeError, -5: MemoryError}


class AchConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('num_det', 'num_seg', 'phi', 'backbone', 'resolution', 'pc_channels',
                                              'pc_classes', 'num_points', 'nano_head', 'spp', 'dtype', 'neck', 'pc_seg')]


class AchTensorDesc(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char_p), ('data', ctypes.c_void_p), ('ndim', ctypes.c_int32),
                ('shape', ctypes.c_int64 * 4)]


_SCALARS = {'void': None, 'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t,
            'float': ctypes.c_float, 'double': ctypes.c_double}


def _ctype(decl):
    """the ctypes class of one C type as the header spells it: every pointer is c_void_p (byref(), ctypes arrays and pointer instances all pass as one),
    `const char*` is c_char_p, a scalar is looked up by name; anything else raises"""
    words = [w for w in decl.replace('*', ' ').split() if w != 'const']
    if '*' in decl:
        return ctypes.c_char_p if words == ['char'] and decl.count('*') == 1 else ctypes.c_void_p
    if len(words) != 1 or words[0] not in _SCALARS:
        raise ValueError(f'include/achelous.h: no ctypes class for the type {decl.strip()!r}')
    return _SCALARS[words[0]]


def parse_header(text):
    """{entry: (restype, [argtypes])} of every `RET ach_name(ARGS);` in the text of include/achelous.h, in the header's order"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', '', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    protos = {}
    for ret, name, args in re.findall(r'([\w\s*]+?)\b(ach_\w+)\s*\(([^()]*)\)\s*;', text):
        argtypes = []
        for arg in ([] if args.strip() == 'void' else args.split(',')):
            m = re.fullmatch(r'\s*(.*?)\b\w+\s*(\[\d*\])?\s*', arg, flags=re.S)          # type, name, the array form `int64_t shape[4]`
            if not m:
                raise ValueError(f'include/achelous.h: {name}: cannot read the parameter {arg.strip()!r}')
            argtypes.append(_ctype(m.group(1) + ('*' if m.group(2) else '')))
        protos[name] = (_ctype(ret), argtypes)
    return protos


with open(HEADER) as _f:
    PROTOTYPES = parse_header(_f.read())

# extension headers next to include/achelous.h: entries declared outside it, read and bound the same way (include/achelous_heatmap.h: the heat-map mode)
EXTENSION_HEADERS = ('achelous_heatmap.h',)
EXTENSIONS = {}
for _name in EXTENSION_HEADERS:
    with open(os.path.join(os.path.dirname(HEADER), _name)) as _f:
        EXTENSIONS.update(parse_header(_f.read()))

# include/achelous_points.h (the point-class scatter on served frames): a table of its own, read and bound the same way
with open(os.path.join(os.path.dirname(HEADER), 'achelous_points.h')) as _f:
    POINT_ENTRIES = parse_header(_f.read())

# include/achelous_optim.h (the optimizer step and weight EMA over the flat training-state arena, achelous_amd/optim.py): likewise
with open(os.path.join(os.path.dirname(HEADER), 'achelous_optim.h')) as _f:
    OPTIM_ENTRIES = parse_header(_f.read())


class NativeLibrary:
    """dlopen + prototypes for every symbol declared in include/achelous.h (SYMBOLS), in its extension headers (EXTENSIONS), in include/achelous_points.h
    (POINT_ENTRIES) and in include/achelous_optim.h (OPTIM_ENTRIES), derived from the headers themselves (parse_header)."""
    SYMBOLS = tuple(PROTOTYPES)

    def __init__(self, path):
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C achelous_amd/csrc` "
                               f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        self.path = path
        self.lib = ctypes.CDLL(path)
        # (an entry is bound where the library exports it: the co-residency tests also load libraries built from older sources; tests/test_abi_and_host.py
        #  holds the product to every declared symbol, and calling an entry a library lacks raises AttributeError)
        for name, (restype, argtypes) in {**PROTOTYPES, **EXTENSIONS, **POINT_ENTRIES, **OPTIM_ENTRIES}.items():
            fn = getattr(self.lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes


_hip_library = None


def hip_library():
    """The product library.  Raises (never falls back) when it has not been built."""
    global _hip_library
    if _hip_library is None:
        _hip_library = NativeLibrary(HIP_LIBRARY)
    return _hip_library


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


class NativeEngine:
    """One ach_handle: a (config, dtype) specialisation of the forward engine on the current device."""

    def __init__(self, lib, *, num_det, num_seg, phi, backbone, resolution, pc_channels, pc_classes, num_points,
                 nano_head, spp, dtype, neck='gdf', pc_seg='pn'):
        self.lib = lib
        self.L = lib.lib
        self.cfg = AchConfig(num_det, num_seg, PHIS[phi], BACKBONES[backbone], resolution, pc_channels, pc_classes,
                             num_points, int(bool(nano_head)), int(bool(spp)), dtype, NECKS[neck], PC_SEGS[pc_seg])
        self.dtype = dtype
        self.torch_dtype = {DTYPE_F32: torch.float32, DTYPE_BF16: torch.bfloat16, DTYPE_F16: torch.float16}[dtype]     # of the caller's tensors (bf16 after set_option('io_bf16', 1))
        self.h = ctypes.c_void_p()
        rc = self.L.ach_create(ctypes.byref(self.cfg), ctypes.byref(self.h))
        if rc != 0:
            msg = self.L.ach_last_error(None)
            raise _ERRORS.get(rc, RuntimeError)((msg or b'ach_create failed').decode())
        self.batch = 0
        self.num_det, self.num_seg, self.resolution = num_det, num_seg, resolution
        self.pc_classes, self.num_points, self.pc_channels = pc_classes, num_points, pc_channels

    def destroy(self, reason='destroyed'):
        """ach_destroy: frees the weight and activation arenas now (the handle is unusable afterwards: every call raises, naming `reason`)."""
        if getattr(self, 'h', None) and self.h.value:
            self.L.ach_destroy(self.h)
            self.h = ctypes.c_void_p()
            self.batch = 0
            self._dead = reason

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0 and getattr(self, '_dead', None):
            raise RuntimeError(f'achelous_amd: this engine was {self._dead}')
        if rc != 0:
            msg = (self.L.ach_last_error(self.h) or b'').decode()
            raise _ERRORS.get(rc, RuntimeError)(msg)

    # ---------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """Reference-keyed state_dict (achelous.py:171) -> the handle's host copy of the weights; plan() folds and packs them on the device."""
        keep, descs = [], []
        for k, v in state_dict.items():
            if not torch.is_floating_point(v):
                continue                                   # BatchNorm num_batches_tracked
            t = v.detach().to(device='cpu', dtype=torch.float32).contiguous()
            if t.dim() > 4:
                raise ValueError(f'{k}: rank {t.dim()} tensor')
            keep.append((k.encode(), t))
        arr = (AchTensorDesc * len(keep))()
        for i, (name, t) in enumerate(keep):
            arr[i].name = name
            arr[i].data = t.data_ptr()
            arr[i].ndim = t.dim()
            for d in range(t.dim()):
                arr[i].shape[d] = t.shape[d]
        self._check(self.L.ach_load_weights(self.h, arr, len(keep)))
        self.batch = 0

    def set_option(self, key, value):
        self._check(self.L.ach_set_option(self.h, key.encode(), int(value)))
        self.batch = 0
        if key == 'io_bf16' and self.dtype == DTYPE_F16:
            self.torch_dtype = torch.bfloat16 if int(value) else torch.float16

    def get_option(self, key):
        """the stored (normalised) value of an option"""
        v = ctypes.c_int32()
        self._check(self.L.ach_get_option(self.h, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def plan(self, batch):
        self._check(self.L.ach_plan(self.h, int(batch)))
        self.batch = int(batch)

    def arena_bytes(self):
        return int(self.L.ach_arena_bytes(self.h))

    def launches(self):
        return int(self.L.ach_plan_launches(self.h))

    def forward(self, image, radar, points, outs, stream=0):
        det3, det4, det5, se, lane, pc = outs
        self._check(self.L.ach_forward(self.h, _ptr(image), _ptr(radar), _ptr(points), _ptr(det3), _ptr(det4), _ptr(det5),
                                       _ptr(se), _ptr(lane), _ptr(pc), ctypes.c_void_p(stream)))

    def forward_detect(self, image, radar, points, outs, decoded, conf, iou, max_det, rows, idx, count, workspace, stream=0):
        """forward + decode + NMS; decode / NMS ride the detection-branch stream behind the head (include/achelous.h)."""
        det3, det4, det5, se, lane, pc = outs
        self._check(self.L.ach_forward_detect(self.h, _ptr(image), _ptr(radar), _ptr(points), _ptr(det3), _ptr(det4), _ptr(det5),
                                              _ptr(se), _ptr(lane), _ptr(pc), _ptr(decoded), float(conf), float(iou), int(max_det),
                                              _ptr(rows), _ptr(idx), _ptr(count), _ptr(workspace), ctypes.c_void_p(stream)))

    def join(self, stream=0):
        """Pipelined mode: make `stream` wait for the oldest forward that has not been joined yet."""
        self._check(self.L.ach_join(self.h, ctypes.c_void_p(stream)))

    def forwards_in_flight(self):
        return int(self.L.ach_forwards_in_flight(self.h))

    def count_saturated(self, stream=0):
        """fp16-storage engine: elements of the plan's activation tensors that are saturated (+-65504) or non-finite after the forwards
        enqueued on `stream` so far (synchronises the stream); always 0 for the fp32 / bf16 engines (include/achelous.h)."""
        n = ctypes.c_uint64(0)
        self._check(self.L.ach_count_saturated(self.h, ctypes.c_void_p(stream), ctypes.byref(n)))
        return int(n.value)

    def op_table(self):
        """[(name, algorithmic bytes, flops)] of every launch in the plan."""
        return [(self.L.ach_op_name(self.h, i).decode(), self.L.ach_op_bytes(self.h, i), self.L.ach_op_flops(self.h, i))
                for i in range(self.launches())]

    def op_table_full(self):
        """[{name, bytes (real channels), layout_bytes (stored pitches), flops, stream}] of every launch in the plan."""
        return [dict(op=self.L.ach_op_name(self.h, i).decode(), bytes=self.L.ach_op_bytes(self.h, i),
                     layout_bytes=self.L.ach_op_layout_bytes(self.h, i), flops=self.L.ach_op_flops(self.h, i),
                     stream=self.L.ach_op_stream(self.h, i)) for i in range(self.launches())]

    def op_schedule(self):
        """[{op, stream, wait, signal, xwait, xsignal}] of every launch in the plan: the stream it runs on and the events it waits for / records,
        as the bit masks of ach_op_sync (include/achelous.h)."""
        out = []
        for i in range(self.launches()):
            m = [ctypes.c_int() for _ in range(4)]
            if self.L.ach_op_sync(self.h, i, *map(ctypes.byref, m)) != 0:
                raise IndexError(f'launch {i} is outside the plan')
            out.append(dict(op=self.L.ach_op_name(self.h, i).decode(), stream=self.L.ach_op_stream(self.h, i),
                            wait=m[0].value, signal=m[1].value, xwait=m[2].value, xsignal=m[3].value))
        return out

    def forward_profiled(self, image, radar, points, outs, stream=0):
        """One forward with every launch bracketed by HIP events -> per-launch milliseconds."""
        n = self.launches()
        ms = (ctypes.c_float * n)()
        det3, det4, det5, se, lane, pc = outs
        self._check(self.L.ach_forward_profiled(self.h, _ptr(image), _ptr(radar), _ptr(points), _ptr(det3), _ptr(det4),
                                                _ptr(det5), _ptr(se), _ptr(lane), _ptr(pc), ctypes.c_void_p(stream),
                                                ctypes.cast(ms, ctypes.c_void_p), n))
        return list(ms)

    def bench_gemm(self, M, K, N, act=0, ln=0, residual=0, P=0, iters=20, stream=0):
        ms = ctypes.c_float()
        self._check(self.L.ach_bench_gemm(self.h, M, K, N, act, ln, residual, P, iters, ctypes.c_void_p(stream), ctypes.byref(ms)))
        return float(ms.value)

    def set_probe(self, op_index):
        self._check(self.L.ach_set_probe(self.h, int(op_index)))

    def read_probe(self):
        avg, n = ctypes.c_float(), ctypes.c_int()
        self._check(self.L.ach_read_probe(self.h, ctypes.byref(avg), ctypes.byref(n)))
        return float(avg.value), int(n.value)

    def set_probe_range(self, slot, first, last):
        self._check(self.L.ach_set_probe_range(self.h, int(slot), int(first), int(last)))

    def read_probe_slot(self, slot):
        avg, n = ctypes.c_float(), ctypes.c_int()
        self._check(self.L.ach_read_probe_slot(self.h, int(slot), ctypes.byref(avg), ctypes.byref(n)))
        return float(avg.value), int(n.value)

    def decode(self, batch, det3, det4, det5, decoded, stream=0):
        self._check(self.L.ach_decode(self.h, int(batch), _ptr(det3), _ptr(det4), _ptr(det5), _ptr(decoded),
                                      ctypes.c_void_p(stream)))

    def nms_workspace_bytes(self, batch):
        return int(self.L.ach_nms_workspace_bytes(self.h, int(batch)))

    def nms(self, batch, decoded, conf, iou, max_det, rows, idx, count, workspace, stream=0):
        self._check(self.L.ach_nms(self.h, int(batch), _ptr(decoded), float(conf), float(iou), int(max_det), _ptr(rows),
                                   _ptr(idx), _ptr(count), _ptr(workspace), ctypes.c_void_p(stream)))

    # ---- pre / post-processing
    def preprocess_radar(self, batch, channels, src, dst, stream=0):
        self._check(self.L.ach_preprocess_radar(self.h, int(batch), int(channels), _ptr(src), _ptr(dst), ctypes.c_void_p(stream)))

    def normalize_points(self, batch, n, d, src, dst, stream=0):
        self._check(self.L.ach_normalize_points(self.h, int(batch), int(n), int(d), _ptr(src), _ptr(dst), ctypes.c_void_p(stream)))

    def preprocess_image(self, batch, src, dst, stream=0):
        self._check(self.L.ach_preprocess_image(self.h, int(batch), _ptr(src), _ptr(dst), ctypes.c_void_p(stream)))

    def seg_argmax(self, batch, channels, src, dst, stream=0):
        self._check(self.L.ach_seg_argmax(self.h, int(batch), int(channels), _ptr(src), _ptr(dst), ctypes.c_void_p(stream)))

    def seg_resize_argmax(self, batch, channels, src, out_h, out_w, prob_ws, dst, stream=0):
        self._check(self.L.ach_seg_resize_argmax(self.h, int(batch), int(channels), _ptr(src), int(out_h), int(out_w), _ptr(prob_ws), _ptr(dst),
                                                 ctypes.c_void_p(stream)))

    def correct_boxes(self, batch, max_det, rows, count, image_h, image_w, letterbox, out, stream=0):
        self._check(self.L.ach_correct_boxes(self.h, int(batch), int(max_det), _ptr(rows), _ptr(count), int(image_h), int(image_w),
                                             int(bool(letterbox)), _ptr(out), ctypes.c_void_p(stream)))

    def seg_overlay_frames(self, batch, channels, se, lane, prob_se, prob_line, arena, arena_bytes, table_host, table_dev, consts_host, consts_dev,
                           palette_se_len, palette_line_len, blend_se, blend_line, use_lut, out_semantic, semantic_bytes, out_waterline, waterline_bytes,
                           out_overlay, overlay_bytes, stream=0):
        """the ragged batch's class maps and overlay in one launch behind the softmax launches (include/achelous.h); the table / constants arguments are raw
        addresses (host copy, device copy), every other pointer a tensor or None"""
        vp = ctypes.c_void_p
        self._check(self.L.ach_seg_overlay_frames(self.h, int(batch), int(channels), _ptr(se), _ptr(lane), _ptr(prob_se), _ptr(prob_line), _ptr(arena), int(arena_bytes),
                                                  vp(table_host), vp(table_dev), vp(consts_host), vp(consts_dev), int(palette_se_len), int(palette_line_len),
                                                  float(blend_se), float(blend_line), int(bool(use_lut)), _ptr(out_semantic), int(semantic_bytes),
                                                  _ptr(out_waterline), int(waterline_bytes), _ptr(out_overlay), int(overlay_bytes), vp(stream)))

    def correct_boxes_frames(self, batch, max_det, rows, count, shapes_host, shapes_dev, letterbox, out, stream=0):
        """`correct_boxes` with a (H, W) per frame: int32 [batch, 2], host copy and device copy (raw addresses)"""
        self._check(self.L.ach_correct_boxes_frames(self.h, int(batch), int(max_det), _ptr(rows), _ptr(count), ctypes.c_void_p(shapes_host), ctypes.c_void_p(shapes_dev),
                                                    int(bool(letterbox)), _ptr(out), ctypes.c_void_p(stream)))

    @staticmethod
    def heatmap_frames(lib, det_kind, resolution, num_det, batch, det3, det4, det5, scores, base, base_bytes, table_host, table_dev, cmap_dev, alpha, mask, mask_bytes,
                       stats, out, out_bytes, stream=0):
        """the heat-map mode of a ragged batch in three launches (include/achelous_heatmap.h ach_heatmap_frames): stateless, so `lib` (a `NativeLibrary`) stands where the
        handle would; the table / colour map arguments are raw addresses, every other pointer a tensor or None (base, out: no colour pass)"""
        vp = ctypes.c_void_p
        rc = lib.lib.ach_heatmap_frames(int(det_kind), int(resolution), int(num_det), int(batch), _ptr(det3), _ptr(det4), _ptr(det5), _ptr(scores), _ptr(base),
                                        int(base_bytes), vp(table_host), vp(table_dev), vp(cmap_dev), float(alpha), _ptr(mask), int(mask_bytes), _ptr(stats), _ptr(out),
                                        int(out_bytes), vp(stream))
        if rc != 0:
            raise _ERRORS.get(rc, RuntimeError)((lib.lib.ach_last_error(None) or b'ach_heatmap_frames failed').decode())

    # ---------------------------------------------------------------------------------------------------
    def tap_names(self):
        return [self.L.ach_tap_name(self.h, i).decode() for i in range(self.L.ach_tap_count(self.h))]

    def read_tap(self, name):
        shape = (ctypes.c_int64 * 4)()
        ndim = ctypes.c_int32()
        self._check(self.L.ach_tap_shape(self.h, name.encode(), shape, ctypes.byref(ndim)))
        dims = [int(shape[i]) for i in range(ndim.value)]
        out = torch.empty(dims, dtype=torch.float32)
        self._check(self.L.ach_read_tap(self.h, name.encode(), ctypes.c_void_p(out.data_ptr()), out.numel()))
        return out
