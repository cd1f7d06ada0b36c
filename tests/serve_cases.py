"""Inputs and expected values of tests/test_serve.py (the ragged serving path: achelous_amd/prepost.py seg_maps_frames / correct_boxes_frames / detect_frames,
csrc/k_serve.h).  The class-map side of the truth is oracle/prepost.py; the palette / PIL side — what the reference's detect_image does with the two class maps
(achelous.py:297, 324-345) — lives here: numpy palette lookup, PIL's own Image.blend twice and ImageEnhance.Brightness."""
import json
import os

import numpy as np
from PIL import Image, ImageEnhance

from oracle import prepost as O

HERE = os.path.dirname(os.path.abspath(__file__))
R, C_SE, B = 32, 9, 10
# landscape and portrait windows, down-sampling, identity, a window one source row / column thick, widths 1, 2, 3 (narrower than a thread's four pixels) and widths
# that are no multiple of 4, a frame that spans several tiles in both directions, pitches that need padding
SHAPES = ((67, 131), (131, 67), (13, 21), (32, 32), (8, 300), (300, 8), (150, 261), (5, 3), (1, 1), (97, 2))


def palettes():
    g = json.load(open(os.path.join(HERE, 'golden', 'overlay_palettes.json')))
    return [tuple(c) for c in g['colors_seg']], [tuple(c) for c in g['colors_seg_line']]


def logits(seed=3):
    """as tests/test_prepost.py::_inputs: normal logits, two classes of frame 0 tied everywhere (first maximum wins)"""
    rng = np.random.default_rng(seed)
    se = rng.normal(0, 1, (B, C_SE, R, R)).astype(np.float32)
    se[0, 3] = se[0, 5]
    lane = rng.normal(0, 1, (B, 2, R, R)).astype(np.float32)
    return se, lane


def images(shapes=SHAPES, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def class_map_from_probabilities(prob_chw, h, w):
    """the oracle's crop + INTER_LINEAR + arg-max on probabilities [C, R, R] the kernel itself read"""
    p = np.ascontiguousarray(np.asarray(prob_chw, dtype=np.float32).transpose(1, 2, 0))
    y0, x0, nh, nw = O.letterbox_window(h, w, p.shape[0])
    return O.resize_linear(p[y0:y0 + nh, x0:x0 + nw], h, w).argmax(axis=-1).astype(np.uint8)


def overlay(image, sem, line, palette_se, palette_line, keep_classes, blend, brightness):
    """achelous.py:297, 324-345 with PIL itself"""
    sem = np.asarray(sem).astype(np.int64)
    if keep_classes is not None:
        sem = np.where(np.isin(sem, keep_classes), sem, 0)
    se_img = Image.fromarray(np.array(palette_se, np.uint8)[sem.reshape(-1)].reshape(sem.shape + (3,)))
    line_img = Image.fromarray(np.array(palette_line, np.uint8)[np.asarray(line).astype(np.int64).reshape(-1)].reshape(sem.shape + (3,)))
    out = Image.blend(Image.fromarray(image), se_img, blend[0])
    out = Image.blend(out, line_img, blend[1])
    if brightness is not None:
        out = ImageEnhance.Brightness(out).enhance(brightness)
    return np.array(out)
