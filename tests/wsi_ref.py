"""A Visium spot's patch cut out of the whole-slide image, restated in numpy: the defining arithmetic of
gnx_wsi_patch_grid_u8 (include/gridnext_hip.h, "Patch grid of a Visium array from the whole-slide image").
test_wsi_ref_host.py proves it equal to Pillow (`Image.fromarray(window).resize((P, P))`, default filter BICUBIC) and to the
reference's literal np.pad + slice, byte for byte; test_gpu_wsi_patches.py compares the kernel with Pillow itself.

The window of a spot centred at (cx, cy) with w = window size: source rows and columns [c - w//2, c - w//2 + 2 (w//2)), every
coordinate clamped to the slide (= the slice of the edge-padded slide).  The resize is pillow_ref.py's arithmetic with the
filter bound here to 'bicubic' (Pillow's default); the identity size returns a copy.  This file keeps the windows and the
Pillow oracle."""
import functools

import numpy as np

import pillow_ref
from pillow_ref import patterns  # noqa: F401

# (window, patch) pairs every check runs over: the fixture's, then a spread of ratios around the table edges
PAIRS = [(8, 8), (12, 8), (8, 12), (4, 8), (30, 8), (8, 7), (40, 37), (64, 17), (2, 8), (33, 32), (32, 33), (16, 16),
         (1, 8), (8, 1), (3, 2), (2, 3), (5, 4), (7, 9), (9, 7), (10, 8), (15, 8), (16, 8), (24, 8), (28, 8), (31, 8), (32, 8),
         (20, 16), (40, 32), (48, 12), (13, 11), (11, 13), (50, 49), (49, 50), (100, 25), (6, 24), (5, 37), (256, 64)]


coeffs = functools.partial(pillow_ref.coeffs, filter='bicubic')
ksize = functools.partial(pillow_ref.ksize, filter='bicubic')
_pass = functools.partial(pillow_ref._pass, filter='bicubic')


def resize_hwc(win, P):
    """uint8 window [h][w][3] -> [P][P][3]: horizontal pass, then vertical, on bytes; an unchanged axis is skipped."""
    if win.shape[1] != P:
        win = _pass(win, P, 1)
    if win.shape[0] != P:
        win = _pass(win, P, 0)
    return np.ascontiguousarray(win)


def window_clamped(slide, cx, cy, w):
    """Rows and columns [c - w//2, c - w//2 + 2 (w//2)) of the slide [Hs][Ws][3], every coordinate clamped to it."""
    half = w // 2
    rows = np.clip(np.arange(cy - half, cy + half), 0, slide.shape[0] - 1)
    cols = np.clip(np.arange(cx - half, cx + half), 0, slide.shape[1] - 1)
    return np.ascontiguousarray(slide[rows][:, cols])


def window_padded(slide, cx, cy, w):
    """The reference, literally (imgprocess.py:198, :217-220): pad the whole slide by w//2 with its edge, then slice."""
    half = w // 2
    img = np.pad(slide, pad_width=[(half, half), (half, half), (0, 0)], mode='edge')
    x_px, y_px = cx + half, cy + half
    return img[(y_px - half):(y_px + half), (x_px - half):(x_px + half)]


def patch(slide, cx, cy, w, P):
    """The spot's patch, planar uint8 [3][P][P]."""
    return np.ascontiguousarray(resize_hwc(window_clamped(slide, cx, cy, w), P).transpose(2, 0, 1))


def pillow_patch(slide, cx, cy, w, P):
    """The oracle: the clamped window through Pillow's default resize, planar."""
    from PIL import Image
    win = window_clamped(slide, cx, cy, w)
    return np.ascontiguousarray(np.array(Image.fromarray(win).resize((P, P))).transpose(2, 0, 1))
