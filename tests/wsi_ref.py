"""A Visium spot's patch cut out of the whole-slide image, restated in numpy: the defining arithmetic of
gnx_wsi_patch_grid_u8 (include/gridnext_hip.h, "Patch grid of a Visium array from the whole-slide image").
test_wsi_ref_host.py proves it equal to Pillow (`Image.fromarray(window).resize((P, P))`, default filter BICUBIC) and to the
reference's literal np.pad + slice, byte for byte; test_gpu_wsi_patches.py compares the kernel with Pillow itself.

The window of a spot centred at (cx, cy) with w = window size: source rows and columns [c - w//2, c - w//2 + 2 (w//2)), every
coordinate clamped to the slide (= the slice of the edge-padded slide).  The resize, per axis, all in double, in the order of
Pillow's C loop:
    scale = in / out; filterscale = max(scale, 1); support = 2.0 * filterscale; ksize = (int)ceil(support) * 2 + 1
    for every output index xx:
        center = (xx + 0.5) * scale
        xmin = max(0, (int)(center - support + 0.5)); xmax = min(in, (int)(center + support + 0.5))
        w[x] = bicubic((x + xmin - center + 0.5) * (1 / filterscale)) for x in [0, xmax - xmin), summed sequentially, each
        divided by the sum; k[x] = (int)(0.5 + w[x] * 2^22), or (int)(-0.5 + w[x] * 2^22) for a negative weight
    bicubic(x), a = -0.5: ((a + 2) |x| - (a + 3)) |x|^2 + 1 below 1, (((|x| - 5) |x| + 8) |x| - 4) a below 2, else 0
A pass is clip((2^21 + sum pixel * k) >> 22, 0, 255) (an arithmetic shift: the sum can be negative).  The horizontal pass runs
first and writes bytes, the vertical pass runs on those bytes; the identity size returns a copy.  Scalar loops on purpose:
`gridnext_amd.transforms.axis_tables(..., filter='bicubic')` is the vectorised form and is checked against this one."""
import math

import numpy as np

PRECISION_BITS = 22

# (window, patch) pairs every check runs over: the fixture's, then a spread of ratios around the table edges
PAIRS = [(8, 8), (12, 8), (8, 12), (4, 8), (30, 8), (8, 7), (40, 37), (64, 17), (2, 8), (33, 32), (32, 33), (16, 16),
         (1, 8), (8, 1), (3, 2), (2, 3), (5, 4), (7, 9), (9, 7), (10, 8), (15, 8), (16, 8), (24, 8), (28, 8), (31, 8), (32, 8),
         (20, 16), (40, 32), (48, 12), (13, 11), (11, 13), (50, 49), (49, 50), (100, 25), (6, 24), (5, 37), (256, 64)]


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize(n_in, n_out):
    return int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def coeffs(n_in, n_out):
    """(k int64 [n_out][ksize], bounds [n_out][2] = {xmin, taps}) of one axis."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ks = ksize(n_in, n_out)
    ss = 1.0 / filterscale
    kk = np.zeros((n_out, ks), dtype=np.int64)
    bounds = np.zeros((n_out, 2), dtype=np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        xmax -= xmin
        w, ww = [], 0.0
        for x in range(xmax):
            v = bicubic((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        for x in range(xmax):
            if ww != 0.0:
                w[x] /= ww
            kk[xx, x] = int((-0.5 if w[x] < 0 else 0.5) + w[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(img, n_out, axis):
    """One resampling pass of uint8 `img` along `axis` (the other axes ride along)."""
    img = np.moveaxis(img, axis, -1)
    kk, bounds = coeffs(img.shape[-1], n_out)
    out = np.empty(img.shape[:-1] + (n_out,), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., xmin:xmin + n] * kk[xx, :n]).sum(-1)
        assert acc.max(initial=0) < 2 ** 31 and acc.min(initial=0) >= -2 ** 31      # the accumulator fits 32 bits
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


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


def patterns(shape, seed=0):
    """The byte patterns every geometry is tried with: random, 0/255 extremes, all 0, all 255."""
    rng = np.random.default_rng(seed)
    return {'random': rng.integers(0, 256, shape, dtype=np.uint8),
            'extremes': (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8),
            'zeros': np.zeros(shape, dtype=np.uint8),
            'full': np.full(shape, 255, dtype=np.uint8)}
