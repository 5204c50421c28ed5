"""Pillow's two-pass fixed-point resampling of 8-bit images, restated in numpy once for both filters the kernels run:
'bilinear' (resize_ref.py, gnx_resize_crop_u8) and 'bicubic' (wsi_ref.py, gnx_wsi_patch_grid_u8).  Those two files bind the filter
and keep their geometry, windows and Pillow oracles; the host tests prove this arithmetic equal to Pillow bit for bit.

Per axis, all in double, in the order of Pillow's C loop, with radius 1 and the triangle for 'bilinear', 2 and the cubic:
    scale = in / out; filterscale = max(scale, 1); support = radius * filterscale; ksize = (int)ceil(support) * 2 + 1
    for every output index xx:
        center = (xx + 0.5) * scale
        xmin = max(0, (int)(center - support + 0.5)); xmax = min(in, (int)(center + support + 0.5))
        w[x] = filter((x + xmin - center + 0.5) * (1 / filterscale)) for x in [0, xmax - xmin), summed sequentially, each
        divided by the sum; k[x] = (int)(0.5 + w[x] * 2^22), or (int)(-0.5 + w[x] * 2^22) for a negative weight (bicubic only)
    triangle(x) = 1 - |x| below 1, else 0
    bicubic(x), a = -0.5: ((a + 2) |x| - (a + 3)) |x|^2 + 1 below 1, (((|x| - 5) |x| + 8) |x| - 4) a below 2, else 0
A pass is clip((2^21 + sum pixel * k) >> 22, 0, 255) (an arithmetic shift: with bicubic the sum can be negative).  The horizontal
pass runs first and writes bytes, the vertical pass runs on those bytes; a pass whose size does not change is skipped.  The
tables are written with scalar loops on purpose: `gridnext_amd.transforms.axis_tables` is the vectorised form and is checked
against this one."""
import math

import numpy as np

PRECISION_BITS = 22


def triangle(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


# filter -> (kernel, radius, the least value the 32-bit accumulator of a pass may take: bilinear weights are never negative)
FILTERS = {'bilinear': (triangle, 1.0, 0), 'bicubic': (bicubic, 2.0, -2 ** 31)}


def ksize(n_in, n_out, filter):
    return int(math.ceil(FILTERS[filter][1] * max(n_in / n_out, 1.0))) * 2 + 1


def coeffs(n_in, n_out, filter):
    """(k int64 [n_out][ksize], bounds [n_out][2] = {xmin, taps}) of one axis."""
    kernel, radius, _ = FILTERS[filter]
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = radius * filterscale
    ks = ksize(n_in, n_out, filter)
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
            v = kernel((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        for x in range(xmax):
            if ww != 0.0:
                w[x] /= ww
            kk[xx, x] = int((-0.5 if w[x] < 0 else 0.5) + w[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(img, n_out, axis, filter):
    """One resampling pass of uint8 `img` along `axis` (the other axes ride along)."""
    img = np.moveaxis(img, axis, -1)
    kk, bounds = coeffs(img.shape[-1], n_out, filter)
    out = np.empty(img.shape[:-1] + (n_out,), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., xmin:xmin + n] * kk[xx, :n]).sum(-1)
        assert acc.max(initial=0) < 2 ** 31 and acc.min(initial=0) >= FILTERS[filter][2]      # the accumulator fits 32 bits
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def patterns(shape, seed=0):
    """The byte patterns every geometry is tried with: random, 0/255 extremes, all 0, all 255."""
    rng = np.random.default_rng(seed)
    return {'random': rng.integers(0, 256, shape, dtype=np.uint8),
            'extremes': (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8),
            'zeros': np.zeros(shape, dtype=np.uint8),
            'full': np.full(shape, 255, dtype=np.uint8)}
