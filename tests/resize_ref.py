"""Pillow's BILINEAR resize of 8-bit images, restated in numpy: the defining arithmetic of gnx_resize_crop_u8
(include/gridnext_hip.h, "Resize + CenterCrop of uint8 patches").  test_resize_ref_host.py proves it equal to Pillow bit for
bit; test_gpu_resize.py compares the kernel with Pillow itself and uses this file for geometry only.

Per axis, all in double, in the order of Pillow's C loop:
    scale = in / out; filterscale = max(scale, 1); support = 1.0 * filterscale; ksize = (int)ceil(support) * 2 + 1
    for every output index xx:
        center = (xx + 0.5) * scale
        xmin = max(0, (int)(center - support + 0.5)); xmax = min(in, (int)(center + support + 0.5))
        w[x] = triangle((x + xmin - center + 0.5) * (1 / filterscale)) for x in [0, xmax - xmin), summed sequentially,
        each divided by the sum; k[x] = (int)(0.5 + w[x] * 2^22)
A pass is clip((2^21 + sum pixel * k) >> 22, 0, 255).  The horizontal pass runs first and writes bytes, the vertical pass
runs on those bytes; a pass whose size does not change is skipped.  The tables are written with scalar loops on purpose:
`gridnext_amd.transforms.axis_tables` is the vectorised form and is checked against this one."""
import math

import numpy as np

PRECISION_BITS = 22


def ksize(n_in, n_out):
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def coeffs(n_in, n_out):
    """(k int64 [n_out][ksize], bounds [n_out][2] = {xmin, taps}) of one axis."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
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
            v = (x + xmin - center + 0.5) * ss
            v = -v if v < 0.0 else v
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            if ww != 0.0:
                w[x] /= ww
            kk[xx, x] = int(0.5 + w[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(img, n_out, axis):
    """One resampling pass of uint8 `img` along `axis` (any leading axes ride along)."""
    img = np.moveaxis(img, axis, -1)
    kk, bounds = coeffs(img.shape[-1], n_out)
    out = np.empty(img.shape[:-1] + (n_out,), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., xmin:xmin + n] * kk[xx, :n]).sum(-1)
        assert acc.max(initial=0) < 2 ** 31 and acc.min(initial=0) >= 0      # the accumulator fits 32 bits
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def resize_u8(img, Hr, Wr):
    """uint8 [..., H, W] -> [..., Hr, Wr]: horizontal pass, then vertical; an unchanged axis is skipped."""
    if img.shape[-1] != Wr:
        img = _pass(img, Wr, -1)
    if img.shape[-2] != Hr:
        img = _pass(img, Hr, -2)
    return img


def resized_shape(H, W, size):
    """torchvision's Resize(size): an int scales the short edge; (h, w) as given; None: unchanged."""
    if size is None:
        return H, W
    if isinstance(size, (tuple, list)):
        return int(size[0]), int(size[1])
    if W <= H:
        return (H, W) if W == size else (int(size * H / W), size)
    return (H, W) if H == size else (size, int(size * W / H))


def center_window(H, W, size):
    """torchvision's CenterCrop(size) offsets: (top, left, h, w); None: the whole image."""
    if size is None:
        return 0, 0, H, W
    h, w = (size, size) if isinstance(size, int) else size
    return int(round((H - h) / 2.0)), int(round((W - w) / 2.0)), h, w


def resize_crop_u8(x, resize, crop):
    """The reference transform on uint8 patches [N, 3, H0, W0] in numpy: resize, then centre crop."""
    Hr, Wr = resized_shape(x.shape[-2], x.shape[-1], resize)
    y = resize_u8(x, Hr, Wr)
    top, left, h, w = center_window(Hr, Wr, crop)
    return np.ascontiguousarray(y[..., top:top + h, left:left + w])


def pillow_resize_crop(x, resize, crop):
    """The oracle: Pillow itself on every patch of x [N, 3, H0, W0] (what torchvision's Resize / CenterCrop call for the PIL
    images the datasets hand them)."""
    from PIL import Image
    Hr, Wr = resized_shape(x.shape[-2], x.shape[-1], resize)
    top, left, h, w = center_window(Hr, Wr, crop)
    out = np.empty((x.shape[0], 3, h, w), dtype=np.uint8)
    for i in range(x.shape[0]):
        img = Image.fromarray(np.ascontiguousarray(x[i].transpose(1, 2, 0)))
        if (Hr, Wr) != tuple(x.shape[-2:]):
            img = img.resize((Wr, Hr), Image.BILINEAR)
        img = img.crop((left, top, left + w, top + h))
        out[i] = np.asarray(img).transpose(2, 0, 1)
    return out


def patterns(shape, seed=0):
    """The byte patterns every geometry is tried with: random, 0/255 extremes, all 0, all 255."""
    rng = np.random.default_rng(seed)
    return {'random': rng.integers(0, 256, shape, dtype=np.uint8),
            'extremes': (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8),
            'zeros': np.zeros(shape, dtype=np.uint8),
            'full': np.full(shape, 255, dtype=np.uint8)}
