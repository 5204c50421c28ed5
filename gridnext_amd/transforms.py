"""The tutorials' image transform, on the host and on the device.

Every image notebook of the reference builds its patch datasets with

    transforms.Compose([transforms.Resize(256), transforms.CenterCrop(224),
                        transforms.ToTensor(), transforms.Normalize(mean, std)])

from `torchvision.transforms`, which is not a dependency of this package.  The five names below are drop-ins:

    from gridnext_amd import transforms

  * on a PIL image (the host path: `PatchDataset(img_transforms=Compose([...]))` as in the reference) they compute what
    torchvision computes: `Resize` through Pillow's BILINEAR resampling (short edge to `size`, long edge to
    int(size * long / short); (h, w) is taken as given), `CenterCrop` at int(round((H - size) / 2.0)), `ToTensor` =
    `image_datasets.to_tensor`, `Normalize` = (t - mean) / std.  One stated difference: a crop larger than the image raises
    ValueError (torchvision zero-pads);
  * `Compose.device_plan()` says whether the whole transform can run on the device - steps [Resize] [CenterCrop] ToTensor
    [Normalize] in that order - as (resize, crop, norm).  A dataset with `raw_uint8=True` then only decodes (uint8 patches at
    their stored size, a quarter of the bytes over PCIe) and carries the transform as `dataset.device_transform`;
    `DenseNet.set_input_transform(compose)` makes the classifier run it: `gnx_resize_crop_u8` / `gnx_resize_crop_u8_f32`
    (csrc/resize.hip) in front of its stem, the same bytes as Pillow's bit for bit.

`axis_tables` builds the coefficient tables of Pillow's fixed-point resampling (host, double); `device_axis_tables` keeps them
on the device for the kernels that read them (this file's and `imgprocess`'s); `resize_crop` is the device call.  There is no
CPU fallback for `resize_crop`.
"""
import math

import numpy as np
import torch
from PIL import Image

from . import _lib as L

PRECISION_BITS = 22          # Pillow's fixed-point weights for 8-bit channels
MAX_KSIZE = 17               # what the kernels take: bilinear reductions up to 8x per axis, bicubic ones up to 4x

_BILINEAR = (Image.BILINEAR, 'bilinear')


# ---------------------------------------------------------------------------------------------- geometry (host arithmetic)
def _pair(size, what):
    if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
        return int(size), int(size)
    if isinstance(size, (tuple, list)) and len(size) == 1:
        return int(size[0]), int(size[0])
    if isinstance(size, (tuple, list)) and len(size) == 2:
        return int(size[0]), int(size[1])
    raise TypeError("%s: size must be an int or (h, w), got %r" % (what, size))


def resized_shape(H, W, size):
    """(Hr, Wr) of torchvision's Resize(size) for an H x W image: an int scales the short edge to `size` and the long edge
    to int(size * long / short); (h, w) is the shape itself; None: unchanged."""
    if size is None:
        return H, W
    if isinstance(size, (tuple, list)) and len(size) == 2:
        return int(size[0]), int(size[1])
    size = _pair(size, 'Resize')[0]
    if size <= 0:
        raise ValueError("Resize: size must be positive, got %d" % size)
    if W <= H:
        return (H, W) if W == size else (int(size * H / W), size)
    return (H, W) if H == size else (size, int(size * W / H))


def crop_window(H, W, size):
    """(top, left, h, w) of torchvision's CenterCrop(size) on an H x W image; None: the whole image.  A crop larger than
    the image raises ValueError (torchvision pads with zeros instead)."""
    if size is None:
        return 0, 0, H, W
    h, w = _pair(size, 'CenterCrop')
    if h <= 0 or w <= 0:
        raise ValueError("CenterCrop: size must be positive, got %r" % (size,))
    if h > H or w > W:
        raise ValueError("CenterCrop(%r) is larger than the %d x %d image (zero-padding crops are not supported)"
                         % (size, H, W))
    return int(round((H - h) / 2.0)), int(round((W - w) / 2.0)), h, w


def transform_geometry(H0, W0, resize, crop):
    """(Hr, Wr, top, left, Ph, Pw): stored H0 x W0 patches are resized to (Hr, Wr), then the window is cut."""
    Hr, Wr = resized_shape(H0, W0, resize)
    top, left, Ph, Pw = crop_window(Hr, Wr, crop)
    return Hr, Wr, top, left, Ph, Pw


def _check_filter(filter):
    if filter not in ('bilinear', 'bicubic'):
        raise ValueError("filter must be 'bilinear' or 'bicubic', got %r" % (filter,))
    return 1.0 if filter == 'bilinear' else 2.0


def axis_ksize(n_in, n_out, filter='bilinear'):
    """Taps per output index of one axis: Pillow's (int)ceil(support) * 2 + 1, support = max(in / out, 1) for 'bilinear' and
    twice that for 'bicubic'; an axis whose size does not change is not resampled: 1 (the identity table)."""
    radius = _check_filter(filter)
    if n_in == n_out:
        return 1
    return int(math.ceil(radius * max(n_in / n_out, 1.0))) * 2 + 1


def _bicubic(x):
    """Pillow's bicubic kernel (a = -0.5) of |x| as it is written there, operation for operation."""
    a = -0.5
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def axis_tables(n_in, n_out, lo=0, n=None, filter='bilinear'):
    """(coef int32 [n][ksize], bounds int32 [n][2] = {first tap, taps}) of Pillow's BILINEAR (or, filter='bicubic', BICUBIC)
    resampling of an axis from `n_in` to `n_out` samples, for the output indices [lo, lo + n): double arithmetic in Pillow's
    operation order, each normalised weight rounded to (int)(0.5 + w * 2^22), a negative one (bicubic has them) to
    (int)(-0.5 + w * 2^22).  n_in == n_out: one tap of 2^22 at the index itself."""
    radius = _check_filter(filter)
    n = n_out - lo if n is None else n
    if lo < 0 or n < 0 or lo + n > n_out:
        raise ValueError("window [%d, %d) outside the %d resized samples" % (lo, lo + n, n_out))
    idx = np.arange(lo, lo + n, dtype=np.int64)
    ks = axis_ksize(n_in, n_out, filter)
    if n_in == n_out:
        return (np.full((n, 1), 1 << PRECISION_BITS, dtype=np.int32),
                np.stack([idx, np.ones_like(idx)], 1).astype(np.int32))
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = radius * filterscale
    ss = 1.0 / filterscale
    center = (idx.astype(np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    cnt = xmax - xmin
    k = np.arange(ks, dtype=np.int64)[None, :]
    w = np.abs((k + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((w < radius) & (k < cnt[:, None]), 1.0 - w if filter == 'bilinear' else _bicubic(w), 0.0)
    ww = np.zeros(n, dtype=np.float64)
    for j in range(ks):                                                       # the sequential sum of the C loop
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    half = np.where(w < 0.0, -0.5, 0.5)
    coef = (half + w * float(1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)
    coef[k >= cnt[:, None]] = 0
    return np.ascontiguousarray(coef), np.stack([xmin, cnt], 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------- the device call
_TABLES = {}         # (n_in, n_out, lo, n, filter, device) -> (coef, bnd) device int32


def device_axis_tables(n_in, n_out, lo, n, filter, dev):
    """`axis_tables` of one axis as int32 tensors on `dev`, kept for the next call (64 entries, then all are dropped)."""
    key = (n_in, n_out, lo, n, filter, str(dev))
    hit = _TABLES.get(key)
    if hit is None:
        if len(_TABLES) >= 64:
            _TABLES.clear()
        hit = _TABLES[key] = tuple(torch.from_numpy(a).to(dev) for a in axis_tables(n_in, n_out, lo, n, filter))
    return hit


def resize_crop(x, resize=None, crop=None, norm=None, out_float=False):
    """Resize + CenterCrop of uint8 patches x (N, 3, H0, W0) on their HIP device -> (N, 3, Ph, Pw): uint8, Pillow's bytes
    bit for bit (gnx_resize_crop_u8), or with `out_float` ToTensor (+ Normalize: `norm` = the device vector
    {mean[3], std[3], 1/std[3]}) of those bytes as float32 (gnx_resize_crop_u8_f32).  `x` may be any view whose patches lie
    back to back (any base alignment); other views are copied first."""
    if x.dtype != torch.uint8:
        raise ValueError("resize_crop is defined on uint8 patches (got %s)" % x.dtype)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("expected RGB patches (N, 3, H, W), got %s" % (tuple(x.shape),))
    if not x.is_cuda:
        raise RuntimeError("resize_crop runs on a HIP device only (input is on %s); there is no CPU fallback" % x.device)
    x = x.contiguous()
    N, _, H0, W0 = x.shape
    geom = transform_geometry(H0, W0, resize, crop)
    Hr, Wr, top, left, Ph, Pw = geom
    out = torch.empty((N, 3, Ph, Pw), device=x.device, dtype=torch.float32 if out_float else torch.uint8)
    if max(axis_ksize(H0, Hr), axis_ksize(W0, Wr)) > MAX_KSIZE or N == 0:
        tabs = (None,) * 4                     # (declined by the entry point before it reads a table)
    else:
        hc, hb = device_axis_tables(W0, Wr, left, Pw, 'bilinear', x.device)
        vc, vb = device_axis_tables(H0, Hr, top, Ph, 'bilinear', x.device)
        assert hc.shape[1] == L.query('gnx_resize_ksize', W0, Wr) and vc.shape[1] == L.query('gnx_resize_ksize', H0, Hr)
        tabs = tuple(L.ptr(t, torch.int32) for t in (hc, hb, vc, vb))
    args = (x.data_ptr(), out.data_ptr(), N, H0, W0, Hr, Wr, top, left, Ph, Pw) + tabs
    if out_float:
        L.call('gnx_resize_crop_u8_f32', *args, L.ptr(norm), L.stream())
    else:
        L.call('gnx_resize_crop_u8', *args, L.stream())
    return out


# ---------------------------------------------------------------------------------------------- the five names
def _pil(img, who):
    if not isinstance(img, Image.Image):
        raise TypeError("%s takes a PIL image (got %s); on the device it runs on uint8 patches" % (who, type(img).__name__))
    return img


class Resize:
    def __init__(self, size, interpolation=Image.BILINEAR):
        name = getattr(interpolation, 'value', interpolation)
        if name not in _BILINEAR and interpolation not in _BILINEAR:
            raise NotImplementedError("Resize: only BILINEAR interpolation is implemented (got %r)" % (interpolation,))
        if not (isinstance(size, (tuple, list)) and len(size) == 2):
            size = _pair(size, 'Resize')[0]
        else:
            size = (int(size[0]), int(size[1]))
        resized_shape(1, 1, size)              # (validates the size)
        self.size = size

    def __call__(self, img):
        W, H = _pil(img, 'Resize').size
        Hr, Wr = resized_shape(H, W, self.size)
        return img if (Hr, Wr) == (H, W) else img.resize((Wr, Hr), Image.BILINEAR)

    def __repr__(self):
        return "Resize(size=%r, interpolation=bilinear)" % (self.size,)


class CenterCrop:
    def __init__(self, size):
        self.size = _pair(size, 'CenterCrop')
        crop_window(self.size[0], self.size[1], self.size)      # (validates the size)

    def __call__(self, img):
        W, H = _pil(img, 'CenterCrop').size
        top, left, h, w = crop_window(H, W, self.size)
        return img.crop((left, top, left + w, top + h))

    def __repr__(self):
        return "CenterCrop(size=%r)" % (self.size,)


class ToTensor:
    def __call__(self, img):
        from .image_datasets import to_tensor
        return to_tensor(img)

    def __repr__(self):
        return "ToTensor()"


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if any(v == 0 for v in self.std):
            raise ValueError("Normalize: std must be non-zero")

    def __call__(self, t):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise TypeError("Normalize takes a float tensor (C, H, W): put ToTensor in front of it")
        mean = torch.tensor(self.mean, dtype=t.dtype, device=t.device).reshape(-1, 1, 1)
        std = torch.tensor(self.std, dtype=t.dtype, device=t.device).reshape(-1, 1, 1)
        return (t - mean) / std

    def __repr__(self):
        return "Normalize(mean=%r, std=%r)" % (self.mean, self.std)


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img

    def _plan(self):
        """(plan, None) or (None, the reason there is none: it names the step)."""
        steps = list(self.transforms)
        resize = crop = norm = None
        i = 0
        if i < len(steps) and isinstance(steps[i], Resize):
            resize, i = steps[i].size, i + 1
        if i < len(steps) and isinstance(steps[i], CenterCrop):
            crop = steps[i].size
            crop, i = (crop[0] if crop[0] == crop[1] else crop), i + 1
        if i >= len(steps) or not isinstance(steps[i], ToTensor):
            got = repr(steps[i]) if i < len(steps) else 'the end of the transform'
            return None, "step %d: expected ToTensor() after [Resize] [CenterCrop], found %s" % (i, got)
        i += 1
        if i < len(steps) and isinstance(steps[i], Normalize):
            if len(steps[i].mean) != 3 or len(steps[i].std) != 3:
                return None, "step %d: %r needs three channels" % (i, steps[i])
            norm, i = (steps[i].mean, steps[i].std), i + 1
        if i < len(steps):
            return None, "step %d: %r cannot follow ToTensor() [Normalize] on the device" % (i, steps[i])
        return (resize, crop, norm), None

    def device_plan(self):
        """(resize, crop, norm) when the steps are [Resize] [CenterCrop] ToTensor [Normalize] in that order - resize: int,
        (h, w) or None; crop: int, (h, w) or None; norm: (mean[3], std[3]) or None - else None."""
        return self._plan()[0]

    def device_plan_refusal(self):
        """Why `device_plan()` is None (names the step), or None."""
        return self._plan()[1]

    def __repr__(self):
        return "Compose([%s])" % ", ".join(repr(t) for t in self.transforms)
