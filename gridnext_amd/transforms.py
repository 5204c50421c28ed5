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

Train-time augmentation (the second half of this file): `RandomHorizontalFlip`, `RandomVerticalFlip`, `RandomQuarterTurn` and
`ColorJitter` (brightness and contrast) are PIL steps for a host `Compose`, drawing from torch's global RNG; `Augment(steps,
seed)` draws them for a whole batch of uint8 patches and applies them in one launch (csrc/augment.hip) on a HIP device, or
through torch ops on the CPU - the same bytes.  `Compose.device_plan()` does not know these steps: device use goes through
`Augment` (the slide datasets' `augment=`).  `SaturationHueJitter` is the other half of torchvision's ColorJitter, a step of
its own because it is no per-channel byte map: `saturate_u8`, `rgb_to_hsv_u8`, `hsv_to_rgb_u8` restate Pillow's arithmetic
in numpy, and with the step an `Augment`'s one launch is the three-plane form of the same kernel.
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


# ---------------------------------------------------------------------------------------------- train-time augmentation
# A geometric step is an element of the symmetry group of the square, written as code = 4 f + r:
#     out = rot90^r(fliplr^f(x)) = torch.rot90(x.flip(-1) if f else x, r, (-2, -1)).
# In Pillow's Image.transpose (checked against Pillow 12.2): 1, 2, 3 = ROTATE_90, ROTATE_180, ROTATE_270; 4 = FLIP_LEFT_RIGHT;
# 5 = TRANSPOSE; 6 = FLIP_TOP_BOTTOM; 7 = TRANSVERSE.
_T = Image.Transpose if hasattr(Image, 'Transpose') else Image
PIL_TRANSPOSE = (None, _T.ROTATE_90, _T.ROTATE_180, _T.ROTATE_270, _T.FLIP_LEFT_RIGHT, _T.TRANSPOSE, _T.FLIP_TOP_BOTTOM,
                 _T.TRANSVERSE)
CODE_HFLIP, CODE_VFLIP = 4, 6


def _compose_table():
    """D4[c1][c2] = the code of 'c1, then c2'.  fliplr . rot90 = rot90^-1 . fliplr, so R^r2 F^f2 R^r1 F^f1 =
    R^(r2 + r1) F^f1 without f2 and R^(r2 - r1) F^(1 - f1) with it."""
    t = np.zeros((8, 8), dtype=np.uint8)
    for c1 in range(8):
        for c2 in range(8):
            f1, r1, f2, r2 = c1 >> 2, c1 & 3, c2 >> 2, c2 & 3
            t[c1, c2] = 4 * (f1 ^ f2) + (r2 + (-r1 if f2 else r1)) % 4
    return t


D4 = _compose_table()


def _pil_code(img, code, who):
    code = int(code) & 7
    return _pil(img, who) if code == 0 else _pil(img, who).transpose(PIL_TRANSPOSE[code])


class RandomHorizontalFlip:
    """FLIP_LEFT_RIGHT with probability p.  draw(n): the codes (0 or 4) of n patches, one torch.rand(n, float64) < p."""
    code = CODE_HFLIP

    def __init__(self, p=0.5):
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError("%s: p must lie in [0, 1], got %r" % (type(self).__name__, p))
        self.p = float(p)

    def draw(self, n, generator=None):
        return (torch.rand(n, dtype=torch.float64, generator=generator) < self.p).to(torch.uint8) * self.code

    def __call__(self, img):
        return _pil_code(img, self.draw(1)[0], type(self).__name__)

    def __repr__(self):
        return "%s(p=%r)" % (type(self).__name__, self.p)


class RandomVerticalFlip(RandomHorizontalFlip):
    """FLIP_TOP_BOTTOM with probability p (codes 0 or 6)."""
    code = CODE_VFLIP


class RandomQuarterTurn:
    """ROTATE_90 r times, r uniform in 0..3.  draw(n): one torch.randint(0, 4, (n,))."""

    def draw(self, n, generator=None):
        return torch.randint(0, 4, (n,), generator=generator).to(torch.uint8)

    def __call__(self, img):
        return _pil_code(img, self.draw(1)[0], 'RandomQuarterTurn')

    def __repr__(self):
        return "RandomQuarterTurn()"


def _jitter_range(value, name, centre=1.0, who='ColorJitter'):
    """torchvision's rule: a float b gives [max(0, 1 - b), 1 + b]; a pair is taken as given."""
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError("%s: %s must be a number or a (min, max) pair, got %r" % (who, name, value))
        lo, hi = float(value[0]), float(value[1])
    else:
        if value < 0:
            raise ValueError("%s: a single %s must be non-negative, got %r" % (who, name, value))
        lo, hi = max(0.0, centre - float(value)), centre + float(value)
    if not 0.0 <= lo <= hi:
        raise ValueError("%s: %s range must satisfy 0 <= min <= max, got %r" % (who, name, (lo, hi)))
    return lo, hi


class ColorJitter:
    """Brightness and contrast jitter, the factors drawn uniformly from their ranges.  On a PIL image: ImageEnhance.Contrast,
    then ImageEnhance.Brightness, in that fixed order (stated difference: torchvision draws the order too).  saturation and
    hue are not per-channel byte maps: non-zero values raise NotImplementedError (`SaturationHueJitter` is the step for them).
    draw(n) -> float64 (n, 2) = {contrast, brightness} factors: contrast first, then brightness, each one
    lo + (hi - lo) * torch.rand(n, float64), and only for a range with lo < hi (the others are the constant, nothing is drawn)."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        for name, v, neutral in (('saturation', saturation, (1.0, 1.0)), ('hue', hue, (0.0, 0.0))):
            pair = tuple(float(q) for q in v) if isinstance(v, (tuple, list)) else None
            if (pair is None and v != 0) or (pair is not None and pair != neutral):
                raise NotImplementedError("ColorJitter: %s is not a per-channel byte map and is not implemented (got %r)"
                                          % (name, v))
        self.brightness = _jitter_range(brightness, 'brightness')
        self.contrast = _jitter_range(contrast, 'contrast')

    def needs_grey(self):
        """Whether a contrast factor other than 1 can occur: the tables then need each patch's grey mean."""
        return self.contrast != (1.0, 1.0)

    def is_identity(self):
        return self.contrast == (1.0, 1.0) and self.brightness == (1.0, 1.0)

    def draw(self, n, generator=None):
        f = torch.empty((n, 2), dtype=torch.float64)
        for col, (lo, hi) in enumerate((self.contrast, self.brightness)):
            f[:, col] = lo if lo == hi else lo + (hi - lo) * torch.rand(n, dtype=torch.float64, generator=generator)
        return f

    def __call__(self, img):
        from PIL import ImageEnhance
        fc, fb = self.draw(1)[0].tolist()
        img = _pil(img, 'ColorJitter')
        if self.contrast != (1.0, 1.0):
            img = ImageEnhance.Contrast(img).enhance(fc)
        if self.brightness != (1.0, 1.0):
            img = ImageEnhance.Brightness(img).enhance(fb)
        return img

    def __repr__(self):
        return "ColorJitter(brightness=%r, contrast=%r)" % (self.brightness, self.contrast)


def _blend_u8(m, f, i):
    """uint8: Pillow's Image.blend(m, i, f) per byte restated in float32.  m, i int arrays and f a float32 array that
    broadcast against each other."""
    t = m.astype(np.float32) + f * (i - m).astype(np.float32)                 # float32 throughout, as the C loop
    inside = (f >= 0) & (f <= 1)
    clipped = np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.float32)
    return np.where(inside, t, clipped).astype(np.int64).astype(np.uint8)     # the cast truncates


def _blend_table(m, f):
    """(n, 256) uint8: Pillow's Image.blend(constant m, identity ramp, f) restated in float32.  m int [n], f float [n]."""
    m = np.asarray(m, dtype=np.int64).reshape(-1, 1)
    f = np.asarray(f, dtype=np.float64).astype(np.float32).reshape(-1, 1)
    return _blend_u8(m, f, np.arange(256, dtype=np.int64)[None, :])


def grey_sums(x):
    """int64 [N]: per patch of uint8 x (N, 3, P, P) on the CPU the sum over pixels of Pillow's convert('L') value,
    (19595 R + 38470 G + 7471 B + 0x8000) >> 16 - what gnx_patch_grey_sum_u8 computes on the device."""
    a = (x.numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.int64)
    return ((19595 * a[:, 0] + 38470 * a[:, 1] + 7471 * a[:, 2] + 0x8000) >> 16).sum(axis=(1, 2))


def contrast_means(sums, P):
    """Pillow's ImageEnhance.Contrast mean, int(sum / P^2 + 0.5), of the grey sums."""
    return (np.asarray(sums).astype(np.float64) / float(P * P) + 0.5).astype(np.int64)


def color_tables(factors, grey_means=None):
    """(n, 3, 256) uint8 tables of ImageEnhance.Contrast(img).enhance(fc) followed by ImageEnhance.Brightness(...).enhance(fb)
    for factors float (n, 2) = {fc, fb} and the patches' grey means int [n] (None: no factor fc differs from 1).  Both are
    Image.blend(degenerate, img, f) per byte: t = float32(m) + float32(f) * float32(i - m) with m the grey mean (contrast) or 0
    (brightness); 0 <= f <= 1 truncates t, any other f gives 0 where t <= 0, 255 where t >= 255 and truncates elsewhere.  The
    result is brightness[contrast[i]], the same for the three channels."""
    factors = np.asarray(factors.numpy() if torch.is_tensor(factors) else factors, dtype=np.float64).reshape(-1, 2)
    n = len(factors)
    if grey_means is None:
        if np.any(factors[:, 0] != 1.0):
            raise ValueError("color_tables: contrast factors other than 1 need the patches' grey means")
        grey_means = np.zeros(n, dtype=np.int64)
    grey_means = np.asarray(grey_means.numpy() if torch.is_tensor(grey_means) else grey_means, dtype=np.int64).reshape(-1)
    if len(grey_means) != n:
        raise ValueError("color_tables: %d factor rows but %d grey means" % (n, len(grey_means)))
    contrast = _blend_table(grey_means, factors[:, 0])
    bright = _blend_table(np.zeros(n, dtype=np.int64), factors[:, 1])
    table = np.take_along_axis(bright, contrast.astype(np.int64), axis=1)
    return np.ascontiguousarray(np.broadcast_to(table[:, None, :], (n, 3, 256)))


# ---------------------------------------------------------------------------------------------- saturation and hue
# Pillow's arithmetic restated in numpy, rounding for rounding (checked against Pillow on all 2^24 colours by
# tests/test_augment_hs_ref_host.py): what `SaturationHueJitter` computes on CPU tensors and what csrc/augment.hip is tested
# against.  The arrays hold the three channels on their LAST axis, as np.array(pil_image) does.
def _channels(a, who):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("%s takes a uint8 array (..., 3), got %s of shape %s" % (who, a.dtype, a.shape))
    return (a[..., c].astype(np.int64) for c in range(3))


def rgb_to_hsv_u8(a):
    """Pillow's convert('HSV') of RGB bytes (..., 3) -> HSV bytes (..., 3).  maxc == minc: h = s = 0.  Otherwise, with float32
    cr = maxc - minc: s = cr / float32(maxc) and rc, gc, bc = float32(maxc - channel) / cr (float32 divisions); h = bc - gc
    (float32) where r is the maximum, else float32(2.0 + rc - bc) where g is, else float32(4.0 + gc - rc) (double sums);
    h = float32(fmod(h / 6.0 + 1.0, 1.0)) in double; the bytes are int(h * 255.0) and int(s * 255.0) (double products,
    truncated, clipped to 0..255) and v = maxc."""
    r, g, b = _channels(a, 'rgb_to_hsv_u8')
    f32, f64 = np.float32, np.float64
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    s = cr / np.where(grey, 1, maxc).astype(f32)
    rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                          (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)))
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def _round_u8(y):
    """C's round() of non-negative doubles (halves away from zero), clipped to 0..255."""
    fl = np.floor(y)
    return np.clip((fl + (y - fl >= 0.5)).astype(np.int64), 0, 255)


def hsv_to_rgb_u8(a):
    """Pillow's convert('RGB') of HSV bytes (..., 3) -> RGB bytes (..., 3).  s == 0: grey v.  Otherwise x = h * 6.0 / 255.0
    (double), i = floor(x), float32 f = x - i and fs = s / 255.0; p = round(v * (1.0 - fs)), q = round(v * (1.0 - float32(fs *
    f))), t = round(v * (1.0 - fs * (1.0 - f))) in double; i % 6 selects (r, g, b) = (v, t, p), (q, v, p), (p, v, t), (p, q, v),
    (t, p, v), (v, p, q)."""
    h, s, v = _channels(a, 'hsv_to_rgb_u8')
    f32, f64 = np.float32, np.float64
    x = h.astype(f64) * 6.0 / 255.0
    i = np.floor(x)
    f = (x - i).astype(f32)
    fs = (s.astype(f64) / 255.0).astype(f32)
    dv = v.astype(f64)
    p = _round_u8(dv * (1.0 - fs.astype(f64)))
    q = _round_u8(dv * (1.0 - (fs * f).astype(f64)))
    t = _round_u8(dv * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    i = i.astype(np.int64) % 6
    rgb = [np.choose(i, sel) for sel in ((v, q, p, p, t, v), (t, v, v, q, p, p), (p, p, t, v, v, q))]
    return np.stack([np.where(s == 0, v, c) for c in rgb], -1).astype(np.uint8)


def saturate_u8(a, f):
    """ImageEnhance.Color(img).enhance(f) of RGB bytes (..., 3): Image.blend of each pixel's grey value L = (19595 R + 38470 G
    + 7471 B + 0x8000) >> 16 with every channel, t = float32(L) + float32(f) * float32(c - L) in float32 (`_blend_table`'s
    arithmetic with the constant per pixel): truncated for 0 <= f <= 1, otherwise 0 where t <= 0, 255 where t >= 255 and
    truncated elsewhere.  f: a number, or an array that broadcasts against the pixels a[..., 0]."""
    r, g, b = _channels(a, 'saturate_u8')
    L = ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16)[..., None]
    f = np.asarray(f, dtype=np.float64).astype(np.float32)[..., None]
    return _blend_u8(L, f, np.asarray(a).astype(np.int64))


def hue_shifts(fh):
    """uint8: what torchvision's adjust_hue adds to the H bytes for hue factors fh, int(fh * 255) & 255 with int() truncating
    toward zero (-0.1 -> -25 -> 231)."""
    fh = np.asarray(fh.numpy() if torch.is_tensor(fh) else fh, dtype=np.float64)
    return ((fh * 255.0).astype(np.int64) & 255).astype(np.uint8)


def shift_hue_u8(a, shift):
    """torchvision's adjust_hue of RGB bytes (..., 3) given the uint8 `shift` (a number, or an array that broadcasts against
    the pixels): to HSV bytes, H plus shift modulo 256, back to RGB.  Lossy even at shift 0, as the Pillow calls are."""
    hsv = rgb_to_hsv_u8(a)
    hsv[..., 0] = hsv[..., 0] + np.asarray(shift).astype(np.uint8)          # uint8 sums wrap around
    return hsv_to_rgb_u8(hsv)


def _hue_range(value):
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError("SaturationHueJitter: hue must be a number or a (min, max) pair, got %r" % (value,))
        lo, hi = float(value[0]), float(value[1])
    else:
        if not 0.0 <= value <= 0.5:
            raise ValueError("SaturationHueJitter: a single hue must lie in [0, 0.5], got %r" % (value,))
        lo, hi = -float(value), float(value)
    if not -0.5 <= lo <= hi <= 0.5:
        raise ValueError("SaturationHueJitter: hue range must satisfy -0.5 <= min <= max <= 0.5, got %r" % ((lo, hi),))
    return lo + 0.0, hi                                                       # (-0.0 -> 0.0)


class SaturationHueJitter:
    """The other half of torchvision's ColorJitter: saturation and hue jitter, the factors drawn uniformly from their ranges.
    saturation: a number s gives [max(0, 1 - s), 1 + s], a pair is taken as given; hue: a number h in [0, 0.5] gives [-h, h], a
    pair must satisfy -0.5 <= min <= max <= 0.5.  A stage whose range is neutral - (1, 1) for saturation, (0, 0) for hue - is
    absent and does no work; a present hue stage always makes the HSV round trip, also when the drawn shift is 0 (the round
    trip is lossy: that is what Pillow and torchvision give).
    On a PIL image: ImageEnhance.Color(img).enhance(fs), then torchvision's adjust_hue - convert('HSV'), the H plane plus
    int(fh * 255) & 255 as uint8 with wrap-around, convert('RGB') - in that fixed order (stated difference: torchvision draws
    the order too).  On uint8 patches (`Augment`): `saturate_u8` and `shift_hue_u8`, the same bytes.
    draw(n) -> float64 (n, 2) = {fs, fh}: saturation first, then hue, each lo + (hi - lo) * torch.rand(n, float64) and only
    for a range with lo < hi (the others are the constant, nothing is drawn) - `ColorJitter`'s protocol."""

    def __init__(self, saturation=0, hue=0):
        self.saturation = _jitter_range(saturation, 'saturation', who='SaturationHueJitter')
        self.hue = _hue_range(hue)

    def has_saturation(self):
        return self.saturation != (1.0, 1.0)

    def has_hue(self):
        return self.hue != (0.0, 0.0)

    def is_identity(self):
        return not self.has_saturation() and not self.has_hue()

    def draw(self, n, generator=None):
        f = torch.empty((n, 2), dtype=torch.float64)
        for col, (lo, hi) in enumerate((self.saturation, self.hue)):
            f[:, col] = lo if lo == hi else lo + (hi - lo) * torch.rand(n, dtype=torch.float64, generator=generator)
        return f

    def __call__(self, img):
        from PIL import ImageEnhance
        fs, fh = self.draw(1)[0].tolist()
        img = _pil(img, 'SaturationHueJitter')
        if img.mode != 'RGB':
            raise ValueError("SaturationHueJitter takes an RGB image (got mode %r)" % (img.mode,))
        if self.has_saturation():
            img = ImageEnhance.Color(img).enhance(fs)
        if self.has_hue():
            h, s, v = img.convert('HSV').split()
            h = Image.fromarray(np.array(h, dtype=np.uint8) + hue_shifts(fh))         # (a uint8 plane: mode 'L')
            img = Image.merge('HSV', (h, s, v)).convert('RGB')
        return img

    def __repr__(self):
        return "SaturationHueJitter(saturation=%r, hue=%r)" % (self.saturation, self.hue)


def _norm9(norm, dev):
    """{mean[3], std[3], 1/std[3]} float32 on `dev` of a (mean, std) pair; a tensor is taken to be that vector already."""
    if norm is None:
        return None
    if torch.is_tensor(norm):
        if norm.numel() != 9 or norm.dtype != torch.float32:
            raise ValueError("norm must be the float32 vector {mean[3], std[3], 1/std[3]} or a (mean, std) pair")
        return norm.to(dev)
    sd = torch.tensor(norm[1], dtype=torch.float32)
    return torch.cat([torch.tensor(norm[0], dtype=torch.float32), sd, 1.0 / sd]).to(dev)


def _as_tensor(a, dtype, dev, what, shape):
    if a is None:
        return None
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != dtype or tuple(t.shape) != shape:
        raise ValueError("%s must be %s of shape %s, got %s of shape %s" % (what, dtype, shape, t.dtype, tuple(t.shape)))
    return t.to(dev).contiguous()


def _sat_tensor(sat, dev, N):
    """float32 [N] on `dev` of the saturation factors (any float dtype: cast as Pillow's C `float alpha` is), or None."""
    if sat is None:
        return None
    t = sat if torch.is_tensor(sat) else torch.from_numpy(np.ascontiguousarray(sat))
    if not t.is_floating_point() or tuple(t.shape) != (N,):
        raise ValueError("sat must be a float array of shape (%d,), got %s of shape %s" % (N, t.dtype, tuple(t.shape)))
    return t.to(torch.float32).to(dev).contiguous()


def augment_patches(x, codes=None, tables=None, out=None, out_rows=None, out_float=False, norm=None, sat=None, hue=None):
    """Square uint8 patches x (N, 3, P, P) -> patch k turned by codes[k] (low three bits; None: identity), its bytes mapped
    through tables[k] ((N, 3, 256) uint8; None: as they are), written to row out_rows[k] (int32; None: k) of `out`
    ((..., 3, P, P), its leading axes flattened to rows; None: a new (N, 3, P, P); rows outside it are skipped, rows not named
    keep what they hold).  out_float: ToTensor (+ Normalize: `norm` = a (mean, std) pair or the vector {mean, std, 1/std}) of
    the bytes as float32.  On a HIP tensor this is ONE launch (gnx_patch_augment_u8 / _u8_f32); on a CPU tensor the same
    result through torch.flip, torch.rot90 and a table index - the semantics the kernel is tested against.  `out` must not
    overlap `x`.
    sat (float [N], cast to float32) and hue (uint8 [N], see `hue_shifts`) add, after the tables and in this order,
    `saturate_u8(., sat[k])` and `shift_hue_u8(., hue[k])` per patch; None: the stage is absent.  With either one the HIP
    launch is gnx_patch_augment_hs_u8 / _u8_f32 (csrc/augment.hip), still one; with both None everything is as without
    the two arguments."""
    if not torch.is_tensor(x) or x.dtype != torch.uint8:
        raise ValueError("augment_patches is defined on uint8 patches (got %s)" % (x.dtype if torch.is_tensor(x) else type(x)))
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError("expected square RGB patches (N, 3, P, P), got %s" % (tuple(x.shape),))
    x = x.contiguous()
    N, P, dev = int(x.shape[0]), int(x.shape[2]), x.device
    codes = _as_tensor(codes, torch.uint8, dev, 'codes', (N,))
    tables = _as_tensor(tables, torch.uint8, dev, 'tables', (N, 3, 256))
    out_rows = _as_tensor(out_rows, torch.int32, dev, 'out_rows', (N,))
    sat = _sat_tensor(sat, dev, N)
    hue = _as_tensor(hue, torch.uint8, dev, 'hue', (N,))
    dtype = torch.float32 if out_float else torch.uint8
    if out is None:
        if out_rows is not None:
            raise ValueError("out_rows needs the `out` it indexes")
        out = torch.empty((N, 3, P, P), dtype=dtype, device=dev)      # (every row k is written)
    if out.dtype != dtype or out.device != dev or out.dim() < 4 or tuple(out.shape[-3:]) != (3, P, P) or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor (..., 3, %d, %d) on %s" % (dtype, P, P, dev))
    M = out.numel() // (3 * P * P) if P else 0
    if out_rows is None and M < N:
        raise ValueError("out holds %d patches, fewer than the %d of x" % (M, N))
    norm = _norm9(norm, dev) if out_float else None
    if x.is_cuda:
        with torch.cuda.device(dev):
            args = (x.data_ptr(), out.data_ptr(), N, P, M, L.ptr(codes, torch.uint8), L.ptr(tables, torch.uint8))
            name = 'gnx_patch_augment_u8'
            if sat is not None or hue is not None:
                args, name = args + (L.ptr(sat), L.ptr(hue, torch.uint8)), 'gnx_patch_augment_hs_u8'
            args += (L.ptr(out_rows, torch.int32),)
            if out_float:
                L.call(name + '_f32', *args, L.ptr(norm), L.stream())
            else:
                L.call(name, *args, L.stream())
        return out
    if N == 0:
        return out
    y = torch.empty_like(x)
    c8 = torch.zeros(N, dtype=torch.uint8) if codes is None else codes & 7
    for code in range(8):
        idx = torch.nonzero(c8 == code).reshape(-1)
        if len(idx):
            sel = x[idx]
            y[idx] = torch.rot90(sel.flip(-1) if code & 4 else sel, code & 3, (-2, -1))
    if tables is not None:
        y = torch.gather(tables, 2, y.reshape(N, 3, P * P).long()).reshape(N, 3, P, P)
    if sat is not None or hue is not None:
        a = y.permute(0, 2, 3, 1).numpy()                                     # (N, P, P, 3), as the restatement takes it
        if sat is not None:
            a = saturate_u8(a, sat.numpy().reshape(N, 1, 1))
        if hue is not None:
            a = shift_hue_u8(a, hue.numpy().reshape(N, 1, 1))
        y = torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()
    if out_float:
        y = y.float().div(255)
        if norm is not None:
            y = (y - norm[0:3].reshape(1, 3, 1, 1)) / norm[3:6].reshape(1, 3, 1, 1)
    rows = torch.arange(N) if out_rows is None else out_rows.long()
    keep = (rows >= 0) & (rows < M)
    out.view(M, 3, P, P)[rows[keep]] = y[keep]
    return out


class Augment:
    """A batch of random flips, quarter turns, one brightness / contrast jitter and one saturation / hue jitter for uint8
    patches, on the device or the host.

    steps: a list (or a Compose) of RandomHorizontalFlip, RandomVerticalFlip, RandomQuarterTurn, at most one ColorJitter and
        at most one SaturationHueJitter; anything else raises, naming the step.  The colour order is fixed - contrast,
        brightness, saturation, hue - so a SaturationHueJitter listed before the ColorJitter raises too; among the geometric
        steps its place is free (it commutes with them).
    seed: the Augment owns a CPU torch.Generator; `manual_seed(s)` re-seeds it (None: a seed of torch's choosing).

    The draw protocol, fixed: `draw_all(n)` (and `draw(n)`, its first two values) makes, for each step in the order listed,
    ONE call for the whole batch - a flip: torch.rand(n, float64) < p; a quarter turn: torch.randint(0, 4, (n,));
    ColorJitter: the contrast factors, then the brightness factors; SaturationHueJitter: the saturation factors, then the hue
    factors; each lo + (hi - lo) * torch.rand(n, float64) and only where lo < hi.  The geometric steps of a patch
    compose into ONE code through the multiplication table `D4` of the square's symmetries.  So with a single drawing step n
    draws of one patch consume the generator like one draw of n patches; with several steps the batch consumes it step by
    step and the repeated single draws patch by patch - equal seeds give equal items only under an equal batch structure."""

    def __init__(self, steps, seed=None):
        steps = list(steps.transforms) if isinstance(steps, Compose) else list(steps)
        self.jitter = self.hs = None
        for k, s in enumerate(steps):
            if isinstance(s, ColorJitter):
                if self.jitter is not None:
                    raise ValueError("Augment: step %d: %r is a second ColorJitter (at most one)" % (k, s))
                if self.hs is not None:
                    raise ValueError("Augment: step %d: %r follows %r, but the colour order is fixed (contrast, brightness, "
                                     "saturation, hue): list the ColorJitter first" % (k, s, self.hs))
                self.jitter = s
            elif isinstance(s, SaturationHueJitter):
                if self.hs is not None:
                    raise ValueError("Augment: step %d: %r is a second SaturationHueJitter (at most one)" % (k, s))
                self.hs = s
            elif not isinstance(s, (RandomHorizontalFlip, RandomQuarterTurn)):
                raise ValueError("Augment: step %d: %r is not a flip, a quarter turn, a ColorJitter or a SaturationHueJitter"
                                 % (k, s))
        self.steps = steps
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))

    def manual_seed(self, seed):
        self.generator.manual_seed(int(seed))
        return self

    def draw_all(self, n):
        """(codes uint8 [n], factors float64 (n, 2) = {contrast, brightness} or None without an effective ColorJitter,
        hs float64 (n, 2) = {saturation, hue} factors or None without an effective SaturationHueJitter)."""
        codes = torch.zeros(n, dtype=torch.uint8)
        factors = hs = None
        table = torch.from_numpy(D4)
        for s in self.steps:
            if isinstance(s, ColorJitter):
                factors = s.draw(n, self.generator)
            elif isinstance(s, SaturationHueJitter):
                hs = s.draw(n, self.generator)
            else:
                codes = table[codes.long(), s.draw(n, self.generator).long()]
        if self.jitter is not None and self.jitter.is_identity():
            factors = None
        if self.hs is not None and self.hs.is_identity():
            hs = None
        return codes, factors, hs

    def draw(self, n):
        """(codes uint8 [n], factors float64 (n, 2) = {contrast, brightness} or None without an effective ColorJitter): the
        first two values of `draw_all(n)`, which it consumes the generator as."""
        return self.draw_all(n)[:2]

    def apply(self, x, out=None, out_rows=None, out_float=False, norm=None):
        """`augment_patches` of uint8 x (N, 3, P, P) with one draw for its N patches (arguments as there).  With a contrast
        range the tables need every patch's grey mean: on a HIP device that is gnx_patch_grey_sum_u8 and one 8 N-byte copy
        to the host, i.e. ONE HOST SYNCHRONISATION PER BATCH, before the tables (numpy, N x 768 bytes) are uploaded.  The grey
        mean is that of the INPUT bytes, as ImageEnhance.Contrast's is.  A SaturationHueJitter adds `sat` (4 N bytes) and / or
        `hue` (N bytes) for its present stages and no synchronisation."""
        if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError("Augment.apply takes square uint8 patches (N, 3, P, P)")
        x = x.contiguous()
        N, P = int(x.shape[0]), int(x.shape[2])
        codes, factors, hs = self.draw_all(N)
        tables = None
        if factors is not None:
            means = None
            if self.jitter.needs_grey():
                if x.is_cuda:
                    sums = torch.empty(N, dtype=torch.int64, device=x.device)
                    with torch.cuda.device(x.device):
                        L.call('gnx_patch_grey_sum_u8', x.data_ptr(), N, P, sums.data_ptr(), L.stream())
                    sums = sums.cpu().numpy()                  # the synchronisation
                else:
                    sums = grey_sums(x)
                means = contrast_means(sums, P)
            tables = torch.from_numpy(color_tables(factors, means))
        if hs is None:
            return augment_patches(x, codes, tables, out=out, out_rows=out_rows, out_float=out_float, norm=norm)
        sat = hs[:, 0].contiguous() if self.hs.has_saturation() else None
        hue = torch.from_numpy(hue_shifts(hs[:, 1])) if self.hs.has_hue() else None
        return augment_patches(x, codes, tables, out=out, out_rows=out_rows, out_float=out_float, norm=norm, sat=sat, hue=hue)

    def __repr__(self):
        return "Augment([%s])" % ", ".join(repr(s) for s in self.steps)
