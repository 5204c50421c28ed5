"""What the saturation / hue tests share: the image of all 2^24 colours, Pillow as the oracle (ImageEnhance.Color,
convert('HSV') / convert('RGB'), torchvision's adjust_hue written out in Pillow calls) and 2^24-entry tables of the package's
numpy restatement (`transforms.rgb_to_hsv_u8`, `hsv_to_rgb_u8`), so that the expected bytes of a hue shift are an index.
test_augment_hs_ref_host.py proves the restatement equal to Pillow on every colour; the GPU tests then compare the kernel with
the restatement.  Everything cached here is shared: do not write into it."""
import functools

import numpy as np
import torch
from PIL import Image, ImageEnhance

SHIFTS = (0, 1, 43, 127, 128, 213, 255)
SAT_FACTORS = (0.0, 0.3, 0.77, 1.0 - 1e-7, 1.0, 1.4, 2.5)        # inside, at the ends of and outside [0, 1]


@functools.lru_cache(None)
def all_colours():
    """uint8 (256, 3, 256, 256): patch k holds the colours (R, G, B) = (k, row, column)."""
    a = np.empty((256, 3, 256, 256), dtype=np.uint8)
    v = np.arange(256, dtype=np.uint8)
    a[:, 0], a[:, 1], a[:, 2] = v[:, None, None], v[None, :, None], v[None, None, :]
    return torch.from_numpy(a)


@functools.lru_cache(None)
def all_colours_hwc():
    """The same colours as one (4096, 4096, 3) array for Pillow: pixel index = R << 16 | G << 8 | B, row-major."""
    return np.ascontiguousarray(all_colours().permute(0, 2, 3, 1).numpy().reshape(4096, 4096, 3))


def to_hwc(x):
    """(N, 3, P, P) tensor -> (N, P, P, 3) numpy."""
    return np.ascontiguousarray(x.permute(0, 2, 3, 1).numpy())


def to_chw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


# ---- Pillow
def pil_saturate(a, f):
    return np.array(ImageEnhance.Color(Image.fromarray(a)).enhance(f))


def pil_rgb_to_hsv(a):
    return np.array(Image.fromarray(a).convert('HSV'))


def pil_hsv_to_rgb(a):
    h, s, v = (Image.fromarray(np.ascontiguousarray(a[..., c])) for c in range(3))
    return np.array(Image.merge('HSV', (h, s, v)).convert('RGB'))


def pil_hue(a, shift):
    """torchvision's adjust_hue in Pillow calls, given the uint8 shift."""
    h, s, v = Image.fromarray(a).convert('HSV').split()
    h = Image.fromarray(np.array(h, dtype=np.uint8) + np.uint8(shift))
    return np.array(Image.merge('HSV', (h, s, v)).convert('RGB'))


def pil_shift(fh):
    """The issue's rule for the shift of a hue factor."""
    return int(fh * 255) & 255


def pil_sat_hue(a, fs=None, fh=None):
    """ImageEnhance.Color(fs), then adjust_hue(fh), of the (P, P, 3) array; None: the stage is absent."""
    if fs is not None:
        a = pil_saturate(a, fs)
    if fh is not None:
        a = pil_hue(a, pil_shift(fh))
    return a


# ---- the restatement as tables
def _chunks(fn, a, step=1 << 20):
    """fn over the rows of a (n, 3) array, a chunk at a time (the restatement works in float64 and int64)."""
    return np.concatenate([fn(a[i:i + step]) for i in range(0, len(a), step)])


@functools.lru_cache(None)
def hsv_table():
    """(2^24, 3) uint8: transforms.rgb_to_hsv_u8 of colour R << 16 | G << 8 | B."""
    from gridnext_amd import transforms as T
    return _chunks(T.rgb_to_hsv_u8, all_colours_hwc().reshape(-1, 3))


@functools.lru_cache(None)
def rgb_table():
    """(2^24, 3) uint8: transforms.hsv_to_rgb_u8 of the HSV bytes H << 16 | S << 8 | V."""
    from gridnext_amd import transforms as T
    return _chunks(T.hsv_to_rgb_u8, all_colours_hwc().reshape(-1, 3))


def index(a):
    """(..., 3) uint8 -> the 24-bit index of each triple."""
    a = a.astype(np.int64)
    return (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]


def table_hue(a, shift):
    """`transforms.shift_hue_u8(a, shift)` through the two tables: RGB bytes (..., 3), shift a number or an array that
    broadcasts against the pixels."""
    hsv = hsv_table()[index(a)]
    hsv[..., 0] = hsv[..., 0] + np.asarray(shift).astype(np.uint8)
    return rgb_table()[index(hsv)]


def saturate(a, f):
    from gridnext_amd import transforms as T
    flat = a.reshape(-1, 3)
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), a.shape[:-1]).reshape(-1)
    step = 1 << 20
    return np.concatenate([T.saturate_u8(flat[i:i + step], f[i:i + step]) for i in range(0, len(flat), step)]).reshape(a.shape)
