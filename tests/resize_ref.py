"""Pillow's BILINEAR resize of 8-bit images, restated in numpy: the defining arithmetic of gnx_resize_crop_u8
(include/gridnext_hip.h, "Resize + CenterCrop of uint8 patches").  test_resize_ref_host.py proves it equal to Pillow bit for
bit; test_gpu_resize.py compares the kernel with Pillow itself and uses this file for geometry only.

The resampling arithmetic is pillow_ref.py's, with the filter bound here to 'bilinear'; this file keeps the geometry of
torchvision's Resize / CenterCrop and the Pillow oracle."""
import functools

import numpy as np

import pillow_ref
from pillow_ref import patterns  # noqa: F401

coeffs = functools.partial(pillow_ref.coeffs, filter='bilinear')
ksize = functools.partial(pillow_ref.ksize, filter='bilinear')
_pass = functools.partial(pillow_ref._pass, filter='bilinear')


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
