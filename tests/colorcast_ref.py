"""numpy restatements of the colour-cast arithmetic (the reference's remove_color_cast / scale_rgb, imgprocess.py:49-67) on a
3 x 256 histogram and a 3 x 256 table - what the kernels of csrc/colorcast.hip and the host in between compute.
tests/test_colorcast_ref_host.py proves each of them against numpy's percentile and Pillow's point themselves; the GPU tests
compare the kernels against these.  Written independently of gridnext_amd/imgprocess.py on purpose."""
import numpy as np
from PIL import Image


def hist3(a):
    """uint8 (..., 3) -> int64 (3, 256): hist3(a)[c][v] = number of pixels whose channel c holds v."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.shape[-1] == 3
    flat = a.reshape(-1, 3)
    return np.stack([np.bincount(flat[:, c], minlength=256) for c in range(3)]).astype(np.int64)


def percentile99_from_hist(h):
    """np.percentile(x, q=99) of the n values counted in h (256 bins): numpy's method 'linear' takes the sorted values at
    floor(vi) and floor(vi) + 1, vi = (n - 1) * 0.99, and interpolates with weight g = vi - floor(vi) from below when g < 0.5,
    from above otherwise (numpy's _lerp)."""
    h = [int(x) for x in h]
    n = sum(h)
    assert len(h) == 256 and n > 0
    vi = (n - 1) * 0.99
    lo = int(np.floor(vi))
    hi = lo + 1
    if vi >= n - 1:                            # numpy: both indexes become the last one
        lo = hi = n - 1

    def kth(k):                                # the sorted value at index k
        seen = 0
        for v in range(256):
            seen += h[v]
            if seen > k:
                return v
        raise AssertionError(k)

    a, b = kth(lo), kth(hi)
    g = vi - np.floor(vi)
    if g >= 0.5:
        return float(b - (b - a) * (1 - g))
    return float(a + (b - a) * g)


def lut_from_scale(s):
    """Pillow's table for band.point(lambda i: i * s): round (Python's, half to even) and clip to a byte."""
    return np.array([min(255, max(0, round(i * s))) for i in range(256)], dtype=np.uint8)


def apply_luts(a, luts):
    """out[..., c] = luts[c][a[..., c]]"""
    out = np.empty_like(a)
    for c in range(3):
        out[..., c] = np.asarray(luts[c])[a[..., c]]
    return out


def scale_rgb_ref(a, scales):
    return apply_luts(a, [lut_from_scale(s) for s in scales])


def remove_color_cast_ref(a):
    """uint8 (H, W, 3) -> uint8 (H, W, 3): every channel times 255 / (its 99th percentile), as Pillow rounds and clips."""
    h = hist3(a)
    return scale_rgb_ref(a, [255 / percentile99_from_hist(h[c]) for c in range(3)])


# ---- the libraries themselves (what the restatements are proved against)
def pillow_scale_rgb(a, scales):
    source = Image.fromarray(a).split()
    bands = [source[c].point(lambda i, s=scales[c]: i * s) for c in range(3)]
    return np.array(Image.merge('RGB', bands))


def pillow_remove_color_cast(a):
    """The reference's expression, literally."""
    return pillow_scale_rgb(a, [255 / np.percentile(a[:, :, c].ravel(), q=99) for c in range(3)])


def channel(kind, n, rng):
    """n uint8 values of one of the test distributions."""
    if kind == 'uniform':
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 'band':
        return rng.integers(200, 206, n, dtype=np.uint8)
    if kind == 'skewed':
        return (rng.random(n) ** 0.2 * 250).astype(np.uint8)
    if kind == 'adjacent':
        return rng.integers(100, 103, n, dtype=np.uint8)
    raise ValueError(kind)


KINDS = ('uniform', 'band', 'skewed', 'adjacent')


def tinted(shape, seed):
    """A random slide with a colour cast: a bright background value on most pixels, channel maxima below 255, all percentiles
    positive."""
    rng = np.random.default_rng(seed)
    H, W = shape
    a = np.stack([(rng.random((H, W)) ** 0.3 * top).astype(np.uint8) for top in (231, 197, 246)], axis=-1)
    bg = rng.random((H, W)) < 0.4
    a[bg] = (228, 190, 241)
    return np.ascontiguousarray(a)
