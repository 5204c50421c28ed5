"""The arithmetic of the whole-slide patch gather on the host (no GPU):
 * tests/wsi_ref.py - the numpy restatement of Pillow's fixed-point BICUBIC resize that gnx_wsi_patch_grid_u8 implements -
   equals `Image.fromarray(a).resize((P, P))` byte for byte over a grid of window / patch pairs and byte patterns;
 * clamp addressing equals the reference's literal np.pad(mode='edge') + slice, at corners, edges and for a window larger
   than the whole slide;
 * gridnext_amd.transforms.axis_tables(..., filter='bicubic') (the tables the kernel reads) equals the restatement's;
 * axis_tables / axis_ksize without the argument return what they returned before."""
import numpy as np
import pytest
from PIL import Image

import resize_ref as R
import wsi_ref as W
from gridnext_amd import transforms as T


# (H0, W0, Hr, Wr): the geometries of tests/test_resize_ref_host.py
GEOMETRIES = [(260, 260, 256, 256), (300, 300, 256, 256), (64, 64, 128, 128), (37, 41, 16, 17), (129, 257, 64, 127),
              (41, 41, 40, 40), (40, 40, 41, 41), (50, 60, 50, 45), (60, 50, 45, 50), (127, 255, 16, 32), (120, 90, 31, 23),
              (33, 20, 70, 25)]


@pytest.mark.parametrize("n,P", W.PAIRS)
def test_restatement_equals_pillow_bit_for_bit(n, P):
    for name, a in W.patterns((n, n, 3), seed=100 * n + P).items():
        want = np.array(Image.fromarray(a).resize((P, P)))          # Pillow's default filter
        assert np.array_equal(want, np.array(Image.fromarray(a).resize((P, P), Image.BICUBIC))), "the default is BICUBIC"
        got = W.resize_hwc(a, P)
        assert got.shape == (P, P, 3) and got.dtype == np.uint8
        assert np.array_equal(got, want), "%s: %d bytes differ" % (name, int((got != want).sum()))
        if name == 'zeros':
            assert not got.any()
        if name == 'full':
            assert (got == 255).all()
    const = np.full((n, n, 3), 77, dtype=np.uint8)
    assert np.array_equal(W.resize_hwc(const, P), np.array(Image.fromarray(const).resize((P, P))))


def test_identity_size_is_a_copy_and_single_axes_are_skipped():
    a = W.patterns((8, 8, 3), seed=1)['random']
    assert np.array_equal(np.array(Image.fromarray(a).resize((8, 8))), a)
    assert np.array_equal(W.resize_hwc(a, 8), a)
    b = W.patterns((9, 14, 3), seed=2)['random']                  # (a window is always square; the passes are per axis)
    assert np.array_equal(W.resize_hwc(b, 9), np.array(Image.fromarray(b).resize((9, 9))))
    assert np.array_equal(W.resize_hwc(b, 14), np.array(Image.fromarray(b).resize((14, 14))))


def test_clamped_window_equals_the_padded_slice():
    slide = W.patterns((47, 61, 3), seed=3)['random']
    Hs, Ws = slide.shape[:2]
    centres = [(0, 0), (Ws - 1, 0), (0, Hs - 1), (Ws - 1, Hs - 1), (30, 0), (0, 23), (Ws - 1, 23), (30, Hs - 1), (20, 15),
               (2, 3), (Ws - 3, Hs - 2)]
    for w in (8, 5, 12, 30, 2, 100):
        for cx, cy in centres:
            got = W.window_clamped(slide, cx, cy, w)
            want = W.window_padded(slide, cx, cy, w)
            assert got.shape == (2 * (w // 2), 2 * (w // 2), 3)           # an odd w gives a window of w - 1
            assert np.array_equal(got, want), (w, cx, cy)
    # interior: the plain slice
    assert np.array_equal(W.window_clamped(slide, 20, 15, 8), slide[11:19, 16:24])
    # a window larger than the whole slide: every coordinate is clamped
    small = W.patterns((5, 6, 3), seed=4)['random']
    for cx in range(6):
        for cy in range(5):
            got = W.window_clamped(small, cx, cy, 12)
            assert got.shape == (12, 12, 3) and np.array_equal(got, W.window_padded(small, cx, cy, 12))
            assert np.array_equal(W.patch(small, cx, cy, 12, 8), W.pillow_patch(small, cx, cy, 12, 8))


@pytest.mark.parametrize("n,P", W.PAIRS)
def test_bicubic_axis_tables_equal_the_restatement(n, P):
    coef, bnd = T.axis_tables(n, P, filter='bicubic')
    assert coef.dtype == np.int32 and bnd.dtype == np.int32 and coef.flags['C_CONTIGUOUS']
    if n == P:                                  # identity: one tap of 2^22 at the index itself
        assert T.axis_ksize(n, P, 'bicubic') == T.axis_ksize(n, P, filter='bicubic') == 1 and coef.shape == (P, 1)
        assert (coef == 1 << 22).all() and np.array_equal(bnd, np.stack([np.arange(P), np.ones(P)], 1))
        return
    kk, bb = W.coeffs(n, P)
    assert T.axis_ksize(n, P, 'bicubic') == W.ksize(n, P) == coef.shape[1]
    assert np.array_equal(coef, kk) and np.array_equal(bnd, bb)
    assert (bnd[:, 0] >= 0).all() and (bnd[:, 0] + bnd[:, 1] <= n).all() and (bnd[:, 1] >= 1).all()
    assert (np.diff(bnd[:, 0]) >= 0).all() and (np.diff(bnd[:, 0] + bnd[:, 1]) >= 0).all()      # a tile's rows: first .. last
    if (n, P) in ((12, 8), (8, 12), (30, 8), (40, 37)):
        assert (coef < 0).any()                 # bicubic has negative weights: the (int)(-0.5 + w 2^22) rounding is in play
    # the accumulator fits 32 bits whatever the bytes: 255 * (sum of the positive weights) + 2^21, -255 * (the negative ones)
    pos = np.where(coef > 0, coef, 0).astype(np.int64).sum(1).max()
    neg = np.where(coef < 0, coef, 0).astype(np.int64).sum(1).min()
    assert 255 * int(pos) + (1 << 21) < 2 ** 31 and 255 * int(neg) >= -2 ** 31
    lo, m = P // 3, P - P // 3 - 1              # a window's tables are the rows of the full ones
    if m > 0:
        cw, bw = T.axis_tables(n, P, lo, m, filter='bicubic')
        assert np.array_equal(cw, coef[lo:lo + m]) and np.array_equal(bw, bnd[lo:lo + m])


def test_bicubic_ksize_limits():
    assert T.axis_ksize(30, 8, 'bicubic') == 17 and T.axis_ksize(32, 8, 'bicubic') == 17       # up to 4x: taken
    assert T.axis_ksize(34, 8, 'bicubic') == 19 and T.axis_ksize(1026, 256, 'bicubic') == 19
    assert T.axis_ksize(8, 12, 'bicubic') == 5 and T.axis_ksize(320, 256, 'bicubic') == 7
    with pytest.raises(ValueError, match="filter"):
        T.axis_ksize(8, 12, 'lanczos')
    with pytest.raises(ValueError, match="filter"):
        T.axis_tables(8, 12, filter='nearest')


@pytest.mark.parametrize("H0,W0,Hr,Wr", GEOMETRIES)
def test_default_filter_is_unchanged(H0, W0, Hr, Wr):
    for n_in, n_out in ((W0, Wr), (H0, Hr)):
        coef, bnd = T.axis_tables(n_in, n_out)
        cb, bb = T.axis_tables(n_in, n_out, filter='bilinear')
        assert np.array_equal(coef, cb) and np.array_equal(bnd, bb)
        assert T.axis_ksize(n_in, n_out) == T.axis_ksize(n_in, n_out, 'bilinear')
        if n_in == n_out:
            assert coef.shape == (n_out, 1) and (coef == 1 << 22).all()
            continue
        kk, kb = R.coeffs(n_in, n_out)                   # the bilinear restatement: what the tables were before
        assert np.array_equal(coef, kk) and np.array_equal(bnd, kb) and coef.shape[1] == R.ksize(n_in, n_out)
