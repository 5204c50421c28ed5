"""gnx_resize_crop_u8 / gnx_resize_crop_u8_f32 (csrc/resize.hip) through the C ABI against Pillow itself: Resize + CenterCrop
of uint8 patches, bit for bit.  Every comparison is torch.equal - there is no tolerance anywhere in this file.

Geometries: the tutorial's 260 -> 256 -> 224 and 300 -> 256 -> 224; 37 x 41 -> 16 -> 12 (widths no multiple of 4, odd plane
size so every plane starts at another alignment, a ragged last row tile); upscaling without a crop; a crop alone (margin 23 ->
offset 12, an output width that is no multiple of 4: byte stores); both passes skipped; ksize 9; a non-square source; an input
view that starts 1 byte into its storage; a plane so wide that a tile's rows need more than 64 KB of LDS; N = 0.  Patterns:
random, 0 / 255 extremes, all 0, all 255."""
import numpy as np
import pytest
import torch

import resize_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (N, H0, W0, resize, crop)
CASES = [
    (3, 260, 260, 256, 224),
    (2, 300, 300, 256, 224),
    (5, 37, 41, 16, 12),
    (1, 64, 64, 128, None),
    (2, 224, 224, None, 201),
    (2, 256, 256, 256, 224),
    (1, 1000, 1000, 256, 224),
    (4, 129, 257, 64, 64),
    (2, 40, 40, 32, 32),
]


def _geometry(H0, W0, resize, crop):
    Hr, Wr = R.resized_shape(H0, W0, resize)
    top, left, Ph, Pw = R.center_window(Hr, Wr, crop)
    return Hr, Wr, top, left, Ph, Pw


def _tables(H0, W0, geom):
    from gridnext_amd import transforms as T
    Hr, Wr, top, left, Ph, Pw = geom
    hc, hb = T.axis_tables(W0, Wr, left, Pw)
    vc, vb = T.axis_tables(H0, Hr, top, Ph)
    return [torch.from_numpy(a).to(DEV) for a in (hc, hb, vc, vb)]


def _call(x, resize, crop, norm=None, as_float=False, fill=None):
    """The entry point by hand: x uint8 (N, 3, H0, W0) on the device, any base alignment.  Returns (rc, out)."""
    from gridnext_amd import _lib as L
    N, _, H0, W0 = x.shape
    geom = _geometry(H0, W0, resize, crop)
    Hr, Wr, top, left, Ph, Pw = geom
    tabs = _tables(H0, W0, geom)
    out = torch.empty((N, 3, Ph, Pw), device=DEV, dtype=torch.float32 if as_float else torch.uint8)
    if fill is not None:
        out.fill_(fill)
    args = (x.data_ptr(), out.data_ptr(), N, H0, W0, Hr, Wr, top, left, Ph, Pw) + tuple(t.data_ptr() for t in tabs)
    if as_float:
        rc = L.query('gnx_resize_crop_u8_f32', *args, None if norm is None else norm.data_ptr(), L.stream())
    else:
        rc = L.query('gnx_resize_crop_u8', *args, L.stream())
    torch.cuda.synchronize()
    return rc, out


def _one_byte_in(host):
    """The patches as a device view that starts 1 byte into its storage."""
    store = torch.empty(host.size + 1, device=DEV, dtype=torch.uint8)
    view = store[1:].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize("N,H0,W0,resize,crop", CASES)
def test_bytes_equal_pillow(N, H0, W0, resize, crop):
    for name, host in R.patterns((N, 3, H0, W0), seed=H0 + W0).items():
        want = torch.from_numpy(R.pillow_resize_crop(host, resize, crop))
        x = _one_byte_in(host) if (H0, W0) == (40, 40) else torch.from_numpy(host).to(DEV)
        rc, got = _call(x, resize, crop, fill=7)
        assert rc == 0 and got.shape == want.shape
        diff = int((got.cpu() != want).sum())
        print("%s %s: %d of %d bytes differ" % ((N, H0, W0, resize, crop), name, diff, want.numel()))
        assert torch.equal(got.cpu(), want), name
        if name in ('zeros', 'full'):                     # an empty spot stays empty: skip_empty finds it after the resize
            assert bool((got == (0 if name == 'zeros' else 255)).all())


def test_plane_wider_than_64_kb_of_lds_per_tile():
    """2400 x 2400 -> Resize(320) (7.5x, ksize 17) -> CenterCrop(224): four output rows need 40 input rows of 2 400 bytes -
    the tile takes the large-LDS launch."""
    host = R.patterns((1, 3, 2400, 2400), seed=9)['random']
    want = torch.from_numpy(R.pillow_resize_crop(host, 320, 224))
    rc, got = _call(torch.from_numpy(host).to(DEV), 320, 224, fill=7)
    assert rc == 0 and torch.equal(got.cpu(), want)


def test_bytes_do_not_depend_on_batch_size_or_position():
    host = R.patterns((5, 3, 37, 41), seed=4)['random']
    x = torch.from_numpy(host).to(DEV)
    _, whole = _call(x, 16, 12)
    for i in range(5):                                     # x[i:i + 1]: a view at byte offset i * 4551 - every alignment
        _, one = _call(x[i:i + 1], 16, 12)
        assert torch.equal(one[0], whole[i]), i
    order = [3, 0, 4, 2, 1]
    _, moved = _call(x[order].contiguous(), 16, 12)
    assert torch.equal(moved, whole[order])
    _, twice = _call(torch.cat([x, x], 0), 16, 12)
    assert torch.equal(twice[:5], whole) and torch.equal(twice[5:], whole)


def test_reduction_above_8x_is_declined_and_nothing_is_launched():
    from gridnext_amd import _lib as L
    from gridnext_amd import transforms as T
    x = torch.randint(0, 256, (1, 3, 130, 130), device=DEV, dtype=torch.uint8)        # 130 -> 16: 8.125x, ksize 19
    for as_float in (False, True):
        rc, out = _call(x, 16, None, as_float=as_float, fill=7)
        assert rc == L.ERR_UNSUPPORTED and bool((out == 7).all())
    with pytest.raises(RuntimeError, match="unsupported shape"):
        T.resize_crop(x, 16, None)
    rc, out = _call(torch.randint(0, 256, (1, 3, 128, 128), device=DEV, dtype=torch.uint8), 16, None, fill=7)     # 8x: taken
    assert rc == 0 and not bool((out == 7).all())
    # a window outside the resized image: bad argument
    geom = (16, 16, 8, 0, 12, 12)
    tabs = _tables(128, 128, (16, 16, 0, 0, 12, 12))
    out = torch.full((1, 3, 12, 12), 7, device=DEV, dtype=torch.uint8)
    rc = L.query('gnx_resize_crop_u8', x.data_ptr(), out.data_ptr(), 1, 128, 128, *geom, *(t.data_ptr() for t in tabs), L.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == 7).all())


def test_no_patches():
    from gridnext_amd import transforms as T
    x = torch.empty((0, 3, 260, 260), device=DEV, dtype=torch.uint8)
    for as_float in (False, True):
        out = T.resize_crop(x, 256, 224, None, as_float)
        assert out.shape == (0, 3, 224, 224) and out.dtype == (torch.float32 if as_float else torch.uint8)
    rc, out = _call(x, 256, 224)
    assert rc == 0 and out.shape == (0, 3, 224, 224)


@pytest.mark.parametrize("N,H0,W0,resize,crop", [(3, 260, 260, 256, 224), (5, 37, 41, 16, 12), (2, 224, 224, None, 201),
                                                  (2, 40, 40, 32, 32), (2, 146, 146, 128, 128)])
def test_float_form_equals_the_conversion_of_the_byte_form(N, H0, W0, resize, crop):
    """gnx_resize_crop_u8_f32 == gnx_u8_to_f32 of gnx_resize_crop_u8's bytes, with and without a norm vector (201 x 201
    planes are no multiple of 4 pixels, which gnx_u8_to_f32 does not take: the torch expressions it equals stand in)."""
    from gridnext_amd import _lib as L
    from gridnext_amd import transforms as T
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    nrm = torch.cat([mean, std, 1.0 / std]).to(DEV)
    for name, host in R.patterns((N, 3, H0, W0), seed=1).items():
        x = torch.from_numpy(host).to(DEV)
        _, u8 = _call(x, resize, crop)
        for norm in (None, nrm):
            rc, got = _call(x, resize, crop, norm=norm, as_float=True, fill=-7.0)
            assert rc == 0
            want = torch.empty_like(got)
            if not L.try_call('gnx_u8_to_f32', u8.data_ptr(), L.ptr(want), N, 3, u8.shape[2], u8.shape[3],
                              None if norm is None else L.ptr(norm), L.stream()):
                assert (u8.shape[2] * u8.shape[3]) % 4 != 0
                want = u8.cpu().float().div(255)               # (on the host: a true division, as ToTensor's)
                if norm is not None:
                    want = (want - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
                want = want.to(DEV)
            assert torch.equal(got, want), (name, norm is not None)
            assert torch.equal(T.resize_crop(x, resize, crop, norm, True), got)       # the package's wrapper: the same call
        assert torch.equal(T.resize_crop(x, resize, crop), u8)


def test_wrapper_refuses_what_the_transform_is_not_defined_on():
    from gridnext_amd import transforms as T
    with pytest.raises(ValueError, match="uint8"):
        T.resize_crop(torch.rand(1, 3, 40, 40, device=DEV), 32, 32)
    with pytest.raises(RuntimeError, match="HIP device"):
        T.resize_crop(torch.zeros(1, 3, 40, 40, dtype=torch.uint8), 32, 32)
    with pytest.raises(ValueError, match="larger"):
        T.resize_crop(torch.zeros(1, 3, 40, 40, device=DEV, dtype=torch.uint8), 32, 33)
    # a view whose patches do not lie back to back is copied first
    x = torch.randint(0, 256, (4, 3, 40, 40), device=DEV, dtype=torch.uint8)
    assert torch.equal(T.resize_crop(x[::2], 32, 32), T.resize_crop(x, 32, 32)[::2])
