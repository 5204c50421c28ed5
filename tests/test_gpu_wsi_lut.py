"""gnx_wsi_patch_grid_u8_lut / gnx_wsi_patch_grid_u8_f32_lut (csrc/wsi_patches.hip) through the C ABI against Pillow itself: the
per-channel table applied to the slide (tests/colorcast_ref.py: apply_luts = Pillow's point), then the window of every spot
through `Image.fromarray(window).resize((P, P))` (tests/wsi_ref.py: pillow_patch).  Every comparison is torch.equal - there is
no tolerance anywhere in this file.

Shapes and spots are those of tests/test_gpu_wsi_patches.py, the smallest at which each path can go wrong: the copy path,
byte stores, down, up, ksize 17 with most windows over an edge, ragged row tiles, the copy over two tiles; three of them with
the slide one byte into its storage (the head shift of a staged row and the channel phase of its bytes must not mix); a 5 x 6
slide under a 12-pixel window; 300 spots (the second launch sees the table too); 512 -> 128 (the large-LDS tile with the
table's 768 bytes on top).  Tables: three different random permutations of 0..255 (not monotone: a channel taken for another,
or a byte looked up twice, shows), the identity (== the plain entry point), three constants.  The slide's bytes are the same
after every call; cells that are not listed keep their fill; the refusals write nothing."""
import numpy as np
import pytest
import torch

import colorcast_ref as C
import wsi_ref as W
from test_gpu_wsi_patches import GRID, _call as _plain, _one_byte_in, _spots, _tables

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _perms(seed):
    rng = np.random.default_rng(seed)
    t = np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8)
    assert not np.array_equal(t[0], t[1]) and not np.array_equal(t[1], t[2]) and not np.array_equal(t[0], t[2])
    assert all(np.any(np.diff(t[c].astype(int)) < 0) for c in range(3))
    assert all(not np.array_equal(t[c][t[c]], t[c]) for c in range(3))         # looked up twice: other bytes
    return t


IDENTITY = np.stack([np.arange(256, dtype=np.uint8)] * 3)
CONSTANTS = np.stack([np.full(256, v, dtype=np.uint8) for v in (3, 140, 255)])


def _call(slide, spots, w, P, lut, as_float=False, norm=None, fill=7, grid=GRID, ksize=None, null_lut=False):
    """The _lut entry point by hand; the slide's bytes are compared before and after.  Returns (rc, out)."""
    from gridnext_amd import _lib as L
    half = w // 2
    coef, bnd, ks = _tables(2 * half, P)
    sp = np.ascontiguousarray(np.asarray(spots, dtype=np.int32).reshape(-1, 4))
    out = torch.full(tuple(grid) + (3, P, P), fill, device=DEV, dtype=torch.float32 if as_float else torch.uint8)
    table = torch.from_numpy(np.ascontiguousarray(lut)).to(DEV)
    before = slide.clone()
    args = (slide.data_ptr(), slide.shape[0], slide.shape[1], sp.ctypes.data, len(sp), half, P, grid[0], grid[1],
            coef.data_ptr(), bnd.data_ptr(), ks if ksize is None else ksize, out.data_ptr())
    tp = None if null_lut else table.data_ptr()
    if as_float:
        rc = L.query('gnx_wsi_patch_grid_u8_f32_lut', *args, None if norm is None else norm.data_ptr(), tp, L.stream())
    else:
        rc = L.query('gnx_wsi_patch_grid_u8_lut', *args, tp, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(slide, before), "the slide was written"
    assert torch.equal(table.cpu(), torch.from_numpy(np.ascontiguousarray(lut)))
    return rc, out


def _expected(host, lut, spots, w, P, fill=7, grid=GRID):
    mapped = C.apply_luts(host, lut)
    want = np.full(tuple(grid) + (3, P, P), fill, dtype=np.uint8)
    for x, y, r, c in spots:
        want[r, c] = W.pillow_patch(mapped, x, y, w, P)
    return torch.from_numpy(want)


# (Hs, Ws, P, w, one byte in)
CASES = [
    (41, 37, 8, 8, False),          # the copy path
    (41, 37, 7, 9, False),          # byte stores
    (41, 37, 8, 12, False),         # down
    (41, 37, 12, 8, False),         # up
    (41, 37, 8, 30, False),         # ksize 17; most windows reach over an edge
    (97, 101, 37, 40, False),       # ragged row tiles
    (97, 101, 36, 36, False),       # the copy path over two row tiles
    (41, 37, 8, 12, True),          # the slide 1 byte into its storage
    (41, 37, 8, 8, True),
    (97, 101, 32, 40, True),
]


@pytest.mark.parametrize("Hs,Ws,P,w,shifted", CASES)
def test_bytes_equal_pillow_of_the_mapped_slide(Hs, Ws, P, w, shifted):
    spots = _spots(Hs, Ws)
    pats = W.patterns((Hs, Ws, 3), seed=Hs + P + w)
    perms = _perms(Hs + 3 * P + w)
    for name in ('random', 'extremes'):
        host = pats[name]
        slide = _one_byte_in(host) if shifted else torch.from_numpy(host).to(DEV)
        for tname, lut in (('permutations', perms), ('constants', CONSTANTS)):
            rc, got = _call(slide, spots, w, P, lut)
            want = _expected(host, lut, spots, w, P)
            diff = int((got.cpu() != want).sum())
            print("%s %s %s: %d of %d bytes differ" % ((Hs, Ws, P, w, shifted), name, tname, diff, want.numel()))
            assert rc == 0 and torch.equal(got.cpu(), want), (name, tname)     # (the cells that are not listed: still 7)
        rc, got = _call(slide, spots, w, P, IDENTITY)
        rc0, plain = _plain(slide, spots, w, P)
        assert rc == 0 and rc0 == 0 and torch.equal(got, plain), name


def test_every_coordinate_clamped_window_larger_than_the_slide():
    host = W.patterns((5, 6, 3), seed=4)['random']
    lut = _perms(11)
    spots = [(x, y, y, x) for y in range(5) for x in range(6)]           # every pixel of the slide is a centre
    for P in (8, 12):                                                    # resampled, and the copy path
        rc, got = _call(torch.from_numpy(host).to(DEV), spots, 12, P, lut)
        assert rc == 0 and torch.equal(got.cpu(), _expected(host, lut, spots, 12, P))


def test_more_spots_than_one_launch_carries():
    """300 spots over a 20 x 15 grid: two launches, and the second one reads the table as well."""
    host = W.patterns((41, 37, 3), seed=5)['random']
    slide = torch.from_numpy(host).to(DEV)
    lut = _perms(12)
    rng = np.random.default_rng(6)
    many = [(int(rng.integers(0, 37)), int(rng.integers(0, 41)), i // 15, i % 15) for i in range(300)]
    for w, P in ((12, 8), (8, 8)):
        rc, got = _call(slide, many, w, P, lut, grid=(20, 15))
        assert rc == 0 and torch.equal(got.cpu(), _expected(host, lut, many, w, P, grid=(20, 15)))


def test_large_lds_tile_512_to_128():
    """512 -> 128 (4x, ksize 17) takes the large-LDS launch, the table's 768 bytes behind the two images.  One spot inside, one
    over the bottom-right corner."""
    host = W.patterns((600, 700, 3), seed=9)['random']
    lut = _perms(13)
    spots = [(300, 290, 0, 1), (690, 595, 1, 0)]
    rc, got = _call(torch.from_numpy(host).to(DEV), spots, 512, 128, lut, grid=(2, 2))
    assert rc == 0 and torch.equal(got.cpu(), _expected(host, lut, spots, 512, 128, grid=(2, 2)))


@pytest.mark.parametrize("Hs,Ws,P,w", [(41, 37, 8, 8), (41, 37, 7, 9), (41, 37, 8, 12), (97, 101, 36, 40)])
def test_float_form_equals_the_conversion_of_the_byte_form(Hs, Ws, P, w):
    """gnx_wsi_patch_grid_u8_f32_lut == gnx_resize_crop_u8_f32 run with identity geometry on gnx_wsi_patch_grid_u8_lut's bytes,
    with and without a norm vector; cells that are not listed keep what they held."""
    from gridnext_amd import transforms as T
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    nrm = torch.cat([mean, std, 1.0 / std]).to(DEV)
    host = W.patterns((Hs, Ws, 3), seed=1)['random']
    slide = torch.from_numpy(host).to(DEV)
    lut = _perms(14)
    spots = _spots(Hs, Ws)
    listed = torch.zeros(GRID, dtype=torch.bool)
    for _, _, r, c in spots:
        listed[r, c] = True
    rc, u8 = _call(slide, spots, w, P, lut)
    assert rc == 0 and torch.equal(u8.cpu(), _expected(host, lut, spots, w, P))
    for norm in (None, nrm):
        rc, got = _call(slide, spots, w, P, lut, as_float=True, norm=norm, fill=-7.0)
        assert rc == 0
        want = T.resize_crop(u8.view(-1, 3, P, P), None, None, norm, True).view(GRID + (3, P, P))
        assert torch.equal(got[listed], want[listed]), norm is not None
        assert bool((got[~listed] == -7.0).all())


def test_refusals_write_nothing():
    from gridnext_amd import _lib as L
    slide = torch.randint(0, 256, (41, 37, 3), device=DEV, dtype=torch.uint8)
    good = _spots(41, 37)
    lut = _perms(15)
    for as_float in (False, True):
        rc, out = _call(slide, good, 12, 8, lut, as_float=as_float, null_lut=True)           # NULL table, n > 0
        assert rc == -1 and bool((out == 7).all())
        rc, out = _call(slide, [], 12, 8, lut, as_float=as_float, null_lut=True)             # ... and n == 0: nothing to do
        assert rc == 0 and bool((out == 7).all())
        for bad in ((10, 10, GRID[0], 0), (10, 10, 0, GRID[1]), (10, 10, -1, 0), (10, 10, 0, -1)):
            rc, out = _call(slide, good[:3] + [bad], 12, 8, lut, as_float=as_float)
            assert rc == -1 and bool((out == 7).all())                                       # the good spots neither
        rc, out = _call(slide, good, 12, 8, lut, as_float=as_float, ksize=5)                 # not the ksize of (12, 8)
        assert rc == -1 and bool((out == 7).all())
        rc, out = _call(slide, good, 34, 8, lut, as_float=as_float)                          # 4.25x: ksize 19, the sibling's
        assert rc == L.ERR_UNSUPPORTED and bool((out == 7).all())
