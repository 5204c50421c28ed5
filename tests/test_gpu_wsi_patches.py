"""gnx_wsi_patch_grid_u8 / gnx_wsi_patch_grid_u8_f32 (csrc/wsi_patches.hip) through the C ABI against Pillow itself: the window
of every spot, every coordinate clamped to the slide, through `Image.fromarray(window).resize((P, P))` (BICUBIC), planar, at the
spot's cell.  Every comparison is torch.equal - there is no tolerance anywhere in this file.

Shapes, the smallest at which each path can go wrong: the copy path (8 from 8), byte stores (P = 7), up (8 -> 12), down
(12 -> 8), ksize 17 (30 -> 8), 34 -> 8 declined; slides 37 and 101 pixels wide (111 and 303 bytes per row: rows start at every
alignment modulo 16); a slide view that starts 1 byte into its storage; spots in all four corners, on the mid-edges and inside;
a 5 x 6 slide under a 12-pixel window (every coordinate clamped); several row tiles with a ragged last one (P = 37 from 40);
a tile that needs the large-LDS launch (512 -> 128); n = 0; cells that are not listed keep what they held; a grid index
outside the grid; the float form against gnx_resize_crop_u8_f32; a slide of more than 2^31 bytes."""
import numpy as np
import pytest
import torch

import wsi_ref as W

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRID = (5, 6)           # (grid_h, grid_w) of most calls here: 30 cells


def _tables(win, P):
    from gridnext_amd import transforms as T
    coef, bnd = T.axis_tables(win, P, filter='bicubic')
    return torch.from_numpy(coef).to(DEV), torch.from_numpy(bnd).to(DEV), T.axis_ksize(win, P, 'bicubic')


def _call(slide, spots, w, P, as_float=False, norm=None, fill=7, grid=GRID, ksize=None):
    """The entry point by hand: slide uint8 (Hs, Ws, 3) on the device, spots [(x_px, y_px, grid_row, grid_col)] on the host.
    Returns (rc, out)."""
    from gridnext_amd import _lib as L
    half = w // 2
    coef, bnd, ks = _tables(2 * half, P)
    sp = np.ascontiguousarray(np.asarray(spots, dtype=np.int32).reshape(-1, 4))
    out = torch.full(tuple(grid) + (3, P, P), fill, device=DEV, dtype=torch.float32 if as_float else torch.uint8)
    args = (slide.data_ptr(), slide.shape[0], slide.shape[1], sp.ctypes.data, len(sp), half, P, grid[0], grid[1],
            coef.data_ptr(), bnd.data_ptr(), ks if ksize is None else ksize, out.data_ptr())
    if as_float:
        rc = L.query('gnx_wsi_patch_grid_u8_f32', *args, None if norm is None else norm.data_ptr(), L.stream())
    else:
        rc = L.query('gnx_wsi_patch_grid_u8', *args, L.stream())
    torch.cuda.synchronize()
    return rc, out


def _expected(host, spots, w, P, fill=7, grid=GRID):
    want = np.full(tuple(grid) + (3, P, P), fill, dtype=np.uint8)
    for x, y, r, c in spots:
        want[r, c] = W.pillow_patch(host, x, y, w, P)
    return torch.from_numpy(want)


def _spots(Hs, Ws, grid=GRID):
    """Corners, mid-edges, a pixel off each edge, and inside at several alignments: one cell each, in scattered order."""
    pts = [(0, 0), (Ws - 1, 0), (0, Hs - 1), (Ws - 1, Hs - 1), (Ws // 2, 0), (0, Hs // 2), (Ws - 1, Hs // 2), (Ws // 2, Hs - 1),
           (1, 1), (Ws - 2, Hs - 2), (Ws // 2, Hs // 2), (Ws // 2 + 1, Hs // 2 - 3), (Ws // 3, Hs // 3), (Ws // 3 + 2, Hs // 3 + 1),
           (2 * Ws // 3, Hs // 4), (Ws // 4 + 3, 2 * Hs // 3)]
    cells = [(i * 7) % (grid[0] * grid[1]) for i in range(len(pts))]
    assert len(set(cells)) == len(cells)
    return [(x, y, c // grid[1], c % grid[1]) for (x, y), c in zip(pts, cells)]


def _one_byte_in(host):
    """The slide as a device view that starts 1 byte into its storage."""
    store = torch.empty(host.size + 1, device=DEV, dtype=torch.uint8)
    view = store[1:].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


# (Hs, Ws, P, w, one byte in)
CASES = [
    (41, 37, 8, 8, False),          # the copy path
    (41, 37, 7, 9, False),          # window 8 -> 7: byte stores
    (41, 37, 12, 8, False),         # up
    (41, 37, 8, 12, False),         # down
    (41, 37, 8, 30, False),         # ksize 17; most windows reach over an edge
    (41, 37, 8, 5, False),          # an odd window: 4 pixels
    (41, 37, 8, 12, True),          # the slide 1 byte into its storage
    (41, 37, 8, 8, True),
    (97, 101, 37, 40, False),       # row tiles of 32 + 5, byte stores
    (97, 101, 36, 36, False),       # the copy path over two row tiles
    (97, 101, 32, 40, True),
]


@pytest.mark.parametrize("Hs,Ws,P,w,shifted", CASES)
def test_bytes_equal_pillow(Hs, Ws, P, w, shifted):
    spots = _spots(Hs, Ws)
    pats = W.patterns((Hs, Ws, 3), seed=Hs + P + w)
    for name in (('random', 'extremes', 'zeros', 'full') if P <= 8 else ('random', 'extremes')):
        host = pats[name]
        slide = _one_byte_in(host) if shifted else torch.from_numpy(host).to(DEV)
        rc, got = _call(slide, spots, w, P)
        want = _expected(host, spots, w, P)
        diff = int((got.cpu() != want).sum())
        print("%s %s: %d of %d bytes differ" % ((Hs, Ws, P, w, shifted), name, diff, want.numel()))
        assert rc == 0 and torch.equal(got.cpu(), want), name            # (the cells that are not listed: still 7)


def test_every_coordinate_clamped_window_larger_than_the_slide():
    host = W.patterns((5, 6, 3), seed=4)['random']
    spots = [(x, y, y, x) for y in range(5) for x in range(6)]           # every pixel of the slide is a centre
    rc, got = _call(torch.from_numpy(host).to(DEV), spots, 12, 8)
    assert rc == 0 and torch.equal(got.cpu(), _expected(host, spots, 12, 8))
    rc, got = _call(torch.from_numpy(host).to(DEV), spots, 12, 12)       # ... and on the copy path
    assert rc == 0 and torch.equal(got.cpu(), _expected(host, spots, 12, 12))


def test_bytes_do_not_depend_on_cell_order_or_company():
    host = W.patterns((41, 37, 3), seed=5)['random']
    slide = torch.from_numpy(host).to(DEV)
    spots = _spots(41, 37)
    _, whole = _call(slide, spots, 12, 8)
    for x, y, r, c in spots[::3]:
        rc, one = _call(slide, [(x, y, 0, 0)], 12, 8, grid=(1, 1))
        assert rc == 0 and torch.equal(one[0, 0], whole[r, c])
    # more spots than one launch carries (224): 300 spots over a 20 x 15 grid
    rng = np.random.default_rng(6)
    many = [(int(rng.integers(0, 37)), int(rng.integers(0, 41)), i // 15, i % 15) for i in range(300)]
    rc, got = _call(slide, many, 12, 8, grid=(20, 15))
    assert rc == 0 and torch.equal(got.cpu(), _expected(host, many, 12, 8, grid=(20, 15)))


def test_large_lds_tile_512_to_128():
    """A 512-pixel window to 128 pixels (4x, ksize 17): eight output rows need 47 window rows of 1 536 bytes - the tile takes
    the large-LDS launch.  One spot inside, one over the bottom-right corner."""
    host = W.patterns((600, 700, 3), seed=9)['random']
    spots = [(300, 290, 0, 1), (690, 595, 1, 0)]
    rc, got = _call(torch.from_numpy(host).to(DEV), spots, 512, 128, grid=(2, 2))
    assert rc == 0 and torch.equal(got.cpu(), _expected(host, spots, 512, 128, grid=(2, 2)))


def test_window_above_4x_is_declined_and_nothing_is_launched():
    from gridnext_amd import _lib as L
    slide = torch.randint(0, 256, (41, 37, 3), device=DEV, dtype=torch.uint8)
    spots = _spots(41, 37)
    for as_float in (False, True):
        rc, out = _call(slide, spots, 34, 8, as_float=as_float)            # 4.25x: ksize 19
        assert rc == L.ERR_UNSUPPORTED and bool((out == 7).all())
    rc, out = _call(slide, spots, 32, 8)                                    # 4x: taken
    assert rc == 0 and not bool((out == 7).all())
    rc, out = _call(slide, spots, 12, 8, ksize=5)                           # not the ksize of (12, 8): bad argument
    assert rc == -1 and bool((out == 7).all())


def test_grid_index_outside_the_grid_is_a_bad_argument():
    slide = torch.randint(0, 256, (41, 37, 3), device=DEV, dtype=torch.uint8)
    good = _spots(41, 37)[:3]
    for bad in ((10, 10, GRID[0], 0), (10, 10, 0, GRID[1]), (10, 10, -1, 0), (10, 10, 0, -1)):
        for as_float in (False, True):
            rc, out = _call(slide, good + [bad], 12, 8, as_float=as_float)
            assert rc == -1 and bool((out == 7).all())                      # nothing was launched: the good spots neither


def test_no_spots():
    slide = torch.randint(0, 256, (41, 37, 3), device=DEV, dtype=torch.uint8)
    for as_float in (False, True):
        rc, out = _call(slide, [], 12, 8, as_float=as_float)
        assert rc == 0 and bool((out == 7).all())


@pytest.mark.parametrize("Hs,Ws,P,w", [(41, 37, 8, 8), (41, 37, 7, 9), (41, 37, 8, 12), (97, 101, 36, 40)])
def test_float_form_equals_the_conversion_of_the_byte_form(Hs, Ws, P, w):
    """gnx_wsi_patch_grid_u8_f32 == gnx_resize_crop_u8_f32 run with identity geometry on gnx_wsi_patch_grid_u8's bytes, with
    and without a norm vector; cells that are not listed keep what they held."""
    from gridnext_amd import transforms as T
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    nrm = torch.cat([mean, std, 1.0 / std]).to(DEV)
    host = W.patterns((Hs, Ws, 3), seed=1)['random']
    slide = torch.from_numpy(host).to(DEV)
    spots = _spots(Hs, Ws)
    listed = torch.zeros(GRID, dtype=torch.bool)
    for _, _, r, c in spots:
        listed[r, c] = True
    _, u8 = _call(slide, spots, w, P)
    for norm in (None, nrm):
        rc, got = _call(slide, spots, w, P, as_float=True, norm=norm, fill=-7.0)
        assert rc == 0
        want = T.resize_crop(u8.view(-1, 3, P, P), None, None, norm, True).view(GRID + (3, P, P))
        assert torch.equal(got[listed], want[listed]), norm is not None
        assert bool((got[~listed] == -7.0).all())


def _closed_form(y, x, c):
    """The big slide's bytes as a function of (row, column, channel): int64 arrays or tensors that broadcast."""
    return ((x * 7 + y * 13 + c * 61) + (x * y) % 251) % 256


def test_slide_of_more_than_2_to_31_bytes():
    """26 800 x 26 800 x 3 bytes = 2.15e9: filled on the device in row blocks from a closed form, four spots in its last rows
    (byte offsets above 2^31), the expected windows from the same closed form on the host through Pillow."""
    S = 26800
    slide = torch.empty((S, S, 3), device=DEV, dtype=torch.uint8)
    assert slide.numel() > 2 ** 31
    xs = torch.arange(S, device=DEV, dtype=torch.int64).view(1, S, 1)
    cs = torch.arange(3, device=DEV, dtype=torch.int64).view(1, 1, 3)
    for y0 in range(0, S, 200):
        ys = torch.arange(y0, min(y0 + 200, S), device=DEV, dtype=torch.int64).view(-1, 1, 1)
        slide[y0:y0 + 200] = _closed_form(ys, xs, cs).to(torch.uint8)
    spots = [(S - 1, S - 1, 0, 0), (13000, S - 10, 0, 1), (5, S - 40, 1, 0), (26000, S - 70, 1, 1)]
    assert min(((y - 6) * S + x) * 3 for x, y, _, _ in spots) > 2 ** 31          # (the last 89 rows lie above 2^31)
    for w, P in ((12, 8), (8, 8)):
        half = w // 2
        want = np.full((2, 2, 3, P, P), 7, dtype=np.uint8)
        for x, y, r, c in spots:
            yy = np.clip(np.arange(y - half, y + half), 0, S - 1).astype(np.int64).reshape(-1, 1, 1)
            xx = np.clip(np.arange(x - half, x + half), 0, S - 1).astype(np.int64).reshape(1, -1, 1)
            win = _closed_form(yy, xx, np.arange(3, dtype=np.int64).reshape(1, 1, 3)).astype(np.uint8)
            from PIL import Image
            want[r, c] = np.array(Image.fromarray(win).resize((P, P))).transpose(2, 0, 1)
        rc, got = _call(slide, spots, w, P, grid=(2, 2))
        assert rc == 0 and torch.equal(got.cpu(), torch.from_numpy(want)), (w, P)
    # the read-back of a few bytes past 2^31 agrees with the closed form (the fill itself)
    assert int(slide[S - 1, S - 1, 2]) == int(_closed_form(np.int64(S - 1), np.int64(S - 1), np.int64(2)))
