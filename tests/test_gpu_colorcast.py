"""gnx_rgb_hist_u8 / gnx_rgb_lut_u8 (csrc/colorcast.hip) through the C ABI against np.bincount and a numpy table lookup, and
the public `remove_color_cast` / `scale_rgb` / `grid_from_wsi_visium(remove_cast=True)` on a HIP tensor against
tests/colorcast_ref.py and against Pillow itself.  Every comparison is torch.equal / np.array_equal - there is no tolerance
anywhere in this file.

Shapes, the smallest at which each part can go wrong: 0 .. 33 pixels around the 48-byte unit at every base offset 0 .. 15 (3 does
not divide 16: channel phase and alignment phase are independent); one pixel around what one workgroup covers per pass
(256 threads x 16 pixels) and what the whole grid covers per pass (1 536 workgroups), and a size with more passes than the grid
has workgroups; the lookup's 2 048-workgroup grid likewise; every src-against-dst shift modulo 16; a constant image of
2^22 + 1 pixels; images of more than 2^31 bytes and of more than 2^32 pixels, built on the device."""
import os

import numpy as np
import pytest
import torch

import colorcast_ref as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# restated from csrc/colorcast.hip
THREADS, UNIT_PIXELS, HIST_BLOCKS, LUT_BLOCKS, FLUSH_PASSES = 256, 16, 1536, 2048, 64
PASS = THREADS * UNIT_PIXELS                 # pixels one workgroup covers per pass: 4 096
HIST_LAUNCH = HIST_BLOCKS * PASS             # pixels the histogram's whole grid covers per pass
LUT_LAUNCH = LUT_BLOCKS * PASS
SMALL = (0, 1, 5, 15, 16, 17, 31, 33)
GARBAGE = 0x5A5A5A5A5A5A5A5A


def _at_offset(flat, off, pad=0):
    """The bytes `flat` (host uint8, 1-D) on the device, `off` bytes into a 16-byte aligned storage; returns (storage, view)."""
    flat = torch.as_tensor(flat).reshape(-1)
    store = torch.empty(off + flat.numel() + pad, device=DEV, dtype=torch.uint8)
    assert store.data_ptr() % 16 == 0
    view = store[off:off + flat.numel()]
    view.copy_(flat)
    return store, view


def _hist(view, n_pixels):
    """The entry point by hand, hist and workspace pre-filled with garbage.  Returns (rc, int64 (3, 256) on the host)."""
    from gridnext_amd import _lib as L
    hist = torch.full((768,), GARBAGE, device=DEV, dtype=torch.int64)
    nws = L.query('gnx_rgb_hist_u8_workspace', n_pixels)
    assert nws % 8 == 0 and nws == min(-(-n_pixels // PASS), HIST_BLOCKS) * 768 * 8
    ws = torch.full((max(nws // 8, 1),), GARBAGE, device=DEV, dtype=torch.int64)
    rc = L.query('gnx_rgb_hist_u8', view.data_ptr(), n_pixels, hist.data_ptr(), ws.data_ptr() if nws else None, L.stream())
    torch.cuda.synchronize()
    return rc, hist.cpu().numpy().reshape(3, 256)


def _lut_call(src_ptr, dst_ptr, n_pixels, table):
    from gridnext_amd import _lib as L
    rc = L.query('gnx_rgb_lut_u8', src_ptr, dst_ptr, n_pixels, table.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope='module')
def noise():
    """2 HIST_LAUNCH + PASS + 7 random pixels, shared (read-only) by the tests below."""
    return np.random.default_rng(0).integers(0, 256, 3 * (2 * HIST_LAUNCH + PASS + 7), dtype=np.uint8)


@pytest.fixture(scope='module')
def tables():
    """uint8 (3, 256) tables that differ per channel (a wrong channel phase shows), host and device."""
    rng = np.random.default_rng(1)
    host = np.stack([rng.permutation(256).astype(np.uint8) for _ in range(3)])
    return host, torch.from_numpy(host).to(DEV)


# ---------------------------------------------------------------------------------------------- histogram
def test_hist_small_sizes_at_every_base_offset(noise):
    for n in SMALL:
        for off in range(16):
            a = noise[1000 * off + n:][:3 * n]
            _, view = _at_offset(a, off)
            rc, got = _hist(view, n)
            assert rc == 0 and np.array_equal(got, C.hist3(a.reshape(-1, 3))), (n, off)


@pytest.mark.parametrize("n", [PASS - 1, PASS, PASS + 1, HIST_LAUNCH - 1, HIST_LAUNCH, HIST_LAUNCH + 1, 2 * HIST_LAUNCH + PASS + 7])
def test_hist_around_what_a_workgroup_and_the_grid_cover(noise, n):
    a = noise[:3 * n]
    want = C.hist3(a.reshape(-1, 3))
    for off in (0, 7):
        _, view = _at_offset(a, off)
        rc, got = _hist(view, n)
        assert rc == 0 and np.array_equal(got, want), off
    rc, again = _hist(view, n)                                   # two calls: equal results
    assert rc == 0 and np.array_equal(again, got)


def test_hist_constant_image_every_add_on_one_counter():
    n = 2 ** 22 + 1
    for off in (0, 5):
        store = torch.empty(3 * n + off, device=DEV, dtype=torch.uint8)
        view = store[off:]
        view.view(n, 3).copy_(torch.tensor([228, 190, 241], dtype=torch.uint8, device=DEV).expand(n, 3))
        rc, got = _hist(view, n)
        want = np.zeros((3, 256), dtype=np.int64)
        want[0, 228] = want[1, 190] = want[2, 241] = n
        assert rc == 0 and np.array_equal(got, want), off
    view.fill_(7)                                                # ... and the same value in every channel
    rc, got = _hist(view, n)
    assert rc == 0 and got[:, 7].tolist() == [n, n, n] and int(got.sum()) == 3 * n


def test_hist_edge_bins_only():
    rng = np.random.default_rng(2)
    n = 3 * PASS + 11
    a = (rng.integers(0, 2, 3 * n, dtype=np.uint8) * 255).astype(np.uint8)
    _, view = _at_offset(a, 3)
    rc, got = _hist(view, n)
    want = C.hist3(a.reshape(-1, 3))
    assert rc == 0 and np.array_equal(got, want) and int(got[:, 1:255].sum()) == 0 and int(got[:, 0].min()) > 0


def test_hist_bad_arguments():
    from gridnext_amd import _lib as L
    x = torch.zeros(48, device=DEV, dtype=torch.uint8)
    hist = torch.zeros(769, device=DEV, dtype=torch.int64)
    ws = torch.zeros(768, device=DEV, dtype=torch.int64)
    assert L.query('gnx_rgb_hist_u8', x.data_ptr(), 16, None, ws.data_ptr(), L.stream()) == -1
    assert L.query('gnx_rgb_hist_u8', x.data_ptr(), 16, hist.data_ptr() + 4, ws.data_ptr(), L.stream()) == -1
    assert L.query('gnx_rgb_hist_u8', x.data_ptr(), 16, hist.data_ptr(), None, L.stream()) == -1
    assert L.query('gnx_rgb_hist_u8', None, 16, hist.data_ptr(), ws.data_ptr(), L.stream()) == -1
    assert L.query('gnx_rgb_hist_u8_workspace', 0) == 0
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0


def _crt_counts(n_bytes):
    """Counts of the image whose byte at offset o is o % 251: channel o % 3, value o % 251, so (c, v) owns one residue modulo
    753."""
    want = np.zeros((3, 256), dtype=np.int64)
    for r in range(753):
        if r < n_bytes:
            want[r % 3, r % 251] = (n_bytes - 1 - r) // 753 + 1
    return want


def test_hist_image_of_more_than_2_to_31_bytes():
    n = 2 ** 31 // 3 + 1000
    nb = 3 * n
    assert nb > 2 ** 31 and -(-n // PASS) > HIST_BLOCKS * FLUSH_PASSES          # ... and the 32-bit counters are folded on the way
    store = torch.empty(nb + 1, device=DEV, dtype=torch.uint8)
    view = store[1:]
    step = 2 ** 26
    for o0 in range(0, nb, step):
        o1 = min(o0 + step, nb)
        view[o0:o1] = (torch.arange(o0, o1, device=DEV, dtype=torch.int64) % 251).to(torch.uint8)
    rc, got = _hist(view, n)
    assert rc == 0 and np.array_equal(got, _crt_counts(nb))
    small = 3 * 1000
    assert np.array_equal(C.hist3((np.arange(small) % 251).astype(np.uint8).reshape(-1, 3)), _crt_counts(small))


def test_hist_all_zero_image_of_more_than_2_to_32_pixels():
    n = 2 ** 32 + 48
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        reason = "%.1f GB free on the device, the 12.9 GB image of 2^32 + 48 pixels needs 16 GB" % (free / 2 ** 30)
        print(reason)
        pytest.skip(reason)
    img = torch.zeros(3 * n, device=DEV, dtype=torch.uint8)
    rc, got = _hist(img, n)
    del img
    assert rc == 0 and got[:, 0].tolist() == [n, n, n] and int(got[:, 1:].sum()) == 0


# ---------------------------------------------------------------------------------------------- lookup
def _lookup(a, so, do, table_dev):
    """src `so` bytes and dst `do` bytes into their storages, 32 guard bytes round dst.  Returns (rc, got, guards intact)."""
    n = a.size // 3
    _, src = _at_offset(a, so)
    store = torch.full((32 + do + a.size + 32 + 16,), 0xA5, device=DEV, dtype=torch.uint8)
    assert store.data_ptr() % 16 == 0
    lo = 32 + do
    dst = store[lo:lo + a.size]
    rc = _lut_call(src.data_ptr(), dst.data_ptr(), n, table_dev)
    host = store.cpu()
    intact = bool((host[:lo] == 0xA5).all()) and bool((host[lo + a.size:] == 0xA5).all())
    return rc, host[lo:lo + a.size].numpy(), intact and np.array_equal(src.cpu().numpy(), a)


def test_lut_small_sizes_at_every_pair_of_offsets(noise, tables):
    th, td = tables
    for n in SMALL:
        for so in range(16):
            for do in (0, 1, 2, 5, 15):
                a = noise[500 * so + do:][:3 * n]
                rc, got, intact = _lookup(a, so, do, td)
                want = C.apply_luts(a.reshape(-1, 3), th).reshape(-1)
                assert rc == 0 and intact and np.array_equal(got, want), (n, so, do)


def test_lut_every_shift_of_src_against_dst(noise, tables):
    th, td = tables
    n = 1000                                                     # 62 units: the funnel path with both end units
    a = noise[77:77 + 3 * n]
    want = C.apply_luts(a.reshape(-1, 3), th).reshape(-1)
    for so in range(16):
        for do in (0, 5):
            rc, got, intact = _lookup(a, so, do, td)
            assert rc == 0 and intact and np.array_equal(got, want), (so, do)


@pytest.mark.parametrize("n", [PASS - 1, PASS + 1, LUT_LAUNCH, LUT_LAUNCH + PASS + 1])
def test_lut_around_what_a_workgroup_and_the_grid_cover(noise, tables, n):
    th, td = tables
    a = noise[:3 * n]
    want = C.apply_luts(a.reshape(-1, 3), th).reshape(-1)
    for so, do in ((0, 0), (1, 2), (2, 1), (11, 0)):
        rc, got, intact = _lookup(a, so, do, td)
        assert rc == 0 and intact and np.array_equal(got, want), (so, do)


def test_lut_in_place_identity_empty_and_overlap(noise, tables):
    th, td = tables
    ident = torch.arange(256, dtype=torch.uint8).repeat(3).to(DEV)
    for n, off in ((33, 0), (33, 3), (1000, 7), (PASS + 5, 0), (PASS + 5, 9)):
        a = noise[13:13 + 3 * n]
        want = C.apply_luts(a.reshape(-1, 3), th).reshape(-1)
        store, view = _at_offset(a, 32 + off, pad=32)
        store[:32 + off] = 0xA5
        store[32 + off + 3 * n:] = 0xA5
        assert _lut_call(view.data_ptr(), view.data_ptr(), n, ident) == 0 and np.array_equal(view.cpu().numpy(), a)
        assert _lut_call(view.data_ptr(), view.data_ptr(), n, td) == 0           # in place == out of place
        host = store.cpu().numpy()
        assert np.array_equal(host[32 + off:32 + off + 3 * n], want), (n, off)
        assert (host[:32 + off] == 0xA5).all() and (host[32 + off + 3 * n:] == 0xA5).all()
    # n = 0: nothing is touched, whatever the pointers
    store = torch.full((64,), 0xA5, device=DEV, dtype=torch.uint8)
    assert _lut_call(store.data_ptr(), store.data_ptr() + 1, 0, td) == 0 and bool((store == 0xA5).all())
    # overlapping without being equal: refused, nothing written
    n = 100
    store, _ = _at_offset(noise[:6 * n + 64], 0)         # room for every refused range
    before = store.clone()
    for delta in (1, 3, 48, 3 * n - 1):
        assert _lut_call(store.data_ptr(), store.data_ptr() + delta, n, td) == -1
        assert _lut_call(store.data_ptr() + delta, store.data_ptr(), n, td) == -1
    assert torch.equal(store, before)
    assert _lut_call(store.data_ptr(), None, n, td) == -1


# ---------------------------------------------------------------------------------------------- the public functions
def _one_byte_in(host):
    store = torch.empty(host.size + 1, device=DEV, dtype=torch.uint8)
    view = store[1:].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize("H,W,shifted", [(41, 37, False), (41, 37, True), (97, 101, False), (97, 101, True)])
def test_remove_color_cast_and_scale_rgb_on_the_device(H, W, shifted):
    from gridnext_amd import imgprocess as IP
    a = C.tinted((H, W), seed=H + W)
    want = C.remove_color_cast_ref(a)
    assert np.array_equal(want, C.pillow_remove_color_cast(a)) and not np.array_equal(want, a)
    slide = _one_byte_in(a) if shifted else torch.from_numpy(a).to(DEV)
    got = IP.remove_color_cast(slide)
    assert got.device == slide.device and got.dtype == torch.uint8 and got.data_ptr() != slide.data_ptr()
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(slide.cpu(), torch.from_numpy(a))         # a resident slide passed with inplace=False is unchanged
    scales = (1.25, 0.5, -2.0)
    got = IP.scale_rgb(slide, *scales)
    assert torch.equal(got.cpu(), torch.from_numpy(C.scale_rgb_ref(a, scales)))
    assert torch.equal(got.cpu(), torch.from_numpy(C.pillow_scale_rgb(a, scales)))
    assert torch.equal(slide.cpu(), torch.from_numpy(a))
    r = IP.remove_color_cast(slide, inplace=True)                # the same storage
    assert r.data_ptr() == slide.data_ptr() and torch.equal(slide.cpu(), torch.from_numpy(want))


def test_device_refusals_come_before_any_write():
    from gridnext_amd import imgprocess as IP
    a = C.tinted((20, 20), seed=8)
    a[:, :, 1] = 0
    slide = torch.from_numpy(a).to(DEV)
    with pytest.raises(ValueError, match="green"):
        IP.remove_color_cast(slide, inplace=True)
    with pytest.raises(ValueError, match="finite"):
        IP.scale_rgb(slide, 1.0, float('nan'), 1.0, inplace=True)
    assert torch.equal(slide.cpu(), torch.from_numpy(a))
    wide = torch.from_numpy(np.concatenate([a, a], axis=1)).to(DEV)
    with pytest.raises(ValueError, match="contiguous"):
        IP.scale_rgb(wide[:, :20], 1.0, 1.0, 1.0, inplace=True)
    good = C.tinted((20, 20), seed=9)
    wide = torch.from_numpy(np.concatenate([good, good], axis=1)).to(DEV)
    assert torch.equal(IP.remove_color_cast(wide[:, :20]).cpu(), torch.from_numpy(C.remove_color_cast_ref(good)))


def _tree(tmp_path, name, rows):
    d = tmp_path / name / 'outs' / 'spatial'
    d.mkdir(parents=True)
    with open(str(d / 'tissue_positions.csv'), 'w') as fh:
        fh.write('barcode,in_tissue,array_row,array_col,pxl_row_in_fullres,pxl_col_in_fullres\n')
        for r in rows:
            fh.write('%s,%d,%d,%d,%s,%s\n' % r)
    return str(tmp_path / name)


def test_grid_with_remove_cast_equals_the_host_grid(tmp_path):
    from gridnext_amd import imgprocess as IP
    from gridnext_amd import transforms as T
    H, W = 41, 37
    a = C.tinted((H, W), seed=21)
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W // 3, H // 4), (2 * W // 3 + 1, H // 2 + 3), (5, H - 7)]
    rows = [('S%d-1' % i, 1, i, 2 * i + i % 2, y, x) for i, (x, y) in enumerate(pts)]          # (barcode, in, row, col, y_px, x_px)
    srd = _tree(tmp_path, 'cast', rows)
    norm = T.Normalize((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    resident = torch.from_numpy(a).to(DEV)
    for P, w in ((8, 12), (8, 8), (7, 9)):
        host = IP.grid_from_wsi_visium(a, srd, patch_size=P, window_size=w, remove_cast=True)
        plain = IP.grid_from_wsi_visium(a, srd, patch_size=P, window_size=w)
        assert not torch.equal(host, plain)
        for slide in (a, resident):                              # uploaded by the call (corrected in place), and resident
            raw = IP.grid_from_wsi_visium(slide, srd, patch_size=P, window_size=w, device=DEV, raw_uint8=True, remove_cast=True)
            assert raw.dtype == torch.uint8 and torch.equal(raw.cpu(), host.to(torch.uint8))
            assert int(raw.view(78, 64, -1).amax(-1).gt(0).sum()) == len(pts)
            flt = IP.grid_from_wsi_visium(slide, srd, patch_size=P, window_size=w, device=DEV, remove_cast=True)
            assert flt.dtype == torch.float32 and torch.equal(flt.cpu(), host)
            got = IP.grid_from_wsi_visium(slide, srd, patch_size=P, window_size=w, device=DEV, preprocess_xform=norm, remove_cast=True)
            want = IP.grid_from_wsi_visium(a, srd, patch_size=P, window_size=w, preprocess_xform=norm, remove_cast=True)
            assert torch.equal(got.cpu(), want)
        assert torch.equal(resident.cpu(), torch.from_numpy(a))  # the caller's tensor is never modified
        off = IP.grid_from_wsi_visium(resident, srd, patch_size=P, window_size=w, device=DEV, raw_uint8=True, remove_cast=False)
        assert torch.equal(off, IP.grid_from_wsi_visium(resident, srd, patch_size=P, window_size=w, device=DEV, raw_uint8=True))
        assert torch.equal(off.cpu(), plain.to(torch.uint8))
    d0, d1 = tmp_path / 'host', tmp_path / 'device'
    IP.save_visium_patches(a, srd, str(d0), patch_size=8, window_size=12, remove_cast=True)
    IP.save_visium_patches(resident, srd, str(d1), patch_size=8, window_size=12, device=DEV, remove_cast=True)
    assert sorted(os.listdir(str(d0))) == sorted(os.listdir(str(d1))) and len(os.listdir(str(d0))) == len(pts)
    for name in os.listdir(str(d0)):
        assert open(str(d0 / name), 'rb').read() == open(str(d1 / name), 'rb').read(), name
