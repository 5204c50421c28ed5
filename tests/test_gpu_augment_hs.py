"""gnx_patch_augment_hs_u8 / gnx_patch_augment_hs_u8_f32 (csrc/augment.hip) through the C ABI against the CPU form
`transforms.augment_patches(sat=, hue=)` and the numpy restatement behind it (which tests/test_augment_hs_ref_host.py pins to
Pillow on all 2^24 colours).  Every comparison is torch.equal - there is no tolerance in this file.

The all-colours cases are exhaustive: 256 patches of 256 x 256 hold every colour once, and every saturation factor and every
hue shift of tests/augment_hs_ref.py sees all of them.  The edge sizes sit around the dword (1..5), the 64-pixel tile (63, 64,
65, 67) and two tiles (128, 130); n = 9 carries all eight codes, scrambled, and one code >= 8; n = 8195 at P = 3 is more tile
units than the 8 192 workgroups of the grid, so the last ones are reached by the grid stride."""
import numpy as np
import pytest
import torch

import augment_hs_ref as H
import augment_ref as R
from augment_ref import BAD_ARG, DEV, MAX_BLOCKS, SENTINEL, TILE, _at, _codes, _dev, _ptr

pytestmark = pytest.mark.gpu

PS = (1, 2, 3, 4, 5, 63, 64, 65, 67, 128, 130)


def _hs(src, dst, n, P, dst_n, codes=None, luts=None, sat=None, hue=None, rows=None, norm=None, f32=False):
    from gridnext_amd import _lib as L
    args = (_ptr(src), _ptr(dst), n, P, dst_n, _ptr(codes), _ptr(luts), _ptr(sat), _ptr(hue), _ptr(rows))
    if f32:
        rc = L.query('gnx_patch_augment_hs_u8_f32', *args, _ptr(norm), L.stream())
    else:
        rc = L.query('gnx_patch_augment_hs_u8', *args, L.stream())
    torch.cuda.synchronize()
    return rc


def _factors(n, seed):
    """Saturation factors inside, at the ends of and outside [0, 1], and hue shifts, one per patch."""
    rng = np.random.default_rng(seed)
    sat = np.concatenate([np.array(H.SAT_FACTORS), rng.uniform(0.0, 3.0, n)])[:n].astype(np.float32)
    hue = np.concatenate([np.array(H.SHIFTS), rng.integers(0, 256, n)])[:n].astype(np.uint8)
    return rng.permutation(sat), rng.permutation(hue)


@pytest.fixture(scope='module')
def colours():
    """(the 256 all-colours patches on the device, the same as (256, 256, 256, 3) numpy)."""
    x = H.all_colours()
    return x.to(DEV), H.to_hwc(x)


def _run_colours(xd, sat=None, hue=None, codes=None):
    out = torch.full_like(xd, SENTINEL)
    assert _hs(xd, out, 256, 256, 256, _dev(codes, torch.uint8), None, _dev(sat, torch.float32), _dev(hue, torch.uint8)) == 0
    return out.cpu()


@pytest.mark.parametrize("f", H.SAT_FACTORS)
def test_all_colours_saturation(colours, f):
    xd, a = colours
    got = _run_colours(xd, sat=np.full(256, f))
    want = H.to_chw(H.saturate(a, np.float32(f)))
    bad = int((got != want).any(1).sum())
    print("saturation %r: %d of 2^24 colours differ" % (f, bad))
    assert bad == 0 and torch.equal(got, want)


@pytest.mark.parametrize("shift", H.SHIFTS)
def test_all_colours_hue(colours, shift):
    xd, a = colours
    got = _run_colours(xd, hue=np.full(256, shift))
    want = H.to_chw(H.table_hue(a, shift))
    bad = int((got != want).any(1).sum())
    print("hue shift %d: %d of 2^24 colours differ" % (shift, bad))
    assert bad == 0 and torch.equal(got, want)


def test_all_colours_mixed_shifts_and_codes_in_one_launch(colours):
    xd, a = colours
    shifts = np.array([H.SHIFTS[k % len(H.SHIFTS)] for k in range(256)], dtype=np.uint8)
    codes = R.scrambled_codes(256, seed=3)
    got = _run_colours(xd, hue=shifts, codes=codes)
    want = H.to_chw(H.table_hue(a, shifts.reshape(-1, 1, 1)))
    want = torch.stack([R.torch_code(want[k], int(codes[k])) for k in range(256)])
    assert torch.equal(got, want)


def test_all_colours_saturation_then_hue(colours):
    xd, a = colours
    fs = np.where(np.arange(256) % 2 == 0, 0.77, 1.4).astype(np.float32)
    got = _run_colours(xd, sat=fs, hue=np.full(256, 43))
    want = H.to_chw(H.table_hue(H.saturate(a, fs.reshape(-1, 1, 1)), 43))
    bad = int((got != want).any(1).sum())
    print("saturation 0.77 / 1.4, then hue shift 43: %d of 2^24 colours differ" % bad)
    assert bad == 0
    # the order matters, and the kernel's is saturation first
    assert not torch.equal(want[:2], H.to_chw(H.saturate(H.table_hue(a[:2], 43), fs[:2].reshape(-1, 1, 1))))


@pytest.mark.parametrize("P", PS)
def test_every_code_with_and_without_tables_at_the_edge_sizes(P):
    from gridnext_amd import transforms as T
    n = 9
    x = R.patches(n, P, seed=P)
    codes = _codes(n, seed=P + 1)
    sat, hue = _factors(n, seed=P + 2)
    for luts in (None, R.perm_tables(n, seed=P + 3)):
        want = T.augment_patches(x, codes, luts, sat=sat, hue=hue)
        assert not torch.equal(want, T.augment_patches(x, codes, luts))
        for so, do in ((0, 0), (1, 1), (0, 1), (4, 0)):
            sstore, src = _at(x, so)
            dstore, dst = _at(torch.full_like(x, SENTINEL), do)
            tstore, tab = (None, None) if luts is None else _at(torch.from_numpy(luts), 3)
            hstore, hd = _at(torch.from_numpy(hue), 1)
            rc = _hs(src, dst, n, P, n, _dev(codes, torch.uint8), tab, _dev(sat, torch.float32), hd)
            assert rc == 0
            assert torch.equal(dst.cpu().view(n, 3, P, P), want), (luts is None, so, do)
            assert torch.equal(src.cpu().view(n, 3, P, P), x)
            assert bool((dstore[:do] == SENTINEL).all()) and bool((dstore[do + dst.numel():] == SENTINEL).all())


@pytest.mark.parametrize("P", (5, 64, 67))
def test_absent_stages(P):
    from gridnext_amd import _lib as L
    from gridnext_amd import transforms as T
    n = 9
    x = R.patches(n, P, seed=2 * P)
    codes, luts = _codes(n, seed=P), R.perm_tables(n, seed=P)
    sat, hue = _factors(n, seed=P)
    xd, cd, ld, sd, hd = x.to(DEV), _dev(codes, torch.uint8), _dev(luts, torch.uint8), _dev(sat, torch.float32), _dev(hue, torch.uint8)
    results = {}
    for s in (None, sd):
        for h in (None, hd):
            for tab in (None, ld):
                out = torch.full_like(xd, SENTINEL)
                assert _hs(xd, out, n, P, n, cd, tab, s, h) == 0
                want = T.augment_patches(x, codes, None if tab is None else luts, sat=None if s is None else sat,
                                         hue=None if h is None else hue)
                assert torch.equal(out.cpu(), want), (s is None, h is None, tab is None)
                results[(s is None, h is None, tab is None)] = out
                if s is None and h is None:                                  # both NULL: the plain entry point's result
                    plain = torch.full_like(xd, SENTINEL)
                    rc = L.query('gnx_patch_augment_u8', xd.data_ptr(), plain.data_ptr(), n, P, n, cd.data_ptr(), _ptr(tab),
                                 None, L.stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and torch.equal(out, plain)
    assert len({r.cpu().numpy().tobytes() for r in results.values()}) == 8
    # a present hue stage makes the round trip at shift 0 too, and the round trip is lossy
    out = torch.empty_like(xd)
    assert _hs(xd, out, n, P, n, hue=torch.zeros(n, dtype=torch.uint8, device=DEV)) == 0
    assert torch.equal(out.cpu(), T.augment_patches(x, hue=np.zeros(n, dtype=np.uint8))) and not torch.equal(out, xd)


@pytest.mark.parametrize("P", (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 67, 128, 130))
def test_both_stages_absent_equals_the_plain_entry_points_in_every_form(P):
    """The three-plane and the one-plane instantiation share the mover's offset arithmetic: with sat == hue == NULL their
    destinations are equal byte for byte, storage around the tensor included - bytes and floats (with and without norm), with
    and without tables, contiguous and scattered into a larger destination, aligned and off their alignment."""
    from gridnext_amd import _lib as L
    n, dst_n = 9, 14
    x = R.patches(n, P, seed=7 * P)
    cd = _dev(_codes(n, seed=P + 2), torch.uint8)
    ld = _dev(R.perm_tables(n, seed=P + 4), torch.uint8)
    rd = _dev(np.array([12, 3, -1, 0, dst_n, 13, 7, 5, 6]), torch.int32)        # -1 and dst_n: not written
    norm = torch.cat([torch.tensor(R.NORM[0]), torch.tensor(R.NORM[1]), 1.0 / torch.tensor(R.NORM[1])]).to(DEV)
    for f32, nv in ((False, None), (True, None), (True, norm)):
        for tab in (None, ld):
            for rows, rows_n in ((None, n), (rd, dst_n)):
                for so, do in ((0, 0), (1, 4 if f32 else 1)):
                    fill = torch.full((rows_n, 3, P, P), -7.5) if f32 else torch.full((rows_n, 3, P, P), SENTINEL, dtype=torch.uint8)
                    sstore, src = _at(x, so)
                    hstore, hdst = _at(fill, do)
                    pstore, pdst = _at(fill, do)
                    assert _hs(src, hdst, n, P, rows_n, cd, tab, None, None, rows, nv, f32) == 0
                    args = (src.data_ptr(), pdst.data_ptr(), n, P, rows_n, cd.data_ptr(), _ptr(tab), _ptr(rows))
                    if f32:
                        rc = L.query('gnx_patch_augment_u8_f32', *args, _ptr(nv), L.stream())
                    else:
                        rc = L.query('gnx_patch_augment_u8', *args, L.stream())
                    torch.cuda.synchronize()
                    case = (f32, nv is None, tab is None, rows is None, so, do)
                    assert rc == 0 and torch.equal(hstore, pstore), case
                    assert not torch.equal(hdst.cpu(), fill.view(torch.uint8).reshape(-1)), case       # something was written
                    assert torch.equal(src.cpu().view(n, 3, P, P), x), case


def test_one_batch_above_two_to_the_31_bytes_through_the_three_plane_kernel():
    from gridnext_amd import transforms as T
    n, P = 2731, 512
    assert n * 3 * P * P > 2 ** 31
    x = torch.randint(0, 256, (n, 3, P, P), device=DEV, dtype=torch.uint8)
    out = torch.empty_like(x)
    codes = _codes(n, seed=1)
    luts = np.ascontiguousarray(np.broadcast_to(R.perm_tables(8, seed=2)[None], (n // 8 + 1, 8, 3, 256)).reshape(-1, 3, 256)[:n])
    sat, hue = _factors(n, seed=3)
    tail = x[-3:].cpu()
    assert _hs(x, out, n, P, n, _dev(codes, torch.uint8), _dev(luts, torch.uint8), _dev(sat, torch.float32),
               _dev(hue, torch.uint8)) == 0
    assert torch.equal(out[-3:].cpu(), T.augment_patches(tail, codes[-3:], luts[-3:], sat=sat[-3:], hue=hue[-3:]))
    assert torch.equal(out[:2].cpu(), T.augment_patches(x[:2].cpu(), codes[:2], luts[:2], sat=sat[:2], hue=hue[:2]))
    assert torch.equal(x[-3:].cpu(), tail)


def test_more_units_than_workgroups_and_n_300_at_p_67():
    from gridnext_amd import transforms as T
    for n, P in ((300, 67), (MAX_BLOCKS + 3, 3)):
        units = n * (-(-P // TILE)) ** 2
        assert units > 1024 and (P != 3 or units > MAX_BLOCKS)
        x = R.patches(n, P, seed=n)
        codes, luts = _codes(n, seed=1), R.perm_tables(n, seed=2)
        sat, hue = _factors(n, seed=3)
        want = T.augment_patches(x, codes, luts, sat=sat, hue=hue)
        for so, do in ((0, 0), (1, 1)):
            sstore, src = _at(x, so)
            dstore, dst = _at(torch.full_like(x, SENTINEL), do)
            rc = _hs(src, dst, n, P, n, _dev(codes, torch.uint8), _dev(luts, torch.uint8), _dev(sat, torch.float32),
                     _dev(hue, torch.uint8))
            assert rc == 0 and torch.equal(dst.cpu().view(n, 3, P, P), want), (n, P, so, do)
            assert bool((dstore[:do] == SENTINEL).all()) and bool((dstore[do + dst.numel():] == SENTINEL).all())


@pytest.mark.parametrize("P", (3, 64, 67))
def test_dst_rows_scatter_into_a_larger_sentinel_filled_destination(P):
    from gridnext_amd import transforms as T
    n, dst_n = 9, 14
    x = R.patches(n, P, seed=3 * P)
    codes, luts = _codes(n, seed=P), R.perm_tables(n, seed=P)
    sat, hue = _factors(n, seed=P + 5)
    rows = np.array([12, 3, -1, 0, dst_n, 13, 7, 5, 6], dtype=np.int32)        # -1 and dst_n: not written
    want = T.augment_patches(x, codes, luts, sat=sat, hue=hue)
    mean, std = (torch.tensor(v).reshape(3, 1, 1) for v in R.NORM)
    norm = torch.cat([torch.tensor(R.NORM[0]), torch.tensor(R.NORM[1]), 1.0 / torch.tensor(R.NORM[1])]).to(DEV)
    for f32 in (False, True):
        for so, do in ((0, 0), (1, 4 if f32 else 1)):
            fill = torch.full((dst_n, 3, P, P), -7.5) if f32 else torch.full((dst_n, 3, P, P), SENTINEL, dtype=torch.uint8)
            sstore, src = _at(x, so)
            dstore, dst = _at(fill, do)
            before = dstore.clone()
            rc = _hs(src, dst, n, P, dst_n, _dev(codes, torch.uint8), _dev(luts, torch.uint8), _dev(sat, torch.float32),
                     _dev(hue, torch.uint8), _dev(rows, torch.int32), norm if f32 else None, f32)
            assert rc == 0
            got = dst.cpu().view(torch.float32 if f32 else torch.uint8).view(dst_n, 3, P, P)
            written = set()
            for k in range(n):
                if 0 <= rows[k] < dst_n:
                    written.add(int(rows[k]))
                    w = (want[k].float().div(255) - mean) / std if f32 else want[k]
                    assert torch.equal(got[rows[k]], w), (f32, k)
            assert len(written) == 7
            for row in set(range(dst_n)) - written:
                assert torch.equal(got[row], fill[row]), (f32, row)
            assert torch.equal(dstore[:do], before[:do]) and torch.equal(dstore[do + dst.numel():], before[do + dst.numel():])
            assert torch.equal(src.cpu().view(n, 3, P, P), x)


@pytest.mark.parametrize("P", PS)
def test_f32_form_is_u8_to_f32_of_the_u8_form(P):
    from gridnext_amd import _lib as L
    from gridnext_amd import transforms as T
    mean, std = (torch.tensor(v).reshape(1, 3, 1, 1) for v in R.NORM)
    norm = torch.cat([torch.tensor(R.NORM[0]), torch.tensor(R.NORM[1]), 1.0 / torch.tensor(R.NORM[1])]).to(DEV)
    n = 9
    x = R.patches(n, P, seed=5 * P)
    codes, luts = _codes(n, seed=P + 1), R.perm_tables(n, seed=P)
    sat, hue = _factors(n, seed=P + 7)
    cd, sd, hd = _dev(codes, torch.uint8), _dev(sat, torch.float32), _dev(hue, torch.uint8)
    for tab in (None, luts):
        bytes_out = torch.empty((n, 3, P, P), device=DEV, dtype=torch.uint8)
        sstore, src = _at(x, 0)
        assert _hs(src, bytes_out, n, P, n, cd, _dev(tab, torch.uint8), sd, hd) == 0
        assert torch.equal(bytes_out.cpu(), T.augment_patches(x, codes, tab, sat=sat, hue=hue))
        for nv in (None, norm):
            if P * P % 4 == 0:
                want = torch.empty((n, 3, P, P), device=DEV, dtype=torch.float32)
                L.call('gnx_u8_to_f32', bytes_out.data_ptr(), want.data_ptr(), n, 3, P, P, _ptr(nv), L.stream())
                want = want.cpu()
            else:
                want = bytes_out.cpu().float().div(255)
                want = want if nv is None else (want - mean) / std
            assert torch.equal(want, T.augment_patches(x, codes, tab, out_float=True, norm=None if nv is None else R.NORM,
                                                       sat=sat, hue=hue))
            for so, do in ((0, 0), (1, 4)):
                sstore, src = _at(x, so)
                dstore, dst = _at(torch.full((n, 3, P, P), -7.5), do)
                rc = _hs(src, dst, n, P, n, cd, _dev(tab, torch.uint8), sd, hd, None, nv, True)
                assert rc == 0
                assert torch.equal(dst.cpu().view(torch.float32).view(n, 3, P, P), want), (tab is None, nv is None, so, do)
                assert torch.equal(src.cpu().view(n, 3, P, P), x)
                assert bool((dstore[:do] == SENTINEL).all()) and bool((dstore[do + dst.numel():] == SENTINEL).all())


def test_constant_grey_and_black_patches():
    """Factor 0 and factor 1, grey patches and black patches (maxc == 0: no division may reach the bytes)."""
    from gridnext_amd import transforms as T
    P = 6
    x = R.patches(6, P, seed=1)
    x[1] = 0                                                                 # black
    x[2] = 255                                                               # white
    x[3] = x[3, :1].clone().expand(3, P, P)                                  # grey pixels, each its own value
    x[4] = 77                                                                # a constant grey patch
    x[5, 1:] = 0                                                             # pure reds: s = 255
    n = 6
    for fs in (0.0, 1.0, 0.5, 2.0):
        for shift in (0, 128, 255):
            sat, hue = np.full(n, fs, dtype=np.float32), np.full(n, shift, dtype=np.uint8)
            out = torch.full((n, 3, P, P), SENTINEL, device=DEV, dtype=torch.uint8)
            assert _hs(x.to(DEV), out, n, P, n, None, None, _dev(sat, torch.float32), _dev(hue, torch.uint8)) == 0
            got = out.cpu()
            assert torch.equal(got, T.augment_patches(x, sat=sat, hue=hue)), (fs, shift)
            assert torch.equal(got[1:5], x[1:5]), (fs, shift)                # grey pixels have no saturation and no hue
            if fs == 0.0:
                assert bool((got[:, 0] == got[:, 1]).all()) and bool((got[:, 1] == got[:, 2]).all())
        sat = np.full(n, fs, dtype=np.float32)
        out = torch.full((n, 3, P, P), SENTINEL, device=DEV, dtype=torch.uint8)
        assert _hs(x.to(DEV), out, n, P, n, sat=_dev(sat, torch.float32)) == 0
        assert torch.equal(out.cpu(), T.augment_patches(x, sat=sat)) and (fs != 1.0 or torch.equal(out.cpu(), x))


def test_nothing_to_do_and_every_refusal_leave_the_destination_alone():
    n, P = 4, 8
    x = R.patches(n, P, seed=0)
    sstore, src = _at(x, 0)
    dstore, dst = _at(torch.full((n, 3, P, P), SENTINEL, dtype=torch.uint8), 0)
    fstore, fdst = _at(torch.full((n, 3, P, P), -7.5), 0)
    rows = _dev(np.arange(n), torch.int32)
    satstore, sat = _at(torch.full((n,), 0.5), 0)
    hue = torch.full((n,), 9, dtype=torch.uint8, device=DEV)

    def untouched():
        return bool((dstore == SENTINEL).all()) and bool((fdst.view(torch.float32) == -7.5).all()) and \
            torch.equal(src.cpu().view(n, 3, P, P), x)

    for f32, d in ((False, dst), (True, fdst)):
        kw = dict(sat=sat, hue=hue, f32=f32)
        assert _hs(src, d, 0, P, n, **kw) == 0 and _hs(None, None, 0, P, 0, **kw) == 0 and untouched()
        assert _hs(src, d, n, P, 0, rows=rows, **kw) == 0 and untouched()          # every row is outside
        assert _hs(None, d, n, P, n, **kw) == BAD_ARG and untouched()
        assert _hs(src, None, n, P, n, **kw) == BAD_ARG and untouched()
        assert _hs(src, d, n, 0, n, **kw) == BAD_ARG and _hs(src, d, n, -8, n, **kw) == BAD_ARG and untouched()
        assert _hs(src, d, n, P, n - 1, **kw) == BAD_ARG and untouched()             # dst_n < n, no dst_rows
        assert _hs(src, d, -1, P, n, **kw) == BAD_ARG and untouched()
        assert _hs(src, d, n, P, -1, rows=rows, **kw) == BAD_ARG and untouched()
        assert _hs(src, d, n, 32769, n, **kw) == -3 and untouched()                  # GNX_ERR_UNSUPPORTED: P > 32768
        for off in (1, 2, 3):                                                        # a factor vector off its 4 bytes
            assert _hs(src, d, n, P, n, sat=satstore[off:], hue=hue, f32=f32) == BAD_ARG and untouched()
    assert _hs(src, fstore[1:], n, P, n, sat=sat, hue=hue, f32=True) == BAD_ARG and untouched()      # floats off their 4 bytes
    # overlap: in place, from below, from above, one byte of overlap at either end
    big = torch.full((3 * n * 3 * P * P,), SENTINEL, device=DEV, dtype=torch.uint8)
    nb = n * 3 * P * P
    mid = big[nb:2 * nb]
    mid.copy_(src)
    for off in (0, 1, -1, nb - 1, -(nb - 1), P * P):
        d = big[nb + off:2 * nb + off]
        assert _hs(mid, d, n, P, n, sat=sat, hue=hue) == BAD_ARG, off
        assert _hs(mid, d, n, P, n, sat=sat, hue=hue, rows=rows) == BAD_ARG, off
    for start in (nb - 8, nb // 2, nb + 4):                                # one patch as floats: nb bytes from `start`
        assert _hs(mid, big[start:], 1, P, 1, sat=sat, hue=hue, f32=True) == BAD_ARG, start
    assert torch.equal(mid, src) and bool((big[:nb] == SENTINEL).all()) and bool((big[2 * nb:] == SENTINEL).all())
    assert _hs(mid, big[:nb], n, P, n) == 0 and _hs(mid, big[2 * nb:], n, P, n) == 0                # touching ranges are fine
    assert torch.equal(big[:nb], mid) and torch.equal(big[2 * nb:], mid) and untouched()


def test_public_calls_on_device_tensors():
    """`augment_patches(sat=, hue=)` and `Augment.apply` with a SaturationHueJitter on HIP tensors against the same calls on
    CPU tensors, a grid-shaped `out` included."""
    from gridnext_amd import transforms as T
    n, P = 13, 12
    x = R.patches(n, P, seed=9)
    codes, luts = _codes(n, seed=2), R.perm_tables(n, seed=3)
    sat, hue = _factors(n, seed=4)
    rows = (np.arange(n) * 2 + 1).astype(np.int32)
    for kw in (dict(), dict(out_float=True), dict(out_float=True, norm=R.NORM)):
        for sh in (dict(sat=sat), dict(hue=hue), dict(sat=sat.astype(np.float64), hue=torch.from_numpy(hue).to(DEV))):
            want = T.augment_patches(x, codes, luts, **kw, **{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sh.items()})
            got = T.augment_patches(x.to(DEV), codes, torch.from_numpy(luts).to(DEV), **kw, **sh)
            assert got.is_cuda and got.dtype == want.dtype and torch.equal(got.cpu(), want)
            dgrid = torch.zeros((4, 7, 3, P, P), dtype=want.dtype, device=DEV)
            assert T.augment_patches(x.to(DEV), codes, luts, out=dgrid, out_rows=rows, **kw, **sh) is dgrid
            assert torch.equal(dgrid.view(28, 3, P, P)[rows.astype(np.int64)].cpu(), want)
            assert not bool(dgrid.view(28, 3, P, P)[0::2].any())
        for steps in ([T.SaturationHueJitter(0.4, 0.1)], [T.RandomQuarterTurn(), T.SaturationHueJitter(hue=(-0.5, 0.5))],
                      [T.RandomHorizontalFlip(), T.ColorJitter(0.4, 0.6), T.RandomVerticalFlip(), T.SaturationHueJitter((0.2, 1.8))]):
            aug = T.Augment(steps, seed=6)
            host = aug.apply(x, **kw)
            dev = aug.manual_seed(6).apply(x.to(DEV), **kw)
            assert torch.equal(dev.cpu(), host) and not torch.equal(host, T.augment_patches(x, None, None, **kw))
