"""gnx_patch_augment_u8 / gnx_patch_augment_u8_f32 / gnx_patch_grey_sum_u8 (csrc/augment.hip) through the C ABI against the CPU
form `transforms.augment_patches` / `grey_sums` (which tests/test_augment_ref_host.py pins to Pillow).  Every comparison is
torch.equal / np.array_equal - there is no tolerance in this file.

Shapes: P around 1, the dword (2, 3, 5), half a tile (31, 32, 33), the kernel's 64-byte LDS tile edge (63, 64, 65), two tiles
and an edge (130) and the tutorials' 224; n = 1, 2, 9 (all eight codes, scrambled, and one code >= 8) and 300, which at
P = 224 is 14 400 tile units, more than the 8 192 workgroups of the grid (the launcher does not chunk: further units are
reached by the grid stride); both operands aligned and one byte (one float) into their storage; one batch above 2^31 bytes."""
import numpy as np
import pytest
import torch

import augment_ref as R
from augment_ref import BAD_ARG, DEV, MAX_BLOCKS, SENTINEL, TILE, _at, _codes, _dev, _ptr

pytestmark = pytest.mark.gpu

PS = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 130, 224)
assert all(p in PS for p in (TILE - 1, TILE, TILE + 1))


def _augment(src, dst, n, P, dst_n, codes=None, luts=None, rows=None, norm=None, f32=False):
    from gridnext_amd import _lib as L
    args = (_ptr(src), _ptr(dst), n, P, dst_n, _ptr(codes), _ptr(luts), _ptr(rows))
    if f32:
        rc = L.query('gnx_patch_augment_u8_f32', *args, _ptr(norm), L.stream())
    else:
        rc = L.query('gnx_patch_augment_u8', *args, L.stream())
    torch.cuda.synchronize()
    return rc


def _luts(kind, n, seed):
    if kind == 'none':
        return None
    if kind == 'perm':
        return R.perm_tables(n, seed)
    if kind == 'identity':
        return np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8), (n, 3, 256)))
    return np.full((n, 3, 256), 77, dtype=np.uint8)


@pytest.mark.parametrize("P", PS)
def test_u8_form_every_code_table_and_alignment(P):
    from gridnext_amd import transforms as T
    assert 300 * 3 * (-(-224 // TILE)) ** 2 > MAX_BLOCKS
    for n in (1, 2, 9, 300):
        x = R.patches(n, P, seed=P + n)
        codes = _codes(n, seed=n)
        for kind in (('none', 'perm', 'identity', 'constant') if n <= 9 else ('none', 'perm')):
            luts = _luts(kind, n, seed=7 * n + P)
            want = T.augment_patches(x, codes, luts)
            if kind == 'identity':
                assert torch.equal(want, T.augment_patches(x, codes))
            if kind == 'constant':
                assert bool((want == 77).all())
            for so, do in ((0, 0), (1, 1)) + (((0, 1), (4, 0)) if n == 2 else ()):
                sstore, src = _at(x, so)
                dstore, dst = _at(torch.full_like(x, SENTINEL), do)
                tstore, tab = (None, None) if luts is None else _at(torch.from_numpy(luts), 3)
                rc = _augment(src, dst, n, P, n, _dev(codes, torch.uint8), tab)
                assert rc == 0
                assert torch.equal(dst.cpu().view(n, 3, P, P), want), (n, kind, so, do)
                assert torch.equal(src.cpu().view(n, 3, P, P), x)
                assert bool((dstore[:do] == SENTINEL).all()) and bool((dstore[do + dst.numel():] == SENTINEL).all())
        # codes == NULL: the identity (with a table: the table alone)
        sstore, src = _at(x, 1)
        dstore, dst = _at(torch.zeros_like(x), 0)
        assert _augment(src, dst, n, P, n) == 0 and torch.equal(dst.cpu().view(n, 3, P, P), x)


@pytest.mark.parametrize("P", PS)
def test_dst_rows_scatter_into_a_larger_sentinel_filled_destination(P):
    from gridnext_amd import transforms as T
    n, dst_n = 9, 14
    x = R.patches(n, P, seed=3 * P)
    codes, luts = _codes(n, seed=P), R.perm_tables(n, seed=P)
    rows = np.array([12, 3, -1, 0, dst_n, 13, 7, 5, 6], dtype=np.int32)        # -1 and dst_n: not written
    want = T.augment_patches(x, codes, luts)
    mean, std = (torch.tensor(v).reshape(3, 1, 1) for v in R.NORM)
    norm = torch.cat([torch.tensor(R.NORM[0]), torch.tensor(R.NORM[1]), 1.0 / torch.tensor(R.NORM[1])]).to(DEV)
    for f32 in (False, True):
        for so, do in ((0, 0), (1, 4 if f32 else 1)):
            fill = torch.full((dst_n, 3, P, P), SENTINEL, dtype=torch.uint8)
            if f32:
                fill = torch.full((dst_n, 3, P, P), -7.5)
            sstore, src = _at(x, so)
            dstore, dst = _at(fill, do)
            before = dstore.clone()
            rc = _augment(src, dst, n, P, dst_n, _dev(codes, torch.uint8), _dev(luts, torch.uint8), _dev(rows, torch.int32),
                          norm if f32 else None, f32)
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
    for n in (2, 9):
        x = R.patches(n, P, seed=5 * P + n)
        codes, luts = _codes(n, seed=n + 1), R.perm_tables(n, seed=n)
        for tab in (None, luts):
            bytes_out = torch.empty((n, 3, P, P), device=DEV, dtype=torch.uint8)
            sstore, src = _at(x, 0)
            assert _augment(src, bytes_out, n, P, n, _dev(codes, torch.uint8), _dev(tab, torch.uint8)) == 0
            assert torch.equal(bytes_out.cpu(), T.augment_patches(x, codes, tab))
            for nv in (None, norm):
                if P * P % 4 == 0:
                    want = torch.empty((n, 3, P, P), device=DEV, dtype=torch.float32)
                    L.call('gnx_u8_to_f32', bytes_out.data_ptr(), want.data_ptr(), n, 3, P, P, _ptr(nv), L.stream())
                    want = want.cpu()
                else:
                    want = bytes_out.cpu().float().div(255)
                    want = want if nv is None else (want - mean) / std
                assert torch.equal(want, T.augment_patches(x, codes, tab, out_float=True, norm=None if nv is None else R.NORM))
                for so, do in ((0, 0), (1, 4)):
                    sstore, src = _at(x, so)
                    dstore, dst = _at(torch.full((n, 3, P, P), -7.5), do)
                    rc = _augment(src, dst, n, P, n, _dev(codes, torch.uint8), _dev(tab, torch.uint8), None, nv, True)
                    assert rc == 0
                    assert torch.equal(dst.cpu().view(torch.float32).view(n, 3, P, P), want), (n, tab is None, nv is None, so, do)
                    assert torch.equal(src.cpu().view(n, 3, P, P), x)
                    assert bool((dstore[:do] == SENTINEL).all()) and bool((dstore[do + dst.numel():] == SENTINEL).all())


@pytest.mark.parametrize("P", PS)
def test_grey_sums(P):
    from gridnext_amd import _lib as L
    from gridnext_amd import transforms as T
    for n in (1, 9, 70) + ((MAX_BLOCKS + 3,) if P == 5 else ()):           # (more patches than the grid has workgroups)
        x = R.patches(n, P, seed=P + 11 * n)
        x[0] = 255
        white = torch.full((n, 3, P, P), 255, dtype=torch.uint8)
        for host in (x, white):
            want = T.grey_sums(host)
            for off in (0, 1):
                store, src = _at(host, off)
                sums = torch.full((n + 1,), -1, device=DEV, dtype=torch.int64)
                rc = L.query('gnx_patch_grey_sum_u8', src.data_ptr(), n, P, sums.data_ptr(), L.stream())
                torch.cuda.synchronize()
                assert rc == 0 and np.array_equal(sums[:n].cpu().numpy(), want) and int(sums[n]) == -1, (n, off)
                assert torch.equal(src.cpu().view(n, 3, P, P), host)
        assert int(want[0]) == 255 * P * P == int(want[-1])


def test_one_batch_above_two_to_the_31_bytes():
    from gridnext_amd import transforms as T
    n, P = 2731, 512
    assert n * 3 * P * P > 2 ** 31
    x = torch.randint(0, 256, (n, 3, P, P), device=DEV, dtype=torch.uint8)
    out = torch.empty_like(x)
    codes = _codes(n, seed=1)
    luts = np.ascontiguousarray(np.broadcast_to(R.perm_tables(8, seed=2)[None], (n // 8 + 1, 8, 3, 256)).reshape(-1, 3, 256)[:n])
    tail = x[-3:].cpu()
    assert _augment(x, out, n, P, n, _dev(codes, torch.uint8), _dev(luts, torch.uint8)) == 0
    assert torch.equal(out[-3:].cpu(), T.augment_patches(tail, codes[-3:], luts[-3:]))
    assert torch.equal(out[:2].cpu(), T.augment_patches(x[:2].cpu(), codes[:2], luts[:2]))
    assert torch.equal(x[-3:].cpu(), tail)
    from gridnext_amd import _lib as L
    s = torch.empty(n, device=DEV, dtype=torch.int64)
    L.call('gnx_patch_grey_sum_u8', x.data_ptr(), n, P, s.data_ptr(), L.stream())
    assert np.array_equal(s[-3:].cpu().numpy(), T.grey_sums(tail))


def test_nothing_to_do_and_every_refusal_leave_the_destination_alone():
    from gridnext_amd import _lib as L
    n, P = 4, 8
    x = R.patches(n, P, seed=0)
    sstore, src = _at(x, 0)
    dstore, dst = _at(torch.full((n, 3, P, P), SENTINEL, dtype=torch.uint8), 0)
    fstore, fdst = _at(torch.full((n, 3, P, P), -7.5), 0)
    rows = _dev(np.arange(n), torch.int32)

    def untouched():
        return bool((dstore == SENTINEL).all()) and bool((fdst.view(torch.float32) == -7.5).all()) and \
            torch.equal(src.cpu().view(n, 3, P, P), x)

    for f32, d in ((False, dst), (True, fdst)):
        assert _augment(src, d, 0, P, n, f32=f32) == 0 and _augment(None, None, 0, P, 0, f32=f32) == 0 and untouched()
        assert _augment(src, d, n, P, 0, rows=rows, f32=f32) == 0 and untouched()       # every row is outside
        assert _augment(None, d, n, P, n, f32=f32) == BAD_ARG and untouched()
        assert _augment(src, None, n, P, n, f32=f32) == BAD_ARG and untouched()
        assert _augment(src, d, n, 0, n, f32=f32) == BAD_ARG and _augment(src, d, n, -8, n, f32=f32) == BAD_ARG and untouched()
        assert _augment(src, d, n, P, n - 1, f32=f32) == BAD_ARG and untouched()          # dst_n < n, no dst_rows
        assert _augment(src, d, -1, P, n, f32=f32) == BAD_ARG and untouched()
    # overlap: in place, from below, from above, one byte of overlap at either end
    big = torch.full((3 * n * 3 * P * P,), SENTINEL, device=DEV, dtype=torch.uint8)
    nb = n * 3 * P * P
    mid = big[nb:2 * nb]
    mid.copy_(src)
    for off in (0, 1, -1, nb - 1, -(nb - 1), P * P):
        d = big[nb + off:2 * nb + off]
        assert _augment(mid, d, n, P, n) == BAD_ARG, off
        assert _augment(mid, d, n, P, n, rows=rows) == BAD_ARG, off
    for start in (nb - 8, nb // 2, nb + 4):                                # one patch as floats: nb bytes from `start`
        assert _augment(mid, big[start:], 1, P, 1, f32=True) == BAD_ARG, start
    assert torch.equal(mid, src) and bool((big[:nb] == SENTINEL).all()) and bool((big[2 * nb:] == SENTINEL).all())
    assert _augment(mid, big[:nb], n, P, n) == 0 and _augment(mid, big[2 * nb:], n, P, n) == 0      # touching ranges are fine
    assert torch.equal(big[:nb], mid) and torch.equal(big[2 * nb:], mid)
    # the grey sums
    sums = torch.full((n + 1,), -1, device=DEV, dtype=torch.int64)
    q = lambda *a: L.query('gnx_patch_grey_sum_u8', *a, L.stream())      # noqa: E731
    assert q(src.data_ptr(), 0, P, sums.data_ptr()) == 0 and q(None, 0, P, None) == 0
    assert q(None, n, P, sums.data_ptr()) == BAD_ARG and q(src.data_ptr(), n, P, None) == BAD_ARG
    assert q(src.data_ptr(), n, 0, sums.data_ptr()) == BAD_ARG and q(src.data_ptr(), n, P, sums.data_ptr() + 4) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((sums == -1).all()) and untouched()


def test_public_calls_on_device_tensors():
    """`augment_patches` and `Augment.apply` on HIP tensors against the same calls on CPU tensors, a grid-shaped `out`
    included; views that are not contiguous are copied first."""
    from gridnext_amd import transforms as T
    n, P = 13, 12
    x = R.patches(n, P, seed=9)
    codes, luts = _codes(n, seed=2), R.perm_tables(n, seed=3)
    rows = (np.arange(n) * 2 + 1).astype(np.int32)
    for kw in (dict(), dict(out_float=True), dict(out_float=True, norm=R.NORM)):
        want = T.augment_patches(x, codes, luts, **kw)
        got = T.augment_patches(x.to(DEV), codes, torch.from_numpy(luts).to(DEV), **kw)
        assert got.is_cuda and got.dtype == want.dtype and torch.equal(got.cpu(), want)
        grid = torch.zeros((4, 7, 3, P, P), dtype=want.dtype)
        T.augment_patches(x, codes, luts, out=grid, out_rows=rows, **kw)
        dgrid = torch.zeros((4, 7, 3, P, P), dtype=want.dtype, device=DEV)
        assert T.augment_patches(x.to(DEV), codes, luts, out=dgrid, out_rows=rows, **kw) is dgrid
        assert torch.equal(dgrid.cpu(), grid) and torch.equal(grid.view(28, 3, P, P)[rows.astype(np.int64)], want)
        aug = T.Augment([T.RandomHorizontalFlip(), T.RandomVerticalFlip(), T.RandomQuarterTurn(), T.ColorJitter(0.4, 0.6)], seed=6)
        host = aug.apply(x, **kw)
        dev = aug.manual_seed(6).apply(x.to(DEV), **kw)
        assert torch.equal(dev.cpu(), host) and not torch.equal(host, T.augment_patches(x, None, None, **kw))
    wide = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (n, 3, P, 2 * P), dtype=np.uint8))
    assert torch.equal(T.augment_patches(wide.to(DEV)[..., :P], codes).cpu(), T.augment_patches(wide[..., :P], codes))
    with pytest.raises(ValueError, match="out"):
        T.augment_patches(x.to(DEV), out=torch.zeros((n, 3, P, P), dtype=torch.uint8))
