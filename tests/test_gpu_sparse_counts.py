"""csrc/sparse_counts.hip through the C ABI against the numpy restatement (tests/sparse_counts_ref.py): expand (bit for bit,
into a buffer pre-filled with NaN), the two divisions (numpy's float32 bits), the line moments (exact on integers, within the
derived bound of math.fsum otherwise, equal bits on a second call), log1p (in ulps of float64's log1p, against 4 x numpy's own
float32 error on the same inputs) and every refusal.

Measured on an MI355X (printed by the tests): see the README's sparse-count section."""
import numpy as np
import pytest
import torch

import sparse_counts_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [0, 1, 63, 64, 65, 257, 0, 300]
SIZES = [1, 63, 64, 65, 4992, 8191, 8192, 8193, 16389]


def _L():
    from gridnext_amd import _lib
    return _lib


def _offset(array, dtype):
    """The array on the device, one element into its storage."""
    t = torch.empty(len(array) + 1, dtype=dtype, device=DEV)
    t[1:] = torch.from_numpy(np.ascontiguousarray(array)).to(DEV)
    return t[1:]


def _dev(array):
    return None if array is None else torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def _expand(ptr, idx, val, lines, n_lines, pos, L, ld_out, offset=True):
    lib = _L()
    d_ptr, d_lines, d_pos = _dev(ptr), _dev(lines), _dev(pos)
    d_idx = _offset(idx, torch.int32) if offset else _dev(idx)
    d_val = _offset(val, torch.float32) if offset else _dev(val)
    store = torch.full((n_lines * ld_out + 1 + 8,), float('nan'), dtype=torch.float32, device=DEV)
    out = store[1:1 + n_lines * ld_out] if offset else store[:n_lines * ld_out]
    lib.call('gnx_sparse_expand_f32', lib.ptr(d_ptr, torch.int64), lib.ptr(d_idx, torch.int32), lib.ptr(d_val),
             lib.ptr(d_lines, torch.int32), n_lines, lib.ptr(d_pos, torch.int32), out.data_ptr(), ld_out, L, lib.stream())
    torch.cuda.synchronize()
    assert torch.isnan(store[:1]).all() or not offset
    assert torch.isnan(store[(1 if offset else 0) + n_lines * ld_out:]).all()            # nothing behind the last row
    return out.cpu().numpy().reshape(n_lines, ld_out)


def _same(got, want):
    return torch.equal(torch.from_numpy(got).view(torch.int32), torch.from_numpy(want).view(torch.int32))     # NaN padding too


@pytest.mark.parametrize("L", SIZES)
def test_expand_equals_the_restatement(L):
    """Lines of 0, 1, 63, 64, 65, 257 entries (as many as L allows), out / val / idx one element into their storage: identity
    map, a permutation, lines repeated and reversed, ld_out > L with the padding untouched, an all -1 map."""
    rng = np.random.default_rng(L)
    lengths = [min(n, L) for n in LENGTHS]
    ptr, idx, val = R.random_lines(rng, lengths, L)
    n = len(lengths)
    got = _expand(ptr, idx, val, None, n, None, L, L)
    assert _same(got, R.expand(ptr, idx, val, None, n, None, L))
    assert [int((got[i] != 0).sum()) for i in range(n)] == lengths
    perm = rng.permutation(L).astype(np.int32)
    lines = np.array([n - 1 - i for i in range(n)] + [5, 5, 2], dtype=np.int32)             # reversed, then repeats
    for ld in (L, L + 3):
        got = _expand(ptr, idx, val, lines, len(lines), perm, L, ld)
        assert _same(got, R.expand(ptr, idx, val, lines, len(lines), perm, L, ld))
        assert np.isnan(got[:, L:]).all() and not np.isnan(got[:, :L]).any()
    none = np.full(L, -1, dtype=np.int32)
    assert _same(_expand(ptr, idx, val, lines, len(lines), none, L, L + 1),
                 R.expand(ptr, idx, val, lines, len(lines), none, L, L + 1))
    got = _expand(ptr, idx, val, None, n, None, L, L, offset=False)                         # 16-byte aligned rows where L allows
    assert _same(got, R.expand(ptr, idx, val, None, n, None, L))


def test_expand_drops_what_maps_outside_and_takes_both_uses():
    """A map into fewer positions than indices (gene -> channel with unselected genes; spot -> cell of a grid), positions at or
    beyond L dropped, and n_lines == 0."""
    rng = np.random.default_rng(7)
    ptr, idx, val = R.random_lines(rng, [257, 64, 0, 65, 300, 1], 400)
    pos = np.full(400, -1, dtype=np.int32)
    chosen = rng.choice(400, size=130, replace=False)
    pos[chosen] = rng.permutation(150)[:130]                                                 # some land at >= L = 140: dropped
    got = _expand(ptr, idx, val, None, 6, pos, 140, 144)
    assert _same(got, R.expand(ptr, idx, val, None, 6, pos, 140, 144))
    lib = _L()
    out = torch.full((4,), float('nan'), device=DEV)
    rc = lib.query('gnx_sparse_expand_f32', lib.ptr(_dev(ptr), torch.int64), None, None, None, 0, None, out.data_ptr(), 4, 4,
                   lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.isnan(out).all()


def test_divisions_are_numpys_float32_bits():
    lib = _L()
    rng = np.random.default_rng(2)
    lengths = LENGTHS + [1] * 12 + list(rng.integers(0, 400, 200))
    ptr, idx, val = R.random_lines(rng, lengths, 500)
    mask = rng.random(500) < 0.5                                                             # totals over a gene selection
    totals = np.bincount(np.repeat(np.arange(len(lengths)), lengths), weights=val * mask[idx], minlength=len(lengths))
    d = np.where(totals == 0, np.float32(1), totals.astype(np.float32) / np.float32(1e4)).astype(np.float32)
    assert ((totals == 0) & (np.array(lengths) > 0)).sum() >= 2                              # zero totals on lines with entries
    d_val, d_ptr, d_div = _offset(val, torch.float32), _dev(ptr), _offset(d, torch.float32)
    lib.call('gnx_sparse_div_by_line_f32', lib.ptr(d_ptr, torch.int64), lib.ptr(d_val), len(lengths), lib.ptr(d_div), lib.stream())
    want = R.div_by_line(ptr, val, d)
    assert torch.equal(d_val.cpu(), torch.from_numpy(want))
    # odd divisors, denormal and huge quotients; the other addressing
    per_idx = np.concatenate([rng.random(250).astype(np.float32) * 3 + 1e-3, np.float32(10.0) ** rng.integers(-30, 30, 250)])
    per_idx = per_idx.astype(np.float32)
    vals = (val * np.float32(10.0) ** rng.integers(-20, 10, len(val)).astype(np.float32)).astype(np.float32)
    d_val, d_idx, d_div = _offset(vals, torch.float32), _offset(idx, torch.int32), _offset(per_idx, torch.float32)
    lib.call('gnx_sparse_div_by_idx_f32', lib.ptr(d_idx, torch.int32), lib.ptr(d_val), len(vals), lib.ptr(d_div), lib.stream())
    with np.errstate(over='ignore', under='ignore'):
        want = R.div_by_idx(idx, vals, per_idx)
    got = d_val.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (np.abs(want) < 2.0 ** -126).any() and np.isinf(want).any()                     # denormal and overflowed quotients


def _moments(ptr, idx, val, lines, n_lines, mask):
    lib = _L()
    out = torch.full((n_lines, 2), float('nan'), dtype=torch.float64, device=DEV)
    args = (_dev(ptr), _offset(idx, torch.int32), _offset(val, torch.float32), _dev(lines), _dev(mask))
    lib.call('gnx_sparse_line_moments_f64', lib.ptr(args[0], torch.int64), lib.ptr(args[1], torch.int32), lib.ptr(args[2]),
             lib.ptr(args[3], torch.int32), n_lines, lib.ptr(args[4], torch.uint8), lib.ptr(out, torch.float64), lib.stream())
    return out.cpu().numpy()


def test_line_moments_exact_on_integers_bounded_otherwise_and_reproducible():
    rng = np.random.default_rng(3)
    lengths = LENGTHS + [4992, 3000]
    ptr, idx, val = R.random_lines(rng, lengths, 5000)
    mask = (rng.random(5000) < 0.6).astype(np.uint8)
    lines = np.array([9, 8, 5, 5, 0, 1, 2, 3, 4], dtype=np.int32)
    for ls, n, m in ((None, len(lengths), None), (lines, len(lines), mask), (None, len(lengths), mask)):
        got = _moments(ptr, idx, val, ls, n, m)
        for i, (s1, s2, cnt, _) in enumerate(R.moments_fsum(ptr, idx, val, ls, n, m)):
            assert got[i, 0] == s1 and got[i, 1] == s2, (i, cnt)                            # integers: exact
    x = np.log1p(val / np.float32(3.7)).astype(np.float32)
    worst = 0.0
    for ls, n, m in ((None, len(lengths), None), (lines, len(lines), mask)):
        got = _moments(ptr, idx, x, ls, n, m)
        assert np.array_equal(got, _moments(ptr, idx, x, ls, n, m))                         # two calls: equal bits
        for i, (s1, s2, cnt, sabs) in enumerate(R.moments_fsum(ptr, idx, x, ls, n, m)):
            e1, e2 = abs(got[i, 0] - s1), abs(got[i, 1] - s2)
            assert e1 <= R.moments_bound(cnt, sabs) and e2 <= R.moments_bound(cnt, s2), (i, cnt, e1, e2)
            if cnt:
                worst = max(worst, e1 / R.moments_bound(cnt, sabs), e2 / R.moments_bound(cnt, s2))
    print("line moments: largest error / bound %.3g" % worst)


def test_log1p_within_four_times_numpys_own_error():
    lib = _L()
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 3000, 100000).astype(np.float32)
    totals = rng.integers(200, 60000, 100000).astype(np.float32)
    x = (counts / (totals / np.float32(1e4))).astype(np.float32)                             # what normalize_total leaves
    x = np.concatenate([x, np.float32(2.0) ** rng.uniform(-30, 20, 20000).astype(np.float32), [np.float32(0)]]).astype(np.float32)
    bar, own = R.log1p_bar(x)
    d = _offset(x, torch.float32)
    lib.call('gnx_log1p_f32', lib.ptr(d), len(x), lib.stream())
    got = d.cpu().numpy()
    mine = float(R.ulps_of(got, np.log1p(x.astype(np.float64))).max())
    print("log1p: device %.3f ulp, numpy float32 %.3f ulp, bar %.3f ulp on %d values" % (mine, own, bar, len(x)))
    assert got[-1] == 0 and mine <= bar


def test_refusals():
    lib = _L()
    ptr, idx, val = R.random_lines(np.random.default_rng(5), [3, 4], 10)
    p, i, v = _dev(ptr), _dev(idx), _dev(val)
    out = torch.full((32,), float('nan'), device=DEV)
    P, I, V, O, S = p.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), lib.stream()
    bad, ok = lib.CONSTANTS['GNX_ERR_BAD_ARG'], 0
    q = lib.query
    assert q('gnx_sparse_expand_f32', P, I, V, None, 2, None, O, 10, 0, S) == bad           # L <= 0
    assert q('gnx_sparse_expand_f32', P, I, V, None, 2, None, O, 10, -1, S) == bad
    assert q('gnx_sparse_expand_f32', P, I, V, None, 2, None, O, 9, 10, S) == bad           # ld_out < L
    assert q('gnx_sparse_expand_f32', P, I, V, None, -1, None, O, 10, 10, S) == bad         # n_lines < 0
    assert q('gnx_sparse_expand_f32', None, I, V, None, 2, None, O, 10, 10, S) == bad       # NULL required pointers
    assert q('gnx_sparse_expand_f32', P, None, V, None, 2, None, O, 10, 10, S) == bad
    assert q('gnx_sparse_expand_f32', P, I, None, None, 2, None, O, 10, 10, S) == bad
    assert q('gnx_sparse_expand_f32', P, I, V, None, 2, None, None, 10, 10, S) == bad
    assert q('gnx_sparse_expand_f32', P, I, V, None, 0, None, O, 10, 10, S) == ok           # n_lines == 0
    assert q('gnx_sparse_expand_f32', P, I, V, None, 2, None, O, 65536 * 8192, 65536 * 8192, S) == lib.ERR_UNSUPPORTED
    m = torch.full((4,), float('nan'), dtype=torch.float64, device=DEV)
    M = m.data_ptr()
    assert q('gnx_sparse_line_moments_f64', P, I, V, None, -1, None, M, S) == bad
    assert q('gnx_sparse_line_moments_f64', None, I, V, None, 2, None, M, S) == bad
    assert q('gnx_sparse_line_moments_f64', P, None, V, None, 2, None, M, S) == bad
    assert q('gnx_sparse_line_moments_f64', P, I, None, None, 2, None, M, S) == bad
    assert q('gnx_sparse_line_moments_f64', P, I, V, None, 2, None, None, S) == bad
    assert q('gnx_sparse_line_moments_f64', P, I, V, None, 0, None, M, S) == ok
    assert q('gnx_sparse_div_by_line_f32', P, V, -1, V, S) == bad
    assert q('gnx_sparse_div_by_line_f32', None, V, 2, V, S) == bad
    assert q('gnx_sparse_div_by_line_f32', P, None, 2, V, S) == bad
    assert q('gnx_sparse_div_by_line_f32', P, V, 2, None, S) == bad
    assert q('gnx_sparse_div_by_line_f32', P, V, 0, V, S) == ok
    assert q('gnx_sparse_div_by_idx_f32', I, V, -1, V, S) == bad
    assert q('gnx_sparse_div_by_idx_f32', None, V, 2, V, S) == bad
    assert q('gnx_sparse_div_by_idx_f32', I, None, 2, V, S) == bad
    assert q('gnx_sparse_div_by_idx_f32', I, V, 2, None, S) == bad
    assert q('gnx_sparse_div_by_idx_f32', I, V, 0, V, S) == ok
    assert q('gnx_log1p_f32', V, -1, S) == bad and q('gnx_log1p_f32', None, 2, S) == bad and q('gnx_log1p_f32', V, 0, S) == ok
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(m).all()                                   # nothing was launched
    assert torch.equal(v.cpu(), torch.from_numpy(val))
