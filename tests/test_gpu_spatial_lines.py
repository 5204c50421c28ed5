"""gnx_sparse_line_spatial_f64 (csrc/sparse_spatial.hip) through the C ABI: P, D, Q of every (table, line) against math.fsum -
exact on integers, within n 2^-53 sum |term| on fractions (tests/sparse_counts_ref.py's moments_bound) - over the line lengths
around the wavefront and the workgroup, every K form, tables with absent, out-of-range and self entries, entries outside the
vector, several lines per workgroup, the LDS sizes around the 64 KB opt-in and at the cap, offset storage, determinism,
refusals."""
import math

import numpy as np
import pytest
import torch

import sparse_counts_ref as CR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 0, 600]
N_IDX = 700
LIST = np.array([9, 5, -1, 5, 0, 2, 1, 3, 4, 6, 8, 7], dtype=np.int32)                 # permuted, with a negative entry
BLOCKS = 2048                                    # the launch's workgroups in x (include/gridnext_hip.h): row i -> i mod 2048
NAN = float('nan')


def _L():
    from gridnext_amd import _lib
    return _lib


def _offset(array, dtype):
    """The array on the device, one element into its storage."""
    flat = np.ascontiguousarray(array).reshape(-1)
    t = torch.empty(len(flat) + 1, dtype=dtype, device=DEV)
    t[1:] = torch.from_numpy(flat).to(DEV)
    return t[1:]


def _run(ptr, idx, val, lines, n, n_idx, tables):
    """(n_tables, n, 3) float64 numpy; every buffer sits one element into its storage, the output inside NaN-filled storage
    whose surroundings stay."""
    lib = _L()
    nt, _, K = tables.shape
    keep = (_offset(ptr, torch.int64), _offset(idx, torch.int32), _offset(val, torch.float32),
            None if lines is None else _offset(lines, torch.int32), _offset(tables, torch.int32))
    out = torch.full((nt * n * 3 + 2,), NAN, dtype=torch.float64, device=DEV)
    lib.call('gnx_sparse_line_spatial_f64', lib.ptr(keep[0], torch.int64), lib.ptr(keep[1], torch.int32), lib.ptr(keep[2]),
             lib.ptr(keep[3], torch.int32), n, n_idx, lib.ptr(keep[4], torch.int32), K, nt, out[1:].data_ptr(), lib.stream())
    host = out.cpu()
    assert torch.isnan(host[0]) and torch.isnan(host[-1])
    assert not torch.isnan(host[1:-1]).any()                                          # every element was written
    return host[1:-1].view(nt, n, 3).numpy()


def _want_line(ptr, idx, val, line, n_idx, table):
    """((P, D, Q) by fsum, their bars n 2^-53 sum |term|) of one line over one table; a negative line is empty."""
    if line < 0:
        return (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    b, e = int(ptr[line]), int(ptr[line + 1])
    j, v = idx[b:e].astype(np.int64), val[b:e].astype(np.float64)
    kept = (j >= 0) & (j < n_idx)
    j, v = j[kept], v[kept]
    x = np.zeros(n_idx)
    x[j] = v
    T = table[j].astype(np.int64)
    present = (T >= 0) & (T < n_idx)
    deg = present.sum(1).astype(np.float64)
    terms = ((v[:, None] * x[np.where(present, T, 0)] * present).ravel(), deg * v, deg * v * v)
    sums, bars = [], []
    for t in terms:
        t = t[t != 0]
        sums.append(math.fsum(t))
        bars.append(CR.moments_bound(len(t), math.fsum(np.abs(t))))
    return tuple(sums), tuple(bars)


def _want(ptr, idx, val, lines, n, n_idx, tables):
    """(sums (n_tables, n, 3), bars) - each distinct line once."""
    sums, bars, seen = np.empty((len(tables), n, 3)), np.empty((len(tables), n, 3)), {}
    for t in range(len(tables)):
        for i in range(n):
            line = i if lines is None else int(lines[i])
            if (t, line) not in seen:
                seen[(t, line)] = _want_line(ptr, idx, val, line, n_idx, tables[t])
            sums[t, i], bars[t, i] = seen[(t, line)]
    return sums, bars


def _tables(rng, n_tables, n_idx, K):
    """Random neighbours with about a quarter absent, a few out-of-range values of either sign, and self entries."""
    T = rng.integers(0, n_idx, size=(n_tables, n_idx, K)).astype(np.int64)
    T[rng.random(T.shape) < 0.25] = -1
    odd = rng.random(T.shape) < 0.03
    T[odd] = rng.choice([n_idx, n_idx + 7, -5, 2 ** 31 - 1, -2 ** 31], size=int(odd.sum()))
    own = rng.random((n_tables, n_idx)) < 0.1
    T[..., 0][own] = np.broadcast_to(np.arange(n_idx), (n_tables, n_idx))[own]
    return T.astype(np.int32)


def _matrix(rng, integer, lengths=LENGTHS, n_idx=N_IDX, stray=True):
    ptr, idx, val = CR.random_lines(rng, lengths, n_idx, integer=integer)
    if stray:                                                                         # entries outside the vector: skipped
        idx[ptr[10] - 1] = n_idx + 3                                                  # the last entry of the 600-entry line
        idx[ptr[7]] = -2                                                              # the first of the 257-entry line
    return ptr, idx, val


@pytest.mark.parametrize("K", [1, 6, 18, 32])
def test_every_k_on_integers_and_fractions(K):
    rng = np.random.default_rng(100 + K)
    worst = 0.0
    for integer in (True, False):
        ptr, idx, val = _matrix(rng, integer)
        tables = _tables(rng, 3, N_IDX, K)
        for lines, n in ((None, len(LENGTHS)), (LIST, len(LIST))):
            got3, got1 = _run(ptr, idx, val, lines, n, N_IDX, tables), _run(ptr, idx, val, lines, n, N_IDX, tables[:1])
            assert np.array_equal(got3[0].view(np.int64), got1[0].view(np.int64))      # table 0 does not see the split
            assert np.array_equal(got3.view(np.int64), _run(ptr, idx, val, lines, n, N_IDX, tables).view(np.int64))
            want, bars = _want(ptr, idx, val, lines, n, N_IDX, tables)
            if integer:
                assert np.array_equal(got3, want), (K, n)
            err = np.abs(got3 - want)
            assert (err <= bars).all(), (K, integer, n)
            worst = max(worst, float((err[bars > 0] / bars[bars > 0]).max()))
        assert want[..., 0].max() > 0
    print("K = %d: largest |err| / (n 2^-53 sum |term|) = %.3f" % (K, worst))


def test_several_lines_per_workgroup():
    """More rows than the launch has workgroups: workgroup b walks rows b, b + 2048, b + 4096 - the 600-entry line, then an
    empty line (of no entries, or a negative one), then the one-entry line: the vector must be clean again every time."""
    rng = np.random.default_rng(31)
    ptr, idx, val = _matrix(rng, False)
    tables = _tables(rng, 3, N_IDX, 6)
    lines = np.concatenate([np.full(BLOCKS, 9), np.where(np.arange(BLOCKS) % 2 == 0, 0, -1), np.full(BLOCKS, 1),
                            [5, 9, 1, 7, 3]]).astype(np.int32)
    n = len(lines)
    got = _run(ptr, idx, val, lines, n, N_IDX, tables)
    want, bars = _want(ptr, idx, val, lines, n, N_IDX, tables)
    assert (np.abs(got - want) <= bars).all()
    assert (got[:, BLOCKS:2 * BLOCKS] == 0).all() and (got[:, :BLOCKS, 0] > 0).all()
    for a, b in ((0, BLOCKS), (BLOCKS, 2 * BLOCKS), (2 * BLOCKS, 3 * BLOCKS)):         # one line, one result, whichever workgroup
        assert (got[:, a:b].view(np.int64) == got[:, a:a + 1].view(np.int64)).all()
    few = _run(ptr, idx, val, lines[[0, BLOCKS, 2 * BLOCKS]], 3, N_IDX, tables)      # the same lines on a launch of their own
    assert np.array_equal(few.view(np.int64), got[:, [0, BLOCKS, 2 * BLOCKS]].view(np.int64))


@pytest.mark.parametrize("n_idx", [1, 16384, 16385, 32768])
def test_vector_sizes_around_the_lds_opt_in_and_at_the_cap(n_idx):
    assert _L().query('gnx_sparse_spatial_max_idx') == 32768
    rng = np.random.default_rng(n_idx)
    lengths = [0, 1, 1] if n_idx == 1 else [0, 1, 300, 700, 257]
    ptr, idx, val = _matrix(rng, False, lengths, n_idx, stray=False)
    idx[ptr[-1] - 1] = n_idx - 1                                                      # the vector's last element is used
    tables = _tables(rng, 2, n_idx, 6)
    tables[:, 0, 1] = n_idx - 1
    got = _run(ptr, idx, val, None, len(lengths), n_idx, tables)
    want, bars = _want(ptr, idx, val, None, len(lengths), n_idx, tables)
    assert (np.abs(got - want) <= bars).all() and want[..., 2].max() > 0
    assert np.array_equal(got.view(np.int64), _run(ptr, idx, val, None, len(lengths), n_idx, tables).view(np.int64))


def test_refusals_leave_the_output_untouched():
    lib = _L()
    rng = np.random.default_rng(5)
    ptr, idx, val = CR.random_lines(rng, [3, 4], 10)
    tab = _tables(rng, 2, 10, 6)
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ptr, idx, val, tab.reshape(-1))]
    out = torch.full((2 * 2 * 3 + 1,), NAN, dtype=torch.float64, device=DEV)
    P, I, V, T, O, S = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), out.data_ptr(), lib.stream()
    bad, q, name = lib.CONSTANTS['GNX_ERR_BAD_ARG'], lib.query, 'gnx_sparse_line_spatial_f64'
    assert q(name, None, I, V, None, 2, 10, T, 6, 2, O, S) == bad
    assert q(name, P, None, V, None, 2, 10, T, 6, 2, O, S) == bad
    assert q(name, P, I, None, None, 2, 10, T, 6, 2, O, S) == bad
    assert q(name, P, I, V, None, 2, 10, None, 6, 2, O, S) == bad                     # a NULL table
    assert q(name, P, I, V, None, 2, 10, T, 6, 2, None, S) == bad
    assert q(name, P, I, V, None, -1, 10, T, 6, 2, O, S) == bad
    for K in (0, -1, 33):
        assert q(name, P, I, V, None, 2, 10, T, K, 2, O, S) == bad
    assert q(name, P, I, V, None, 2, 10, T, 6, 0, O, S) == bad
    assert q(name, P, I, V, None, 2, 0, T, 6, 2, O, S) == bad
    assert q(name, P, I, V, None, 2, 10, T, 6, 2, O + 4, S) == bad                    # out not 8-byte aligned
    assert q(name, P, I, V, None, 2, 10, T + 2, 6, 2, O, S) == bad                    # the table not 4-byte aligned
    assert q(name, P, I, V, None, 0, 10, None, 6, 2, O, S) == bad                     # bad arguments come before n == 0
    assert q(name, P, I, V, None, 2, 32769, T, 6, 2, O, S) == lib.ERR_UNSUPPORTED     # the cap + 1
    assert q(name, P, I, V, None, 2, 10, T, 6, 65536, O, S) == lib.ERR_UNSUPPORTED
    assert q(name, P, I, V, None, 2 ** 31, 10, T, 6, 2, O, S) == lib.ERR_UNSUPPORTED
    assert q(name, P, I, V, None, 0, 10, T, 6, 2, O, S) == 0
    assert q(name, P, None, None, None, 0, 10, T, 6, 2, O, S) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                     # nothing was launched
    assert q(name, P, I, V, None, 2, 10, T, 6, 2, O, S) == 0
    torch.cuda.synchronize()
    want, _ = _want(ptr, idx, val, None, 2, 10, tab)
    assert np.array_equal(out[:12].cpu().numpy().reshape(2, 2, 3), want) and torch.isnan(out[12:]).all()
