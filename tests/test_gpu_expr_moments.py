"""csrc/expr_moments.hip through the C ABI against tests/expr_metrics_ref.py (math.fsum over float64 terms).

Bound, every sum: |got - fsum| <= (n + 16) 2^-53 sum |term|, n the terms added so far plus the calls: any order of n
additions in double lies within n 2^-53 sum |term|, and 16 covers the roundings inside one term with more than twofold margin
(exp within 1 ulp in double on both branches of the sigmoid, the add, the divide, the product).  Where a term is itself
subnormal (z = -745) the relative statement has no meaning and the test asks for the range [0, 1e-322] instead.

Also: the padding of M and the other kernel's columns stay NaN, a second call gives equal bits, accumulate adds, a NaN in z
reaches only its own gene, and every refusal leaves a NaN output untouched."""
import numpy as np
import pytest
import torch

import expr_metrics_ref as E
import sparse_counts_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
BS = [1, 3, 4, 5, 63, 64, 65, 257] + [127, 128, 129, 384, 385, 513, 700]    # + around the 128 strips and their 4-row unrolling
GS = [1, 63, 64, 65, 130] + [7, 8, 9]                                       # + around the 8-column tile
LENGTHS = [0, 1, 63, 64, 65, 257, 0, 300]


def _L():
    from gridnext_amd import _lib
    return _lib


def _dev(array, offset=False):
    """The array on the device: at the start of its storage, or one element into it."""
    if array is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(array))
    t = torch.empty(src.numel() + 1, dtype=src.dtype, device=DEV)
    t[int(offset):int(offset) + src.numel()] = src.reshape(-1).to(DEV)
    return t[int(offset):int(offset) + src.numel()]


def _padded(z, ld):
    out = np.full((z.shape[0], ld), np.nan, dtype=np.float32)
    out[:, :z.shape[1]] = z
    return out


class Table:
    """double M[G][ld_m] one element into a NaN-filled buffer with eight guard elements behind."""

    def __init__(self, G, ld_m):
        self.G, self.ld = G, ld_m
        self.store = torch.full((1 + G * ld_m + 8,), NAN, dtype=torch.float64, device=DEV)
        self.view = self.store[1:1 + G * ld_m]

    def ptr(self):
        return self.view.data_ptr()

    def read(self, written):
        """(G, ld_m) on the host after checking that exactly the columns `written` are not NaN, guards included."""
        torch.cuda.synchronize()
        assert torch.isnan(self.store[:1]).all() and torch.isnan(self.store[1 + self.G * self.ld:]).all()
        got = self.view.cpu().numpy().reshape(self.G, self.ld).copy()
        for k in range(self.ld):
            assert np.isnan(got[:, k]).all() != (k in written), (k, written)
        return got


def _dense(z, ldz, act, table, accumulate=0):
    lib = _L()
    zd = _dev(_padded(z, ldz), True)
    lib.call('gnx_act_col_moments_f64', lib.ptr(zd), ldz, z.shape[0], z.shape[1], act, table.ptr(), table.ld, accumulate, lib.stream())
    torch.cuda.synchronize()


def _sparse(mat, gene_lines, n, pos, scale, z, ldz, act, table, accumulate=0, offset=True):
    lib = _L()
    ptr, idx, val = mat
    a = (_dev(ptr), _dev(idx, offset), _dev(val, offset), _dev(gene_lines), _dev(pos), _dev(scale, offset), _dev(_padded(z, ldz), offset))
    lib.call('gnx_sparse_pred_moments_f64', lib.ptr(a[0], torch.int64), lib.ptr(a[1], torch.int32), lib.ptr(a[2]),
             lib.ptr(a[3], torch.int32), n, lib.ptr(a[4], torch.int32), lib.ptr(a[5]), lib.ptr(a[6]), ldz, act, table.ptr(), table.ld,
             accumulate, lib.stream())
    torch.cuda.synchronize()


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _within(got, S, A, N, calls=1):
    return bool((np.abs(got - S) <= E.bound(N, A, calls)).all())


def _ratio(got, S, A):
    return float((np.abs(got - S)[A > 0] / (E.U * A[A > 0])).max()) if (A > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ the dense half
@pytest.mark.parametrize("B", BS)
def test_dense_sums_lie_within_the_bound_of_fsum(B):
    lib = _L()
    rng = np.random.default_rng(B)
    worst = 0.0
    for G in GS:
        z = (rng.standard_normal((B, G)) * 3).astype(np.float32)
        none = np.zeros((B, G), dtype=bool)
        for act in (lib.CONSTANTS['GNX_ACT_NONE'], lib.CONSTANTS['GNX_ACT_SIGMOID']):
            S, A, N = E.sums(z, np.zeros((B, G), np.float32), none, act)
            first = None
            for ldz in (G, G + 3):
                for ld_m in (5, 7):
                    table = Table(G, ld_m)
                    _dense(z, ldz, act, table)
                    got = table.read({0, 1})[:, :2]
                    assert _within(got, S[:, :2], A[:, :2], N[:, :2]), (G, act, ldz, ld_m)
                    first = got if first is None else first
                    assert _bits(got, first), (G, act, ldz, ld_m)                    # ldz, ld_m: the same bits
                    worst = max(worst, _ratio(got, S[:, :2], A[:, :2]))
            if act:
                alone = Table(1, 5)                                                  # the last column alone, elsewhere in memory
                _dense(z[:, G - 1:], 1, act, alone)
                assert _bits(alone.read({0, 1})[:, :2], first[G - 1:])
    print("dense B=%d: largest |err| / (2^-53 sum|term|) = %.3f, allowed %d" % (B, worst, B + 1 + E.EXTRA))


def test_dense_extreme_inputs_stay_in_the_unit_interval():
    lib = _L()
    big = float(np.finfo(np.float32).max)
    vals = [0.0, 1e-30, -1e-30, 20.0, -20.0, 50.0, -50.0, 745.0, -745.0, 1e4, -1e4, big, -big, np.inf, -np.inf]
    z = np.array([vals], dtype=np.float32)
    table = Table(len(vals), 5)
    _dense(z, len(vals), lib.CONSTANTS['GNX_ACT_SIGMOID'], table)
    got = table.read({0, 1})
    p, pp = got[:, 0], got[:, 1]
    print("sigmoid at the extremes:", dict(zip(vals, p.tolist())))
    assert ((p >= 0) & (p <= 1)).all() and ((pp >= 0) & (pp <= 1)).all()
    assert p[0] == 0.5 and pp[0] == 0.25
    for k, v in enumerate(vals):
        if v >= 50:
            assert p[k] == 1.0 and pp[k] == 1.0, v                                   # 1 + exp(-50) rounds to 1
        elif v <= -1e4:
            assert p[k] == 0.0 and pp[k] == 0.0, v                                   # exp underflows to 0
        elif v == -745.0:
            assert 0.0 <= p[k] <= 1e-322 and pp[k] == 0.0                            # a subnormal: within its own spacing
        else:
            want = float(E.predictions(np.float32(v), 1))
            assert abs(p[k] - want) <= (2 + E.EXTRA) * E.U * want, v
            assert abs(pp[k] - want * want) <= (2 + E.EXTRA) * E.U * want * want, v
    # the identity passes every value through
    table = Table(len(vals), 5)
    _dense(z, len(vals), lib.CONSTANTS['GNX_ACT_NONE'], table)
    assert np.array_equal(table.read({0, 1})[:, 0], z[0].astype(np.float64))


def test_dense_nan_reaches_only_its_own_gene_and_accumulate_adds():
    lib = _L()
    act = lib.CONSTANTS['GNX_ACT_SIGMOID']
    rng = np.random.default_rng(7)
    B, G = 70, 67
    z = (rng.standard_normal((B, G)) * 2).astype(np.float32)
    z[41, 65] = np.nan
    table = Table(G, 6)
    _dense(z, G + 1, act, table)
    got = table.read({0, 1})[:, :2]
    S, A, N = E.sums(z, np.zeros((B, G), np.float32), np.zeros((B, G), bool), act)
    keep = np.arange(G) != 65
    assert np.isnan(got[65]).all() and not np.isnan(got[keep]).any()
    assert _within(got[keep], S[keep, :2], A[keep, :2], N[keep, :2])
    # two calls into one table: the second adds, and a second pair gives the same bits
    z[41, 65] = 0.25
    z2 = (rng.standard_normal((33, G)) * 2).astype(np.float32)
    S, A, N = E.sums(np.concatenate([z, z2]), np.zeros((B + 33, G), np.float32), np.zeros((B + 33, G), bool), act)
    pair = []
    for _ in range(2):
        table = Table(G, 5)
        _dense(z, G, act, table)
        _dense(z2, G, act, table, accumulate=1)
        pair.append(table.read({0, 1})[:, :2])
    assert _bits(pair[0], pair[1]) and _within(pair[0], S[:, :2], A[:, :2], N[:, :2], calls=2)
    # B == 0 writes zeros
    table = Table(3, 5)
    some = torch.zeros(3, device=DEV)
    lib.call('gnx_act_col_moments_f64', lib.ptr(some), 3, 0, 3, act, table.ptr(), 5, 0, lib.stream())
    assert not table.read({0, 1})[:, :2].any()


# ------------------------------------------------------------------------------------------------ the sparse half
def _case(rng, integer, n_rows=320, B=200):
    mat = R.random_lines(rng, LENGTHS, n_rows, integer=integer)
    pos = np.full(n_rows, -1, dtype=np.int32)
    pos[rng.choice(n_rows, size=B, replace=False)] = rng.permutation(B)
    return mat, pos


@pytest.mark.parametrize("integer", [True, False])
def test_sparse_sums_lie_within_the_bound_of_fsum(integer):
    lib = _L()
    rng = np.random.default_rng(11 + integer)
    n_rows, B = 320, 200
    mat, pos = _case(rng, integer, n_rows, B)
    n_lines = len(LENGTHS)
    gene_lines = np.concatenate([rng.permutation(n_lines), [-1, 7, 7]]).astype(np.int32)       # permuted, no line, a repeat
    worst = 0.0
    for gl, n in ((None, n_lines), (gene_lines, len(gene_lines))):
        scale = (rng.random(n) * 0.2 + 0.001).astype(np.float32)
        for ps, rows_z in ((pos, B), (None, n_rows)):
            z = (rng.standard_normal((rows_z, n)) * 3).astype(np.float32)
            for sc in (None, scale):
                t, stored = E.csc_targets(*mat, gl, n, ps, sc, rows_z)
                for act in (lib.CONSTANTS['GNX_ACT_NONE'], lib.CONSTANTS['GNX_ACT_SIGMOID']):
                    S, A, N = E.sums(z, t, stored, act)
                    first = None
                    for ldz, ld_m, offset in ((n, 5, True), (n + 3, 7, False)):
                        table = Table(n, ld_m)
                        _sparse(mat, gl, n, ps, sc, z, ldz, act, table, offset=offset)
                        got = table.read({2, 3, 4})[:, 2:5]
                        assert _within(got, S[:, 2:], A[:, 2:], N[:, 2:]), (n, ps is None, sc is None, act, ldz)
                        first = got if first is None else first
                        assert _bits(got, first)                                     # ldz, ld_m, alignment, a second call
                        worst = max(worst, _ratio(got, S[:, 2:], A[:, 2:]))
                    assert not first[N[:, 2] == 0].any() and (N[:, 2] == 0).sum() >= 2           # zeros are written
                    if gl is not None:
                        assert not first[n_lines].any()                                          # no line: zeros
                        assert sc is not None or _bits(first[-1, :2], first[-2, :2])             # the repeated line's own sums
                    if integer and sc is None:
                        assert np.array_equal(first[:, :2], S[:, 2:4])                         # integer sums are exact
    print("sparse %s values: largest |err| / (2^-53 sum|term|) = %.3f" % ('integer' if integer else 'fractional', worst))


def test_sparse_accumulates_over_two_arrays_beside_the_dense_half():
    lib = _L()
    act = lib.CONSTANTS['GNX_ACT_SIGMOID']
    rng = np.random.default_rng(23)
    n, B = len(LENGTHS), 260
    mat1, pos1 = _case(rng, False, 320, 200)
    mat2 = R.random_lines(rng, [int(k) for k in rng.integers(0, 150, n)], 280, integer=False)
    pos2 = np.full(280, -1, dtype=np.int32)
    pos2[rng.choice(280, size=60, replace=False)] = 200 + rng.permutation(60)
    scale = (rng.random(n) * 0.2 + 0.001).astype(np.float32)
    z = (rng.standard_normal((B, n)) * 3).astype(np.float32)
    t1, k1 = E.csc_targets(*mat1, None, n, pos1, scale, B)
    t2, k2 = E.csc_targets(*mat2, None, n, pos2, scale, B)
    assert not (k1 & k2).any()
    S, A, N = E.sums(z, t1 + t2, k1 | k2, act)
    pair = []
    for _ in range(2):
        table = Table(n, 6)
        _dense(z, n, act, table)
        _sparse(mat1, None, n, pos1, scale, z, n, act, table)
        _sparse(mat2, None, n, pos2, scale, z, n, act, table, accumulate=1)
        pair.append(table.read({0, 1, 2, 3, 4})[:, :5])
    assert _bits(pair[0], pair[1])
    calls = np.array([1, 1, 2, 2, 2])
    assert bool((np.abs(pair[0] - S) <= E.bound(N, A, calls)).all())
    # the statistics a caller derives: mse per gene against the dense float64 evaluation
    p, t = E.predictions(z, act), (t1 + t2).astype(np.float64)
    mse = E.statistics(pair[0], B)[2]
    assert np.allclose(mse, ((p - t) ** 2).mean(0), rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched():
    lib = _L()
    ptr, idx, val = R.random_lines(np.random.default_rng(5), [3, 4], 10)
    p, i, v = _dev(ptr), _dev(idx), _dev(val)
    z = torch.full((10 * 8,), 1.0, device=DEV)
    sc = torch.full((8,), 0.5, device=DEV)
    out = torch.full((64,), NAN, dtype=torch.float64, device=DEV)
    P, I, V, Z, SC, O, S = p.data_ptr(), i.data_ptr(), v.data_ptr(), z.data_ptr(), sc.data_ptr(), out.data_ptr(), lib.stream()
    bad, uns, ok = lib.CONSTANTS['GNX_ERR_BAD_ARG'], lib.ERR_UNSUPPORTED, 0
    q = lib.query
    dense = lambda **k: q('gnx_act_col_moments_f64', *[{**dict(z=Z, ldz=8, B=10, G=2, activation=1, M=O, ld_m=5, accumulate=0,     # noqa: E731
                                                           stream=S), **k}[n] for n in lib.PARAMS['gnx_act_col_moments_f64']])
    sparse = lambda **k: q('gnx_sparse_pred_moments_f64', *[{**dict(lineptr=P, idx=I, val=V, gene_lines=None, n_channels=2,       # noqa: E731
                                                                pos_of_idx=None, gene_scale=SC, z=Z, ldz=8, activation=1, M=O, ld_m=5,
                                                                accumulate=0, stream=S), **k}[n]
                                                        for n in lib.PARAMS['gnx_sparse_pred_moments_f64']])
    assert len(lib.PARAMS['gnx_act_col_moments_f64']) == 9 and len(lib.PARAMS['gnx_sparse_pred_moments_f64']) == 14
    for call, count in ((dense, 'G'), (sparse, 'n_channels')):
        assert call(z=None) == bad and call(M=None) == bad
        assert call(**{count: -1}) == bad and call(**{count: 9}) == bad                  # ldz = 8 < 9
        assert call(ld_m=4) == bad and call(activation=2) == bad and call(activation=-1) == bad
        assert call(M=O + 4) == bad and call(z=Z + 2) == bad                             # 8-byte, 4-byte alignment
        assert call(**{count: 2 ** 31, 'ldz': 2 ** 31}) == uns
        assert call(**{count: 0}) == ok
    assert dense(B=-1) == bad
    assert sparse(lineptr=None) == bad and sparse(idx=None) == bad and sparse(val=None) == bad
    assert sparse(val=V + 2) == bad and sparse(gene_scale=SC + 1) == bad
    assert sparse(n_channels=0, idx=None, val=None) == ok
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                        # nothing was launched
    assert dense() == ok and sparse(gene_scale=None) == ok
    torch.cuda.synchronize()
    got = out[:10].cpu().numpy().reshape(2, 5)
    assert not np.isnan(got).any() and torch.isnan(out[10:]).all()
