"""gridnext_amd/spatial.py on the host (no GPU): the neighbour table against the reference's pdist rule, the decomposition of
Moran's I and Geary's C against their dense definitions within the bars of tests/spatial_ref.py, the permuted table against
permuting dense values, the zero-variance rule, variances, p-values, `top`, the frame, every refusal, the C ABI's parameters."""
import math

import numpy as np
import pytest

import sparse_counts_ref as CR
import spatial_ref as R

_made = {}


def _host():
    """The fixture as host SpotCounts, normalised + log1p."""
    if 'h' not in _made:
        import gridnext_amd as ga
        f = R.fixture()
        _made['h'] = ga.SpotCounts(f['X'], f['obs'], f['genes']).normalize_total(CR.TARGET).log1p()
    return _made['h']


def _tiny(values, x=None, y=None):
    """SpotCounts of one array on a row of the pseudo-hex grid (or the given coordinates) from a dense integer matrix."""
    import pandas as pd
    import gridnext_amd as ga
    values = np.asarray(values, dtype=np.float64)
    n = len(values)
    x = 2 * np.arange(n) if x is None else x
    y = np.zeros(n, dtype=np.int64) if y is None else y
    obs = pd.DataFrame({'x': x, 'y': y, 'array': 'a', 'annotation': 'c0'}, index=['s%d' % k for k in range(n)])
    return ga.SpotCounts(values, obs, ['g%d' % g for g in range(values.shape[1])])


# ------------------------------------------------------------------------------------------------ the graph
def test_table_against_the_pdist_rule_on_the_full_array_and_the_fixture():
    from gridnext_amd import spatial as S
    x, y = R.full_visium_grid()
    T = S.neighbor_table(x, y, 1)
    assert T.dtype == np.int32 and T.shape == (78 * 64, 6) and np.array_equal(T, R.table(x, y, 1))
    ours = S.edge_index([T], [0])
    slack, bare = R.pdist_edges(x, y, 0, 1 + 1e-9), R.pdist_edges(x, y, 0, 1)
    print("full 78 x 64 array: %d directed pairs; the bare `<= 1` rule finds %d and misses %d"
          % (ours.shape[1], bare.shape[1], ours.shape[1] - bare.shape[1]))
    assert ours.dtype == np.int64 and np.array_equal(ours, slack)
    assert ours.shape[1] == 29386 and bare.shape[1] == 19734
    missed = set(map(tuple, ours.T)) - set(map(tuple, bare.T))
    assert all(abs(int(y[a]) - int(y[b])) == 1 for a, b in missed)                    # all diagonal
    f = R.fixture()
    for a in range(2):
        r = slice(int(f['row_start'][a]), int(f['row_start'][a + 1]))
        fx, fy = f['obs']['x'].values[r], f['obs']['y'].values[r]
        assert 500 <= len(fx) <= 600
        assert np.array_equal(S.edge_index([S.neighbor_table(fx, fy)], [0]), R.pdist_edges(fx, fy, 0, 1 + 1e-9))


@pytest.mark.parametrize("n_rings,K", [(1, 6), (2, 18)])
def test_table_symmetry_degrees_and_ring_distances(n_rings, K):
    from gridnext_amd import spatial as S
    assert S.hex_offsets(n_rings) == R.offsets(n_rings) and len(S.hex_offsets(n_rings)) == K
    f = R.fixture()
    r = slice(0, int(f['row_start'][1]))
    x, y = f['obs']['x'].values[r], f['obs']['y'].values[r]
    T = S.neighbor_table(x, y, n_rings)
    assert np.array_equal(T, R.table(x, y, n_rings)) and T.shape[1] == K
    pairs = set(map(tuple, S.edge_index([T], [0]).T))
    assert all((b, a) in pairs for a, b in pairs) and all(a != b for a, b in pairs)
    assert ((T >= 0).sum(1) <= K).all() and (T >= 0).sum(1).max() == K
    t = R.true_coords(x, y)
    for k in range(K):
        at = np.flatnonzero(T[:, k] >= 0)
        d = np.linalg.norm(t[at] - t[T[at, k]], axis=1)
        want = 1.0 if k < 6 else (2.0 if k in (6, 7) else (math.sqrt(3) if k in (8, 9, 10, 11, 16, 17) else 2.0))
        assert np.allclose(d, want, rtol=1e-12), k
    for a in range(len(x)):                                                           # one column per offset, none repeated
        present = T[a][T[a] >= 0]
        assert len(set(present)) == len(present)


def test_refused_coordinates():
    from gridnext_amd import spatial as S
    with pytest.raises(ValueError, match=r"spot 1 .*spot 3.*one coordinate \(2, 0\)"):
        S.neighbor_table([0, 2, 4, 2], [0, 0, 0, 0])
    with pytest.raises(ValueError, match=r"spot b at \(3, 0\) has x \+ y odd"):
        S.neighbor_table([0, 3], [0, 0], names=['a', 'b'])
    with pytest.raises(ValueError, match="integers"):
        S.neighbor_table([0.5, 2], [0, 0])
    for bad in (0, 3, True, None):
        with pytest.raises(ValueError, match="n_rings"):
            S.hex_offsets(bad)
    with pytest.raises(ValueError, match="array a: spot s2 at"):
        _tiny(np.ones((3, 2)), x=np.array([0, 2, 5]), y=np.zeros(3, np.int64)).spot_neighbors()


def test_edge_index_of_a_view_and_no_edge_between_arrays():
    from gridnext_amd import spatial as S
    host, f = _host(), R.fixture()
    rs = f['row_start']
    tabs = host.spot_neighbors()
    assert len(tabs) == 2 and all(t.dtype.is_floating_point is False and t.shape[1] == 6 for t in tabs)
    assert host.spot_neighbors() is tabs and host.spot_neighbors(2)[0].shape[1] == 18       # cached per n_rings
    E = host.edge_index().numpy()
    assert E.dtype == np.int64 and E.shape[0] == 2
    same = (np.searchsorted(rs, E[0], side='right') == np.searchsorted(rs, E[1], side='right'))
    assert same.all()                                                                 # block diagonal
    want = []
    for a in range(2):
        T = tabs[a].numpy()
        want += [(rs[a] + r, rs[a] + T[r, k]) for r in range(len(T)) for k in range(6) if T[r, k] >= 0]
    assert sorted(map(tuple, E.T)) == sorted(want) and len(want) == E.shape[1]
    second = host.subset_arrays(['arr1']).edge_index().numpy()                        # storage rows, not view rows
    assert second.min() >= rs[1] and np.array_equal(second, E[:, E[0] >= rs[1]])
    assert np.array_equal(S.edge_index([tabs[1].numpy()], [rs[1]]), second)


# ------------------------------------------------------------------------------------------------ the statistics
def test_decomposition_against_the_dense_definitions():
    from gridnext_amd import spatial as S
    host, ref = _host(), R.reference()
    assert np.array_equal(np.asarray(host.host_csr().todense()), R.fixture()['dense'])   # the stored values are the restatement's
    margin, gap, away = R.check_fixture()                                             # and the fixture holds its margins
    print("fixture: min planted I - max scattered I %.3f; smallest gap of sorted I %.2e; smallest |I_t - I| %.2e" % (margin, gap, away))
    got = host.spatial_autocorr()
    R.check_result(got, ref, "host")
    # the sums themselves, per array, within their own bars
    lines, worst = host.gene_lines(), 0.0
    for (_, _, trio, _), table, want in zip(host.bound_csc(), host._host_neighbors(1), ref['per']):
        pdq = S.line_spatial(trio, lines, host.n_genes, len(table), table[None], None)[0]
        for c, name in enumerate(('P', 'D', 'Q')):
            err = np.abs(pdq[:, c] - want[name])
            assert (err <= want[name + '_bar']).all(), name
            worst = max(worst, float((err / want[name + '_bar']).max()))
    print("host sums P, D, Q: largest |err| / bar %.3g" % worst)
    # the decomposition from the fsum sums is the dense definition: the identity itself
    I, C = R.statistics(ref['sums'], ref['N'], ref['W'])                              # noqa: E741
    assert (np.abs(I - ref['I']) <= ref['I_bar']).all() and (np.abs(C - ref['C']) <= ref['C_bar']).all()
    # and the dense W matrix itself on one array
    xs, tabs = R.array_parts(arrays=(1,), genes=list(range(0, 96, 8)))
    I1, C1 = R.dense_matrix_statistics(xs[0], R.dense_w(tabs[0]))
    one = host.subset_arrays(['arr1']).subset_genes(np.arange(96) % 8 == 0).spatial_autocorr()
    r1 = R.reference(arrays=(1,), genes=list(range(0, 96, 8)))
    assert (np.abs(one.I - I1) <= r1['I_bar']).all() and (np.abs(one.C - C1) <= r1['C_bar']).all()
    assert np.array_equal(got.top(16), R.fixture()['planted']) and np.array_equal(got.top(16), R.top_mask(ref['I'], 16, True))
    assert np.array_equal(got.top(16, by='C'), R.top_mask(ref['C'], 16, False))


def test_integer_counts_are_exact():
    import gridnext_amd as ga
    f = R.fixture()
    raw = ga.SpotCounts(f['X'], f['obs'], f['genes'])
    D = np.asarray(f['X'].todense(), dtype=np.float64)
    rs, lines = f['row_start'], raw.gene_lines()
    from gridnext_amd import spatial as S
    for a, ((_, _, trio, _), table) in enumerate(zip(raw.bound_csc(), raw._host_neighbors(1))):
        pdq = S.line_spatial(trio, lines, raw.n_genes, len(table), table[None], None)[0]
        want = R.sums_fsum(D[rs[a]:rs[a + 1]], R.table(f['obs']['x'].values[rs[a]:rs[a + 1]], f['obs']['y'].values[rs[a]:rs[a + 1]]))
        for c, name in enumerate(('P', 'D', 'Q')):
            assert np.array_equal(pdq[:, c], want[name]), name
    raw.spatial_autocorr()                                                            # raw counts are served too


def test_permuted_table_against_permuting_dense_values():
    from gridnext_amd import spatial as S
    xs, tabs = R.array_parts(arrays=(0,), genes=[0, 5, 40])
    x, T = xs[0], tabs[0]
    rng = np.random.default_rng(11)
    for _ in range(3):
        perm = rng.permutation(len(x))
        Tp = S.permuted_table(T, perm)
        assert Tp.dtype == np.int32 and np.array_equal(Tp < 0, T[np.argsort(perm)] < 0)
        moved, direct = R.sums_fsum(x[perm], T), R.sums_fsum(x, Tp)
        for name in ('S1', 'S2', 'P', 'D', 'Q'):
            assert np.array_equal(moved[name], direct[name]), name
    with pytest.raises(ValueError, match="permutation"):
        S.permuted_table(T, np.zeros(len(T), dtype=np.int64))


def test_permutations_on_the_host():
    host, ref = _host(), R.reference()
    got = host.spatial_autocorr(n_perms=R.N_PERMS, seed=R.SEED)
    R.check_result(got, ref, "host, 49 permutations", R.simulations())
    frame = got.to_frame()
    from gridnext_amd import spatial as S
    assert list(frame.columns) == S.COLUMNS + S.SIM_COLUMNS and list(frame.index) == list(host.gene_ids)
    assert np.array_equal(frame['pval_sim_I'].values, got.pval_sim_I) and got.sim_I.shape == (R.N_PERMS, 96)
    plain = host.spatial_autocorr()
    assert list(plain.to_frame().columns) == S.COLUMNS and not hasattr(plain, 'sim_I')
    assert np.array_equal(plain.I, got.I) and np.array_equal(plain.C, got.C)
    assert (got.pval_sim_I[R.fixture()['planted']] == 1.0 / 50).all()


def test_flat_genes_are_nan_and_disturb_nothing():
    rng = np.random.default_rng(5)
    D = rng.integers(0, 6, size=(40, 5)).astype(np.float64)
    x, y = 2 * (np.arange(40) % 8) + (np.arange(40) // 8) % 2, np.arange(40) // 8
    full = _tiny(D, x, y).spatial_autocorr(n_perms=5)
    D2 = D.copy()
    D2[:, 1] = 0                                                                      # never seen
    D2[:, 3] = 7                                                                      # constant
    got = _tiny(D2, x, y).spatial_autocorr(n_perms=5)
    for name in got.columns:
        v = getattr(got, name)
        if not name.startswith(('expected', 'var_norm')):
            assert np.isnan(v[[1, 3]]).all(), name
        if 'fdr' not in name:
            assert np.array_equal(v[[0, 2, 4]], getattr(full, name)[[0, 2, 4]]), name
    assert np.isnan(got.sim_I[:, [1, 3]]).all() and np.isfinite(got.pval_norm_fdr_bh_I[[0, 2, 4]]).all()
    assert np.allclose(got.pval_norm_fdr_bh_I, R.bh(got.pval_norm_I), rtol=1e-13, atol=0, equal_nan=True)
    mask = got.top(4)
    assert list(np.flatnonzero(mask)) == [0, 1, 2, 4]                                  # NaN last, ties among NaN to the lower index


def test_top_with_ties_and_nan():
    from gridnext_amd.spatial import SpatialAutocorr
    I = np.array([0.3, np.nan, 0.5, 0.3, 0.1, 0.5])                                    # noqa: E741
    C = np.array([0.7, np.nan, 0.2, 0.7, 0.9, 0.2])
    r = SpatialAutocorr(np.arange(6), 10, 20, {'I': I, 'C': C})
    assert list(np.flatnonzero(r.top(3))) == [0, 2, 5] and list(np.flatnonzero(r.top(3, by='C'))) == [0, 2, 5]
    assert list(np.flatnonzero(r.top(1))) == [2] and list(np.flatnonzero(r.top(5))) == [0, 2, 3, 4, 5] and r.top(6).all()
    for bad in (0, 7, 1.5, True):
        with pytest.raises(ValueError, match="n must be"):
            r.top(bad)
    with pytest.raises(ValueError, match="by must be"):
        r.top(2, by='G')


def test_variances_and_benjamini_hochberg():
    from gridnext_amd import spatial as S
    ref = R.reference()
    e_i, var_i, var_c = S.normality_variances(ref['N'], ref['W'], sum(int(((T >= 0).sum(1) ** 2).sum()) for T in R.array_parts()[1]))
    assert math.isclose(e_i, ref['e_i'], rel_tol=1e-14) and math.isclose(var_i, ref['var_i'], rel_tol=1e-13)
    assert math.isclose(var_c, ref['var_c'], rel_tol=1e-13)
    # a path of 3 spots, by hand: N = 3, W = 4, degrees 1 2 1: S1w = 8, S2w = 24
    e, vi, vc = S.normality_variances(3, 4, 6)
    assert e == -0.5 and math.isclose(vi, (9 * 8 - 3 * 24 + 48) / (8 * 16) - 0.25) and math.isclose(vc, ((16 + 24) * 2 - 64) / (2 * 4 * 16))
    p = np.array([0.01, np.nan, 0.04, 0.03, 0.04, 0.9, np.inf, 0.002])
    assert np.allclose(S.benjamini_hochberg(p), R.bh(p), rtol=1e-15, atol=0, equal_nan=True)
    assert np.isnan(S.benjamini_hochberg(p)[[1, 6]]).all()


def test_refusals():
    host = _host()
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_perms"):
            host.spatial_autocorr(n_perms=bad)
    with pytest.raises(ValueError, match="n_rings"):
        host.spatial_autocorr(n_rings=3)
    with pytest.raises(ValueError, match="n_rings"):
        host.spot_neighbors(0)
    with pytest.raises(ValueError, match="at least 3"):
        _tiny(np.ones((2, 2))).spatial_autocorr()
    with pytest.raises(ValueError, match="W == 0"):
        _tiny(np.ones((3, 2)), x=np.array([0, 6, 12])).spatial_autocorr()


def test_the_abi_of_the_new_entry_point():
    from gridnext_amd import _lib
    assert _lib.PARAMS['gnx_sparse_line_spatial_f64'] == ['lineptr', 'idx', 'val', 'lines', 'n_lines', 'n_idx', 'nbr', 'K',
                                                           'n_tables', 'out', 'stream']
    assert _lib.PARAMS['gnx_sparse_spatial_max_idx'] == []
    import ctypes
    res, args = _lib.SIGNATURES['gnx_sparse_line_spatial_f64']
    assert res is ctypes.c_int and args[4:6] == [ctypes.c_long, ctypes.c_long] and args[7:9] == [ctypes.c_long, ctypes.c_long]
    assert _lib.SIGNATURES['gnx_sparse_spatial_max_idx'][0] is ctypes.c_long
