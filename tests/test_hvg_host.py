"""`SpotCounts.highly_variable_genes` on the host and gridnext_amd/hvg.py's loess against the numpy restatement
(tests/hvg_ref.py): moments, fitted values under the loess bar, identical ranks and masks for batch=None and batch='array', views,
the loess's properties at its edge cases, every refusal, the frame, and the new entry points."""
import os

import numpy as np
import pytest

import hvg_ref as R

N_TOP = R.N_TOP
_made = {}


def _counts():
    if 'c' not in _made:
        import gridnext_amd as ga
        X, obs, genes, D = R.fixture()
        _made['c'] = (ga.SpotCounts(X, obs, genes), D)
    return _made['c']


def _reference(batch):
    return R.reference(batch)


def test_fixture_conditions():
    """Every batch clips at least 5 entries, and among each batch's top N_TOP + 1 scores adjacent ones differ by 1e-6 relative -
    seven orders over the rounding differences between two float64 evaluations, so equal masks are a fair demand."""
    counts, D = _counts()
    assert D.shape == (401, 300) and not D[:, 7].any() and (D[:, 11] != 0).sum() == 1
    for batch in (None, 'array'):
        for p in _reference(batch)[0]:
            gap = R.min_adjacent_gap(p['norm'], N_TOP + 1)
            print("batch of %d spots: %d entries above their bound, smallest adjacent gap %.1e" % (p['N'], p['above'], gap))
            assert p['above'] >= 5 and gap >= 1e-6


@pytest.mark.parametrize("batch", [None, 'array'])
def test_host_path_against_the_restatement(batch):
    counts, _ = _counts()
    got = counts.highly_variable_genes(n_top_genes=N_TOP, span=0.3, batch=batch)
    R.check_against_reference(got, batch, "host path")
    if batch == 'array':
        assert set(np.unique(got.highly_variable_nbatches)) <= {0, 1, 2} and (got.highly_variable_nbatches == 2).any()


def test_fitted_values_under_the_loess_bar():
    from gridnext_amd import hvg
    for p in _reference(None)[0] + _reference('array')[0]:
        reg_std, clip = hvg.clip_bounds(p['mean'], p['var'], p['N'], 0.3)
        fit = 2 * np.log10(reg_std)
        err = np.abs(fit - p['fit'])
        pos = p['var'] > 0
        print("host loess on %d genes: largest |err| / bar %.3g" % (pos.sum(), float((err[pos] / p['fit_bar'][pos]).max())))
        assert (err <= p['fit_bar'] + 4 * R.U * np.abs(p['fit'])).all() and (fit[~pos] == 0).all() and (~pos).sum() >= 1


def test_gene_subset_and_array_subset():
    counts, D = _counts()
    picks = np.random.default_rng(3).permutation(300)[:120]
    view = counts.subset_genes([counts.gene_ids[g] for g in picks]).subset_arrays(['arr1'])
    got = view.highly_variable_genes(n_top_genes=20)
    r0, r1 = counts.array_span(1)
    per, mean, var, (vn, rank, nb, hv) = R.recipe(D[r0:r1][:, picks], [0, r1 - r0], None, n_top=20)
    assert np.array_equal(got.highly_variable, hv) and np.array_equal(got.highly_variable_rank, rank, equal_nan=True)
    assert (np.abs(got.variances_norm - vn) <= R.norm_bar(per[0])).all() and list(got.gene_ids) == list(view.gene_ids)
    assert view.subset_genes(got.highly_variable).n_genes == 20


# ------------------------------------------------------------------------------------------------ the loess alone
def _check_loess(xs, ys, span):
    from gridnext_amd import hvg
    fit, bar, wins = R.loess(xs, ys, span)
    got_wins = hvg.loess_windows(xs, span)
    for a, b in zip(got_wins, wins):
        assert a.dtype == b.dtype and np.array_equal(a, b), (len(xs), span)
    got = hvg.loess_fit(xs, ys, span)
    assert (np.abs(got - fit) <= bar).all(), (len(xs), span, float((np.abs(got - fit) / bar).max()))
    return got, got_wins


@pytest.mark.parametrize("n", [3, 4, 10])
def test_small_n_every_q(n):
    rng = np.random.default_rng(n)
    xs, ys = np.sort(rng.random(n) * 4), rng.standard_normal(n)
    for q in sorted({1, 2, 3, n}):
        span = (q + 0.5) / n if q < n else 1.0
        assert R.q_of(n, span) == q
        got, (lo, cnt, inv_h, degree) = _check_loess(xs, ys, span)
        if q == 1:
            assert np.array_equal(got, ys) and (inv_h == 0).all() and (degree == 0).all()       # the point alone
        if q == 2:
            assert (degree == 0).all() and np.array_equal(got, ys)       # the far point has weight 0: the point alone again


def test_a_quadratic_is_reproduced_and_a_constant_stays():
    rng = np.random.default_rng(1)
    xs = np.sort(rng.random(200) * 6 - 3)
    quad = 0.7 * xs * xs - 1.3 * xs + 0.4
    for span in (0.05, 0.3, 0.77, 1.0):
        got, (_, _, _, degree) = _check_loess(xs, quad, span)
        assert (degree == 2).all() and np.abs(got - quad).max() <= 1e-9
        const, _ = _check_loess(xs, np.full(200, 2.5), span)
        assert np.abs(const - 2.5).max() <= 1e-12


def test_ties_longer_than_q_and_two_distinct_abscissae():
    from gridnext_amd import hvg
    rng = np.random.default_rng(2)
    xs = np.sort(np.concatenate([np.full(9, 1.5), rng.random(11) * 3, np.full(2, 2.25)]))
    ys = rng.standard_normal(len(xs))
    got, (lo, cnt, inv_h, degree) = _check_loess(xs, ys, 0.3)            # q = 6 < the block of 9
    block = np.flatnonzero(xs == 1.5)
    assert len(block) == 9 and (inv_h[block] == 0).all() and (cnt[block] == 9).all() and (lo[block] == block[0]).all()
    assert np.allclose(got[block], ys[block].mean(), rtol=0, atol=1e-15) and (degree[block] == 0).all()
    # a window whose positive-weight points hold 2 distinct abscissae takes degree 1: the line through the two groups' means
    xs = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 3.0, 9.0])
    ys = np.array([1.0, 2.0, 3.0, 5.0, 7.0, 0.0, 0.0])
    lo, cnt, inv_h, degree = hvg.loess_windows(xs, 6.5 / 7)              # q = 6: the window of point 0 is [0, 6), h = 3
    assert (lo[0], cnt[0], degree[0]) == (0, 6, 1) and inv_h[0] == 1 / 3.0
    got, _ = _check_loess(xs, ys, 6.5 / 7)
    assert abs(got[0] - 2.0) <= 1e-14                                    # the fitted line at x0 = 0 is the mean of 1, 2, 3
    with pytest.raises(ValueError, match="sorted"):
        hvg.loess_windows(np.array([1.0, 0.5]), 0.5)
    with pytest.raises(ValueError, match="degree must be 0, 1 or 2"):
        hvg.fit_windows(xs, ys, lo, cnt, inv_h, np.full(7, 3, dtype=np.int32))
    with pytest.raises(ValueError, match="inside the points"):
        hvg.fit_windows(xs, ys, lo + 3, cnt, inv_h, degree)


# ------------------------------------------------------------------------------------------------ refusals, frame, symbols
def test_refusals():
    import gridnext_amd as ga
    counts, _ = _counts()
    for bad in (0, 301, 2.5, True):
        with pytest.raises(ValueError, match="n_top_genes must be an integer in \\[1, 300\\]"):
            counts.highly_variable_genes(n_top_genes=bad)
    for bad in (0, -0.1, 1.01):
        with pytest.raises(ValueError, match="span must lie in \\(0, 1\\]"):
            counts.highly_variable_genes(n_top_genes=10, span=bad)
    with pytest.raises(ValueError, match="batch must be None"):
        counts.highly_variable_genes(n_top_genes=10, batch='slide')
    X, obs, genes, _ = R.fixture()
    one = ga.SpotCounts(X[:201], obs.iloc[:201], genes)                  # arr0's 200 spots and a single spot of arr1
    assert one.highly_variable_genes(n_top_genes=10).highly_variable.sum() == 10
    with pytest.raises(ValueError, match="a batch of 1 spots"):
        one.highly_variable_genes(n_top_genes=10, batch='array')
    flat = ga.SpotCounts(np.array([[1, 0, 3, 2], [1, 5, 3, 2], [1, 0, 3, 7]]), obs.iloc[:3], list('abcd'))
    with pytest.raises(ValueError, match="2 genes with a positive variance"):
        flat.highly_variable_genes(n_top_genes=2)
    fresh = ga.SpotCounts(X, obs, genes)
    assert fresh._s.raw and fresh._s.transformed_by is None
    view = fresh.subset_arrays(['arr0'])
    view.normalize_total(1e4)
    assert not fresh._s.raw and not fresh.to('cpu')._s.raw
    with pytest.raises(ValueError, match="rewritten by normalize_total"):
        fresh.highly_variable_genes(n_top_genes=10)
    fresh.log1p()
    with pytest.raises(ValueError, match="rewritten by log1p"):
        view.highly_variable_genes(n_top_genes=10)
    logged = ga.SpotCounts(X, obs, genes).log1p()
    with pytest.raises(ValueError, match="needs raw counts.*log1p"):
        logged.highly_variable_genes(n_top_genes=10)


def test_to_frame_columns():
    counts, _ = _counts()
    got = counts.highly_variable_genes(n_top_genes=N_TOP, batch='array')
    frame = got.to_frame()
    assert list(frame.columns) == ['means', 'variances', 'variances_norm', 'highly_variable_rank', 'highly_variable_nbatches',
                                   'highly_variable']
    assert list(frame.index) == list(counts.gene_ids) and frame['highly_variable'].sum() == N_TOP
    assert np.array_equal(frame['variances_norm'].values, got.variances_norm)
    assert frame['highly_variable_rank'].isna().sum() == (got.highly_variable_nbatches == 0).sum()


def test_new_symbols_are_declared_bound_and_exported():
    from gridnext_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = _lib.lib()
    assert _lib.PARAMS['gnx_sparse_line_clip_moments_f64'] == ['lineptr', 'idx', 'val', 'lines', 'n_lines', 'idx_mask', 'clip',
                                                               'out', 'stream']
    assert _lib.PARAMS['gnx_loess_fit_f64'] == ['xs', 'ys', 'n', 'lo', 'cnt', 'inv_h', 'degree', 'out', 'n_eval', 'stream']
    for name in ('gnx_sparse_line_clip_moments_f64', 'gnx_loess_fit_f64'):
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.PARAMS[name]) and hasattr(handle, name)
    text = open(_lib.HEADER_PATH).read()
    assert 'notebooks/register_hvgs.ipynb' in text and "gridnext/count_datasets.py" in text and 'select_genes' in text
    import gridnext_amd as ga
    assert ga.HighlyVariableGenes is ga.hvg.HighlyVariableGenes and callable(ga.SpotCounts.highly_variable_genes)
    assert callable(ga.visium_datasets.line_clip_moments)
