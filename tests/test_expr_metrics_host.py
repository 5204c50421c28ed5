"""Per-gene expression metrics on the host: the fsum restatement (tests/expr_metrics_ref.py) against a dense numpy evaluation,
`ExpressionMetrics` on host counts against the restatement, its statistics against np.corrcoef and the dense mean, its `loss`
against `SparseMSELoss`, splits of the rows into batches, `top_genes`, `evaluate_expression`, the refusals and the ABI.  No GPU.

Bound of a sum: (n + 16) 2^-53 sum |term|, n the terms plus the calls (tests/expr_metrics_ref.bound).

Tolerance of the statistics, worked out from that bound for targets and predictions in [0, 1] (every mean of terms <= 1, so
each of the five means carries an error e <= (n + 16) 2^-53): pearson = cov / (sp st) moves by at most
e (1 / (sp st) + 1 / (2 sp^2) + 1 / (2 st^2)) to first order for an error e in each moment; three moments enter each factor,
hence 3 (n + 16) 2^-53 (1 / (sp st) + 1 / (2 sp^2) + 1 / (2 st^2)) per gene.  The test asserts that this is below 1e-10 for
every gene of the fixture (401 spots, 300 genes, every gene stored >= 6 times, target std >= 0.108, prediction std >= 0.19 for
the z = N(0, 1) + 2 (t - 0.3) drawn here: the tolerance is <= 1.5e-11 there and the formulas sit 9e-15 from np.corrcoef).  mse = (sum p^2 - 2 sum p t + sum t^2) / n
carries at most (n + 16) 2^-53 (sum p^2 + 2 sum p t + sum t^2) / n from its sums; the dense float64 mean it is compared with
carries as much again, hence twice that."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import expr_metrics_ref as E
import sparse_counts_ref as CR

_made = {}


def _fixture():
    """(counts, scale, z float32 (401, 300), t float32, stored, fsum sums (S, A, N)) - made once, never changed."""
    if 'f' not in _made:
        import gridnext_amd as ga
        X, obs, genes = CR.synthetic_arrays(seed=6, n_arrays=2)
        counts = ga.SpotCounts(X, obs, genes)
        counts.normalize_total(1e4).log1p()
        scale = ga.SparseMSELoss.unit_scale(counts)
        n, G = counts.n_spots, counts.n_genes
        t, stored = E.stored_targets(*(x.numpy() for x in counts._s.csr), None, n, n, None, scale.numpy(), G)
        rng = np.random.default_rng(60)
        z = (rng.standard_normal((n, G)) + 2.0 * (t.astype(np.float64) - 0.3)).astype(np.float32)
        _made['f'] = (counts, scale, z, t, stored, E.sums(z, t, stored, 1))
    return _made['f']


def _metrics(counts, scale, z, batch, **kw):
    import gridnext_amd as ga
    m = ga.ExpressionMetrics(counts, gene_scale=scale, **kw)
    rows = torch.arange(z.shape[0])
    for b in range(0, z.shape[0], batch):
        m.update(torch.from_numpy(z[b:b + batch]), rows[b:b + batch])
    return m


# ------------------------------------------------------------------------------------------------ sums
def test_restatement_is_the_dense_numpy_evaluation():
    counts, scale, z, t, stored, (S, A, N) = _fixture()
    assert z.shape == (401, 300) and (stored.sum(0) >= 6).all() and t.min() >= 0 and t.max() <= 1
    assert np.array_equal(stored, t != 0)                                            # log1p of a count >= 1 is never 0
    p, t64 = E.predictions(z, 1), t.astype(np.float64)
    dense = np.stack([p.sum(0), (p * p).sum(0), t64.sum(0), (t64 * t64).sum(0), (p * t64).sum(0)], axis=1)
    assert bool((np.abs(dense - S) <= E.bound(N, A, 0)).all())
    assert np.array_equal(N[:, 0], np.full(300, 401)) and np.array_equal(N[:, 2], stored.sum(0)) and np.array_equal(N[:, 2], N[:, 4])
    assert np.array_equal(E.predictions(z, 0), z.astype(np.float64))
    # the CSC restatement over one array is the CSR one
    ptr, idx, val = (x.numpy() for x in counts._s.csc[1])
    r0 = int(counts._s.row_start[1])
    tc, kc = E.csc_targets(ptr, idx, val, None, 300, None, scale.numpy(), 401 - r0)
    assert np.array_equal(tc, t[r0:]) and np.array_equal(kc, stored[r0:])


@pytest.mark.parametrize("activation", ['sigmoid', None])
def test_host_sums_lie_within_the_bound_of_fsum(activation):
    counts, scale, z, t, stored, ref = _fixture()
    S, A, N = ref if activation else E.sums(z, t, stored, 0)
    m = _metrics(counts, scale, z, 401, activation=activation)
    got = m.table.numpy()
    assert m.n == 401 and got.shape == (300, 5) and got.dtype == np.float64
    assert bool((np.abs(got - S) <= E.bound(N, A, 1)).all())
    print("host sums, activation %r: largest |err| / (2^-53 sum|term|) = %.3f" % (activation, float((np.abs(got - S) / (E.U * A)).max())))


# ------------------------------------------------------------------------------------------------ statistics
def test_statistics_against_corrcoef_and_the_dense_mean():
    counts, scale, z, t, stored, (S, A, N) = _fixture()
    n = 401
    out = _metrics(counts, scale, z, 401).compute()
    p, t64 = E.predictions(z, 1), t.astype(np.float64)
    sp, st = p.std(0), t64.std(0)
    print("smallest prediction std %.4f, smallest target std %.4f" % (sp.min(), st.min()))
    assert st.min() >= 0.108                                                          # the fixture's, whatever z is drawn
    tol = 3 * (n + 16) * E.U * (1 / (sp * st) + 1 / (2 * sp * sp) + 1 / (2 * st * st))
    assert tol.max() < 1e-10                                                          # the tolerance cannot hide a failure
    want = np.array([np.corrcoef(p[:, g], t64[:, g])[0, 1] for g in range(300)])
    err = np.abs(out['pearson'] - want)
    print("pearson: largest |difference| to corrcoef %.3g, tolerance <= %.3g" % (err.max(), tol.max()))
    assert bool((err <= tol).all())
    mse = ((p - t64) ** 2).mean(0)
    mtol = 2 * (n + 16) * E.U * (S[:, 1] + 2 * S[:, 4] + S[:, 3]) / n
    print("mse: largest relative difference to the dense mean %.3g" % float((np.abs(out['mse'] - mse) / mse).max()))
    assert bool((np.abs(out['mse'] - mse) <= mtol).all())
    assert out['n'] == n and np.allclose(out['mean_pred'], p.mean(0), rtol=1e-13) and np.allclose(out['mean_target'], t64.mean(0), rtol=1e-13)
    assert np.allclose(out['r2'], 1 - mse / t64.var(0), rtol=0, atol=1e-10 * (1 + mse / t64.var(0)))
    assert abs(out['loss'] - mse.mean()) <= 1e-13 * mse.mean()


def test_loss_is_the_criterions_on_all_rows_at_once():
    import gridnext_amd as ga
    counts, _, z, _, _, _ = _fixture()
    m = ga.ExpressionMetrics(counts, gene_scale=None)
    z64 = torch.from_numpy(z).double()
    rows = torch.arange(401)
    want = float(ga.SparseMSELoss(counts, gene_scale=None)(z64, rows))
    got = m.update(z64, rows).compute()['loss']
    print("loss %.17g, criterion %.17g, relative difference %.3g" % (got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-12 * want


# ------------------------------------------------------------------------------------------------ splits
def test_batches_of_1_7_and_all_agree_within_the_bound():
    counts, scale, z, t, stored, (S, A, N) = _fixture()
    tables = {b: _metrics(counts, scale, z, b).table.numpy().copy() for b in (1, 7, 401)}
    calls = {1: 401, 7: 58, 401: 1}
    for b in (1, 7, 401):
        assert bool((np.abs(tables[b] - S) <= E.bound(N, A, calls[b])).all()), b
    for a, b in ((1, 7), (7, 401), (1, 401)):
        assert bool((np.abs(tables[a] - tables[b]) <= E.bound(N, A, calls[a]) + E.bound(N, A, calls[b])).all())
    rows = torch.from_numpy(np.random.default_rng(1).permutation(401))
    import gridnext_amd as ga
    m = ga.ExpressionMetrics(counts, gene_scale=scale)
    for b in range(0, 401, 50):                                                      # shuffled rows, int32
        m.update(torch.from_numpy(z)[rows[b:b + 50]], rows[b:b + 50].int())
    assert m.n == 401 and bool((np.abs(m.table.numpy() - S) <= E.bound(N, A, 9)).all())
    assert m.reset().n == 0 and not m.table.any() and np.isnan(m.compute()['pearson']).all() and np.isnan(m.compute()['loss'])


def _with_an_unseen_gene():
    import gridnext_amd as ga
    X, obs, genes = CR.synthetic_arrays(seed=4, n_arrays=2, n_genes=40, n_spots=30)
    X = X.tolil()
    X[:, 7] = 0
    counts = ga.SpotCounts(X.tocsr(), obs, genes)
    counts.normalize_total(1e4).log1p()
    return counts, genes


def test_a_gene_never_seen_and_a_constant_prediction_give_nan():
    import gridnext_amd as ga
    counts, _ = _with_an_unseen_gene()
    n = counts.n_spots
    z = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 40)))
    z[:, 11] = 0.75                                                                  # a constant prediction
    out = ga.ExpressionMetrics(counts, gene_scale=ga.SparseMSELoss.unit_scale(counts)).update(z, torch.arange(n)).compute()
    assert np.isnan(out['pearson'][7]) and np.isnan(out['r2'][7]) and out['mean_target'][7] == 0 and np.isfinite(out['mse'][7])
    assert np.isnan(out['pearson'][11]) and np.isfinite(out['r2'][11])
    assert np.isnan(out['pearson'][26]) and np.isnan(out['r2'][26])                  # the fixture's own unseen gene
    rest = np.ones(40, bool)
    rest[[7, 11, 26]] = False
    assert np.isfinite(out['pearson'][rest]).all() and np.isfinite(out['r2'][rest]).all() and np.isfinite(out['loss'])
    assert (np.abs(out['pearson'][rest]) <= 1).all()


def test_top_genes_orders_best_first_nans_last_ties_by_index():
    import gridnext_amd as ga
    counts, _ = _with_an_unseen_gene()
    n = counts.n_spots
    z = torch.from_numpy(np.random.default_rng(3).standard_normal((n, 40)))
    z[:, 20] = z[:, 5] = 0.0                                                         # two more NaNs
    m = ga.ExpressionMetrics(counts).update(z, torch.arange(n))
    out = m.compute()
    for by, sign in (('pearson', -1), ('r2', -1), ('mse', 1)):
        v = out[by]
        want = sorted(range(40), key=lambda g: (bool(np.isnan(v[g])), 0.0 if np.isnan(v[g]) else sign * v[g], g))
        got = m.top_genes(40, by=by)
        assert got.dtype == np.int64 and got.tolist() == want and m.top_genes(6, by=by).tolist() == want[:6]
    assert m.top_genes(40).tolist()[-4:] == [5, 7, 20, 26] and m.top_genes(3).tolist() == m.top_genes(3, by='pearson').tolist()
    # ties by index: a table with equal rows
    m.table[:] = m.table[0]
    assert m.top_genes(5).tolist() == [0, 1, 2, 3, 4] and m.top_genes(5, by='mse').tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="by must be"):
        m.top_genes(3, by='spearman')


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_both_sides():
    import gridnext_amd as ga
    counts, _ = _with_an_unseen_gene()
    view = counts.subset_arrays(['arr1'])
    m = ga.ExpressionMetrics(view)
    r0, r1 = (int(v) for v in counts._s.row_start[1:3])
    z = torch.zeros(2, 40)
    m.update(z, torch.tensor([r0, r1 - 1]))
    before = m.table.clone()
    with pytest.raises(ValueError, match="repeated row"):
        m.update(z, torch.tensor([r0, r0]))
    with pytest.raises(ValueError, match="bound arrays"):
        m.update(z, torch.tensor([r0, r0 - 1]))                                      # a row of arr0: not of the bound view
    with pytest.raises(ValueError, match="bound arrays"):
        m.update(z, torch.tensor([r0, r1]))                                          # outside the storage
    with pytest.raises(ValueError, match="bound arrays"):
        m.update(z, torch.tensor([-1, r0]))
    with pytest.raises(ValueError, match=r"z must be \(B, 40\), one column per selected gene, got \(2, 39\)"):
        m.update(torch.zeros(2, 39), torch.tensor([r0, r0 + 1]))
    with pytest.raises(ValueError, match=r"floating point with the counts on cpu, got torch.int64"):
        m.update(torch.zeros(2, 40, dtype=torch.int64), torch.tensor([r0, r0 + 1]))
    with pytest.raises(ValueError, match="z is on meta, the counts are on cpu"):
        m.update(torch.zeros(2, 40, device='meta'), torch.tensor([r0, r0 + 1]))
    with pytest.raises(ValueError, match="rows must be"):
        m.update(z, torch.tensor([r0]))
    with pytest.raises(ValueError, match="rows must be"):
        m.update(z, torch.tensor([1.0, 2.0]))
    assert m.n == 2 and torch.equal(m.table, before)                                 # a refused batch changes nothing
    with pytest.raises(ValueError, match="activation"):
        ga.ExpressionMetrics(counts, activation='relu')
    with pytest.raises(ValueError, match=r"gene_scale must be \(40,\)"):
        ga.ExpressionMetrics(counts, gene_scale=torch.ones(39))
    with pytest.raises(TypeError, match="SpotCounts"):
        ga.ExpressionMetrics(object())
    free = ga.ExpressionMetrics(view, check_rows=False)                              # unchecked: a row of arr0 gets its target
    assert free.update(z, torch.tensor([r0 - 1, r0])).n == 2
    # a gene subset in a permuted order: the view's channels
    genes = list(counts.gene_ids)
    sub = counts.subset_genes([genes[g] for g in (9, 3, 21)])
    zz = torch.from_numpy(np.random.default_rng(4).standard_normal((counts.n_spots, 40)))
    full = ga.ExpressionMetrics(counts).update(zz, torch.arange(counts.n_spots)).table
    part = ga.ExpressionMetrics(sub).update(zz[:, [9, 3, 21]], torch.arange(counts.n_spots)).table
    assert torch.equal(part, full[[9, 3, 21]])


# ------------------------------------------------------------------------------------------------ the pass, the ABI
def test_evaluate_expression_equals_manual_updates_and_restores_the_mode():
    import gridnext_amd as ga
    counts, _ = _with_an_unseen_gene()
    n = counts.n_spots
    torch.manual_seed(0)
    model = nn.Sequential(nn.Flatten(), nn.Linear(12, 40), nn.Dropout(0.5))           # dropout: eval() matters
    x = torch.randn(n, 3, 2, 2)
    rows = torch.arange(n)
    loader = [(x[b:b + 8], rows[b:b + 8], torch.zeros(len(rows[b:b + 8]))) for b in range(0, n, 8)]
    scale = ga.SparseMSELoss.unit_scale(counts)
    for training in (True, False):
        model.train(training)
        m = ga.ExpressionMetrics(counts, gene_scale=scale)
        m.update(torch.zeros(1, 40), rows[:1])                                       # the pass resets what was there
        out = ga.evaluate_expression(model, loader, m)
        assert model.training is training
        model.eval()
        ref = ga.ExpressionMetrics(counts, gene_scale=scale)
        with torch.no_grad():
            for xb, rb, _ in loader:
                ref.update(model(xb), rb)
        want = ref.compute()
        assert out['n'] == n and torch.equal(m.table, ref.table)
        assert all(np.array_equal(out[k], want[k], equal_nan=True) for k in want)

    class Boom(nn.Module):
        def forward(self, x):
            raise KeyError('boom')
    boom = Boom().train()
    with pytest.raises(KeyError):
        ga.evaluate_expression(boom, loader, m)
    assert boom.training


def test_entry_points_are_declared_bound_and_exported():
    from gridnext_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = _lib.lib()
    assert _lib.PARAMS['gnx_act_col_moments_f64'] == ['z', 'ldz', 'B', 'G', 'activation', 'M', 'ld_m', 'accumulate', 'stream']
    assert _lib.PARAMS['gnx_sparse_pred_moments_f64'] == ['lineptr', 'idx', 'val', 'gene_lines', 'n_channels', 'pos_of_idx',
                                                          'gene_scale', 'z', 'ldz', 'activation', 'M', 'ld_m', 'accumulate', 'stream']
    for name, n in (('gnx_act_col_moments_f64', 9), ('gnx_sparse_pred_moments_f64', 14)):
        assert len(_lib.SIGNATURES[name][1]) == n and hasattr(handle, name)
    assert _lib.CONSTANTS['GNX_ACT_NONE'] == 0 and _lib.CONSTANTS['GNX_ACT_SIGMOID'] == 1
    header = open(_lib.HEADER_PATH).read()
    block = header[header.index('Per-gene moments of an expression prediction'):]
    for name in ('gnx_act_col_moments_f64', 'gnx_sparse_pred_moments_f64'):
        assert '%s (notebooks/counts_from_img.ipynb' % name in block
    import gridnext_amd as ga
    assert ga.ExpressionMetrics is ga.expression.ExpressionMetrics and ga.evaluate_expression is ga.expression.evaluate_expression
