"""`SpotCounts.fit_pca` / `CountPCA` / `use_pcs=` with the counts on the host, against tests/sparse_pca_ref.py and against sklearn's
full-SVD PCA of the dense, centred and scaled float64 matrix.  Fixture: 600 spots in 2 arrays x 96 genes with six planted
factors (sparse_pca_ref.fixture) after normalize_total(1e4).log1p().

Bars (sparse_pca_ref): eps = G 2^-52 lambda_1; eigenvalues within eps (Weyl), ratios within eps / sum lambda, the six separated
components within sin <= 2 eps / gap_i (Davis-Kahan), the projector of the first 8 within 2 eps / its gap.  The transform is the
sparse layer's: within gamma(n) T of the float64 value of its own fp32 weights (tests/sparse_linear_ref.py), and within
(gamma(n) + 3 u) T of sklearn's transform: the weight and the bias are rounded to fp32 once each, one u is left for the
difference between the two float64 fits (measured below 1e-13).

Measured here (printed by the tests): see the README's count-PCA section."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

import sparse_counts_ref as R
import sparse_linear_ref as SL
import sparse_pca_ref as P

_made = {}


def _counts():
    """(host counts after the recipe, the dense float64 matrix of the same values); built once, never modified."""
    if 'c' not in _made:
        import gridnext_amd as ga
        c = ga.SpotCounts(*P.fixture())
        c.normalize_total(1e4).log1p()
        dense = P.fixture_dense()
        rows = torch.arange(c.n_spots, dtype=torch.int32)
        from gridnext_amd import visium_datasets as V
        out = torch.empty((c.n_spots, c.n_genes))
        V.expand(c._s.csr, rows, c.n_spots, None, out, c.n_genes)
        assert np.array_equal(out.numpy(), dense)                                        # the package's values are the helper's
        _made['c'] = (c, dense.astype(np.float64))
    return _made['c']


# ------------------------------------------------------------------------------------------------ the Gram matrix
def test_gram_restatement_against_scipy_and_exact_on_raw_counts():
    import scipy.sparse as sp
    from gridnext_amd import count_pca
    import gridnext_amd as ga
    c, X = _counts()
    Xs = sp.csr_matrix(X)
    scipy64 = np.asarray((Xs.T @ Xs).todense())
    want, terms, T = P.gram_fsum_dense(X)
    bound = P.gram_bound(terms, T)                                                       # per element: n its own terms
    assert 60 < np.median(terms) < 120 and terms.max() <= 600
    assert (np.abs(P.gram64(X) - want) <= bound).all() and (np.abs(scipy64 - want) <= bound).all()
    got = count_pca.gram(c)
    assert got.dtype == np.float64 and np.array_equal(got, got.T)
    print("host Gram against fsum: largest |err| / (n 2^-53 sum |v u|) = %.4f" % float((np.abs(got - want) / bound).max()))
    assert (np.abs(got - want) <= bound).all()
    # raw integer counts: every product and every partial sum is an integer below 2^53, exact in any order
    raw = ga.SpotCounts(*P.fixture())
    counts = P.planted_counts().astype(np.int64)
    assert np.array_equal(count_pca.gram(raw), (counts.T @ counts).astype(np.float64)) and int((counts.T @ counts).max()) < 2 ** 53
    # a lazy view: its genes in its order, its arrays
    ids = [raw.gene_ids[g] for g in (5, 2, 90, 17)]
    view = raw.subset_genes(ids).subset_arrays(['arr1'])
    sub = counts[300:][:, [5, 2, 90, 17]]
    assert np.array_equal(count_pca.gram(view), (sub.T @ sub).astype(np.float64))
    # the helper's statement of the kernel's arithmetic is the same product
    m, mc = sp.csr_matrix(counts.astype(np.float32)), sp.csc_matrix(counts[300:].astype(np.float32))
    csr = (m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data)
    csc = (mc.indptr.astype(np.int64), mc.indices.astype(np.int32), mc.data)
    chan = np.full(96, -1, dtype=np.int32)
    chan[[5, 2, 90, 17]] = np.arange(4)
    assert np.array_equal(P.gram_int(csc, 300, np.array([5, 2, 90, 17], np.int32), 4, csr, 300, chan), sub.T @ sub)
    fs, n, T = P.gram_fsum(csc, 300, np.array([5, 2, 90, 17], np.int32), 4, csr, 300, chan)
    assert np.array_equal(fs, (sub.T @ sub).astype(np.float64)) and np.array_equal(T, fs) and n.max() <= 300


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("scale", [True, False])
def test_fit_against_sklearn_full_svd(scale):
    c, X = _counts()
    pca = c.fit_pca(scale=scale)
    P.check_fit(pca, X, scale, "host fit, scale=%s" % scale)
    ref = P.fit64(X, scale)
    assert np.allclose(pca.components_.numpy()[:P.PLANTED], ref['components'][:P.PLANTED], rtol=0, atol=1e-12)
    assert list(pca.gene_ids) == list(c.gene_ids)
    if not scale:
        assert torch.equal(pca.scale_, torch.ones(96, dtype=torch.float64))
    few = c.fit_pca(n_components=5, scale=scale)
    assert few.components_.shape == (5, 96) and torch.equal(few.components_, pca.components_[:5])
    assert torch.equal(few.explained_variance_ratio_, pca.explained_variance_ratio_[:5])   # over the sum of ALL eigenvalues


def test_fit_on_one_array_of_two_and_on_a_gene_view():
    c, X = _counts()
    one = c.subset_arrays(['arr1'])
    P.check_fit(one.fit_pca(), X[300:], True, "host fit on arr1 alone")
    ids = [c.gene_ids[g] for g in range(95, 15, -1)]                                      # 80 genes, reversed
    view = c.subset_genes(ids)
    pca = view.fit_pca()
    ref = P.fit64(X[:, list(range(95, 15, -1))])
    assert list(pca.gene_ids) == ids and pca.components_.shape == (80, 80)
    assert np.allclose(pca.explained_variance_.numpy(), ref['variance'], rtol=0, atol=P.eps_of(ref['variance'][0], 80))


def test_sign_rule_and_n_pcs_for():
    c, X = _counts()
    pca = c.fit_pca()
    V = pca.components_.numpy()
    first = np.argmax(np.abs(V), axis=1)
    assert (V[np.arange(len(V)), first] > 0).all()
    tie = np.array([[0.5, -0.5, 0.1], [-0.5, 0.5, 0.1], [0.1, 0.2, -0.3]])
    from gridnext_amd import count_pca
    for rule in (count_pca.sign_rule, P.sign_rule):                                       # the package's step and the helper's
        assert np.array_equal(rule(tie), np.array([[0.5, -0.5, 0.1], [0.5, -0.5, -0.1], [-0.1, -0.2, 0.3]]))
    cum = np.cumsum(pca.explained_variance_ratio_.numpy())
    k = pca.n_pcs_for(0.5)
    assert k == int(np.where(cum > 0.5)[0][0]) + 1 and cum[k - 1] > 0.5 and (k == 1 or cum[k - 2] <= 0.5)
    assert pca.n_pcs_for(0.0) == 1 and pca.n_pcs_for(cum[3]) == 5
    with pytest.raises(ValueError, match="explain"):
        c.fit_pca(n_components=2).n_pcs_for(0.99)


def test_constant_gene_under_scale():
    """A gene that is the same in every spot (here: never seen) has std 0: scale_ 1, a zero row and column of the covariance,
    no influence on the others."""
    import gridnext_amd as ga
    import scipy.sparse as sp
    X, obs, genes = P.fixture()
    dense = np.asarray(X.todense())
    wide = np.concatenate([dense[:, :40], np.zeros((600, 1)), dense[:, 40:]], axis=1)
    c = ga.SpotCounts(sp.csr_matrix(wide), obs, genes[:40] + ['CONST'] + genes[40:])
    # normalise over the 96 real genes the fixture has: the constant gene adds nothing to any total
    c.normalize_total(1e4).log1p()
    pca = c.fit_pca(scale=True)
    base = _counts()[0].fit_pca(scale=True)
    assert float(pca.scale_[40]) == 1.0 and float(pca.mean_[40]) == 0.0
    V = pca.components_.numpy()
    assert np.abs(V[:96, 40]).max() <= 1e-12                                              # not in any component with variance
    rest = np.delete(V[:P.PLANTED], 40, axis=1)
    eps = P.eps_of(float(base.explained_variance_[0]), 97)
    gap = P.gaps(base.explained_variance_.numpy())
    assert np.abs(pca.explained_variance_.numpy()[:95] - base.explained_variance_.numpy()[:95]).max() <= eps
    assert all(P.sin_angle(rest[i], base.components_.numpy()[i]) <= 2 * eps / gap[i] for i in range(P.PLANTED))


def test_every_refusal():
    import gridnext_amd as ga
    c, _ = _counts()
    for bad in (0, -1, 97, 2.0, 'all', True):
        with pytest.raises(ValueError, match="n_components"):
            c.fit_pca(n_components=bad)
    few = c.subset_arrays(['arr0'])
    assert few.fit_pca(n_components=96).components_.shape == (96, 96)
    flat = ga.SpotCounts(np.full((4, 3), 2.0), P.fixture()[1].iloc[:4], ['a', 'b', 'c'])
    with pytest.raises(ValueError, match="no variance"):
        flat.fit_pca(scale=True)
    with pytest.raises(ValueError, match="%d bytes" % (8 * 96 * 96)):
        c.fit_pca(max_genes=95)
    assert c.fit_pca(max_genes=96).components_.shape == (96, 96)
    pca = c.fit_pca(n_components=10)
    other = ga.SpotCounts(*P.fixture())
    view = c.subset_genes([c.gene_ids[g] for g in (0, 1, 3, 2)] + list(c.gene_ids[4:]))
    for call in (pca.to_layer, pca.transform):
        with pytest.raises(ValueError, match="another storage"):
            call(other)
        with pytest.raises(ValueError, match="gene 2 is ENSG00003.*ENSG00002"):
            call(view)
        with pytest.raises(ValueError, match="gene 5 is None"):
            call(c.subset_genes(list(c.gene_ids[:5])))
        with pytest.raises(ValueError, match="n_pcs"):
            call(c, n_pcs=11)
    # the datasets' keyword
    for cls in (ga.SparseCountDataset, ga.SparseCountGridDataset):
        with pytest.raises(ValueError, match="pca"):
            cls(c, use_pcs=3)
        with pytest.raises(ValueError, match="use_pcs"):
            cls(c, use_pcs=11, pca=pca)
        with pytest.raises(ValueError, match="another storage"):
            cls(other, use_pcs=3, pca=pca)
        with pytest.raises(ValueError, match="gene 2 is"):
            cls(view, use_pcs=3, pca=pca)
    with pytest.raises(ValueError, match="as_rows"):
        ga.SparseCountDataset(c, use_pcs=3, pca=pca, as_rows=True)
    layer = pca.to_layer(c, n_pcs=3)
    with pytest.raises(ValueError, match="first_layer"):
        ga.SparseCountGridDataset(c, use_pcs=3, pca=pca, first_layer=layer)


# ------------------------------------------------------------------------------------------------ transform and use_pcs
def _layer_float64(layer, X):
    """(the float64 value of the layer's own fp32 weights on the dense rows X, T, n)."""
    W, b = layer.weight.detach().double().numpy(), layer.bias.detach().double().numpy()
    return X @ W + b, np.abs(X) @ np.abs(W) + np.abs(b), (X != 0).sum(1)


@pytest.mark.parametrize("scale", [True, False])
def test_transform_and_to_layer(scale):
    c, X = _counts()
    pca = c.fit_pca(scale=scale)
    k = pca.n_pcs_for(0.5)
    state = torch.random.get_rng_state()
    layer = pca.to_layer(c, n_pcs=k)
    assert torch.equal(torch.random.get_rng_state(), state)                               # no draw of the global RNG is consumed
    assert layer.weight.shape == (96, k) and layer.weight.dtype == torch.float32
    assert not any(p.requires_grad for p in layer.parameters())
    W, b = pca.affine(k)
    V, sc, mean = pca.components_.numpy()[:k], pca.scale_.numpy(), pca.mean_.numpy()
    assert np.array_equal(W, (V / sc).T) and np.array_equal(b, -(mean / sc) @ V.T)
    assert np.array_equal(layer.weight.numpy(), W.astype(np.float32)) and np.array_equal(layer.bias.numpy(), b.astype(np.float32))
    z = pca.transform(c, n_pcs=k)
    assert z.shape == (600, k) and z.dtype == torch.float32
    want, T, n = _layer_float64(layer, X)
    err = np.abs(z.numpy() - want)
    print("host transform scale=%s, k=%d: largest |err| / (gamma(n) T) = %.3f" % (scale, k, (err / (SL.gamma(n)[:, None] * T)).max()))
    assert (err <= SL.gamma(n)[:, None] * T).all()
    sk, _, _ = P.sklearn_fit(X, scale)
    zs = sk.transform((X - mean) / sc)[:, :k] * np.sign((sk.components_[:k] * V).sum(1))
    T64 = np.abs(X) @ np.abs(W) + np.abs(b)
    err = np.abs(z.numpy() - zs)
    print("against sklearn's transform: largest |err| / ((gamma(n) + 3 u) T) = %.3f" % (err / ((SL.gamma(n)[:, None] + 3 * SL.U) * T64)).max())
    assert (err <= (SL.gamma(n)[:, None] + 3 * SL.U) * T64).all()
    # a view of one array: its spots, in its order; every component by default
    z1 = pca.transform(c.subset_arrays(['arr1']))
    assert z1.shape == (300, 96) and torch.equal(z1[:, :k], z[300:])


def test_use_pcs_items_and_unchanged_defaults():
    import gridnext_amd as ga
    c, X = _counts()
    pca = c.fit_pca()
    k = 7
    z = pca.transform(c, n_pcs=k)
    spots = ga.SparseCountDataset(c, use_pcs=k, pca=pca)
    plain = ga.SparseCountDataset(c)
    assert len(spots) == len(plain) == 600
    picks = [3, 599, 0, 300]
    for (x, y), p in zip(spots.__getitems__(picks), picks):
        assert x.shape == (k,) and x.dtype == torch.float32 and torch.equal(x, z[p]) and torch.equal(y, plain[p][1])
    assert torch.equal(spots[-1][0], z[599])
    xb, yb = next(iter(DataLoader(spots, batch_size=9)))
    assert torch.equal(xb, z[:9]) and yb.dtype == torch.int64
    grids = ga.SparseCountGridDataset(c, use_pcs=k, pca=pca)
    plain_grids = ga.SparseCountGridDataset(c)
    for a in range(2):
        x, y = grids[a]
        cells, labels = grids._array(a)
        assert x.shape == (k, 78, 64) and x.dtype == torch.float32 and torch.equal(y, plain_grids[a][1])
        flat = x.reshape(k, -1).t()
        assert torch.equal(flat[cells.long()], z[300 * a:300 * (a + 1)])
        empty = torch.ones(78 * 64, dtype=torch.bool)
        empty[cells.long()] = False
        assert int(empty.sum()) == 78 * 64 - 300 and torch.equal(flat[empty], torch.zeros(int(empty.sum()), k))
        assert float(pca.to_layer(c, k).bias.abs().min()) > 0                             # 0, not the layer's bias
    # the keywords left at their defaults: the items of the classes as they were
    for a, b in ((ga.SparseCountDataset(c, use_pcs=None, pca=None), plain), (ga.SparseCountDataset(c, pca=pca), plain)):
        assert a.pc_layer is None and all(torch.equal(a[p][0], b[p][0]) and torch.equal(a[p][1], b[p][1]) for p in picks)
    for a in (ga.SparseCountGridDataset(c, use_pcs=None, pca=None), ga.SparseCountGridDataset(c, pca=pca)):
        assert a.pc_layer is None and torch.equal(a[1][0], plain_grids[1][0]) and torch.equal(a[1][1], plain_grids[1][1])
    layer = pca.to_layer(c, k)
    with_bias = ga.SparseCountGridDataset(c, first_layer=layer)[1][0].reshape(k, -1).t()          # cells, empty: array 1's
    assert torch.equal(with_bias[cells.long()], z[300:]) and torch.equal(with_bias[empty], layer.bias.expand(int(empty.sum()), k))


def test_one_epoch_of_train_spotwise_on_pc_items():
    import gridnext_amd as ga
    c, _ = _counts()
    pca = c.subset_arrays(['arr0']).fit_pca()
    k = pca.n_pcs_for(0.5)
    classes = ga.SparseCountDataset(c).classes
    train = ga.SparseCountDataset(c.subset_arrays(['arr0']), classes=classes, use_pcs=k, pca=pca)
    val = ga.SparseCountDataset(c.subset_arrays(['arr1']), classes=classes, use_pcs=k, pca=pca)
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(k, 16), nn.ReLU(), nn.Linear(16, len(classes)))
    loaders = {'train': DataLoader(train, batch_size=50, shuffle=True, generator=torch.Generator().manual_seed(1)),
               'val': DataLoader(val, batch_size=50)}
    with contextlib.redirect_stdout(io.StringIO()):
        model, vh, th = ga.train_spotwise(model, loaders, nn.CrossEntropyLoss(), torch.optim.Adam(model.parameters(), lr=1e-3),
                                          num_epochs=1)
    assert len(th) == len(vh) == 1 and np.isfinite(th[0]) and np.isfinite(vh[0])
