"""`SpotCounts.fit_pca`, `CountPCA` and `use_pcs=` with the counts resident on a HIP device: the device and the host Gram matrix against math.fsum per element,
the device fit against the host fit and against sklearn under the bars of tests/test_sparse_pca_host.py, the transform against
the float64 value of the layer's own weights within gamma(n) T (tests/sparse_linear_ref.py), the launches per item, the two
training loops against the same loops fed the same tensors, the memory condition and determinism.  Fixture: sparse_pca_ref's
600 spots x 96 genes, normalised and log1p'd ON THE DEVICE; the host side of every comparison is `.to('cpu')` of the same values.

Measured on an MI355X (printed by the tests): see the README's count-PCA section."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

import sparse_linear_ref as SL
import sparse_pca_ref as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K, C = 8, 4
_made = {}


def _recipe():
    """(device counts after the recipe, the same values on the host, the dense float64 matrix of them); built once."""
    if 'r' not in _made:
        import gridnext_amd as ga
        from gridnext_amd import visium_datasets as V
        dev = ga.SpotCounts(*P.fixture()).to(DEV)
        dev.normalize_total(1e4).log1p()
        host = dev.to('cpu')
        out = torch.empty((host.n_spots, host.n_genes))
        V.expand(host._s.csr, torch.arange(host.n_spots, dtype=torch.int32), host.n_spots, None, out, host.n_genes)
        _made['r'] = (dev, host, out.double().numpy())
    return _made['r']


def _fits():
    if 'f' not in _made:
        dev, host, _ = _recipe()
        _made['f'] = (dev.fit_pca(), host.fit_pca())
    return _made['f']


def _recorded(monkeypatch, fn):
    """(fn(), the names of the launches it made through _lib.call)."""
    from gridnext_amd import _lib
    seen, real = [], _lib.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    try:
        return fn(), seen
    finally:
        monkeypatch.setattr(_lib, 'call', real)


def test_device_gram_against_the_host_gram(monkeypatch):
    from gridnext_amd import count_pca
    dev, host, X = _recipe()
    got, seen = _recorded(monkeypatch, lambda: count_pca.gram(dev))
    assert seen == ['gnx_sparse_gram_f64'] * 2                                           # one launch per array of the view
    want, terms, T = P.gram_fsum_dense(X)
    bound = P.gram_bound(terms, T)                                                       # per element: n its own terms
    err, err_host = np.abs(got - want), np.abs(count_pca.gram(host) - want)
    print("Gram against fsum, largest |err| / (n 2^-53 sum |v u|) with n the element's terms (median %d): device %.4f, host %.4f"
          % (np.median(terms), float((err / bound).max()), float((err_host / bound).max())))
    assert (err <= bound).all() and (err_host <= bound).all() and np.array_equal(got, got.T)
    view = dev.subset_genes([dev.gene_ids[g] for g in (40, 3, 95, 0, 17)]).subset_arrays(['arr1'])
    w5, n5, T5 = P.gram_fsum_dense(X[300:][:, [40, 3, 95, 0, 17]])
    assert (np.abs(count_pca.gram(view) - w5) <= P.gram_bound(n5, T5)).all()
    import gridnext_amd as ga
    raw = ga.SpotCounts(*P.fixture()).to(DEV)
    counts = P.planted_counts().astype(np.int64)
    assert np.array_equal(count_pca.gram(raw), (counts.T @ counts).astype(np.float64))   # raw counts: exact


@pytest.mark.parametrize("scale", [True, False])
def test_device_fit_against_the_host_fit_and_sklearn(scale):
    dev, host, X = _recipe()
    pd_, ph = (dev.fit_pca(scale=scale), host.fit_pca(scale=scale)) if not scale else _fits()
    P.check_fit(pd_, X, scale, "device fit, scale=%s" % scale)
    lam = ph.explained_variance_.numpy()
    eps, gap = P.eps_of(lam[0], 96), P.gaps(lam)
    assert np.abs(pd_.explained_variance_.numpy() - lam).max() <= eps
    assert all(P.sin_angle(pd_.components_.numpy()[i], ph.components_.numpy()[i]) <= 2 * eps / gap[i] for i in range(P.PLANTED))
    assert torch.equal(pd_.mean_, ph.mean_) or np.allclose(pd_.mean_.numpy(), ph.mean_.numpy(), rtol=0, atol=1e-14)
    one = dev.subset_arrays(['arr1']).fit_pca(scale=scale)
    P.check_fit(one, X[300:], scale, "device fit on arr1 alone, scale=%s" % scale)


def test_transform_and_to_layer(monkeypatch):
    dev, host, X = _recipe()
    pca, _ = _fits()
    k = pca.n_pcs_for(0.5)
    layer = pca.to_layer(dev, n_pcs=k)
    assert layer.weight.is_cuda and layer.weight.shape == (96, k) and not any(p.requires_grad for p in layer.parameters())
    z, seen = _recorded(monkeypatch, lambda: pca.transform(dev, n_pcs=k))
    assert seen == ['gnx_sparse_linear_fwd_f32']                                         # one forward launch
    assert z.is_cuda and z.shape == (600, k) and z.dtype == torch.float32
    W, b = layer.weight.double().cpu().numpy(), layer.bias.double().cpu().numpy()
    want, T, n = X @ W + b, np.abs(X) @ np.abs(W) + np.abs(b), (X != 0).sum(1)
    err = np.abs(z.double().cpu().numpy() - want)
    print("device transform, k=%d: largest |err| / (gamma(n) T) = %.3f" % (k, float((err / (SL.gamma(n)[:, None] * T)).max())))
    assert (err <= SL.gamma(n)[:, None] * T).all()
    z1 = pca.transform(dev.subset_arrays(['arr1']), n_pcs=k)
    assert torch.equal(z1, z[300:])
    with pytest.raises(ValueError, match="another storage"):
        pca.transform(host)


def test_use_pcs_items_of_both_datasets(monkeypatch):
    import gridnext_amd as ga
    dev, _, _ = _recipe()
    pca, _ = _fits()
    z = pca.transform(dev, n_pcs=K)
    spots = ga.SparseCountDataset(dev, use_pcs=K, pca=pca)
    picks = [5, 599, 0, 300, 301]
    items, seen = _recorded(monkeypatch, lambda: spots.__getitems__(picks))
    assert seen == ['gnx_sparse_linear_fwd_f32']                                         # one launch per spot batch
    plain = ga.SparseCountDataset(dev)
    for (x, y), p in zip(items, picks):
        assert x.is_cuda and x.shape == (K,) and torch.equal(x, z[p]) and torch.equal(y, plain[p][1])
    grids = ga.SparseCountGridDataset(dev, use_pcs=K, pca=pca)
    plain_grids = ga.SparseCountGridDataset(dev)
    grids._array(0), grids._array(1)
    for a in range(2):
        (x, y), seen = _recorded(monkeypatch, lambda: grids[a])
        assert 1 <= len(seen) <= 2 and seen[0] == 'gnx_sparse_linear_fwd_f32'             # at most two launches per grid item
        cells, _ = grids._array(a)
        assert x.is_cuda and x.shape == (K, 78, 64) and x.dtype == torch.float32 and torch.equal(y, plain_grids[a][1])
        flat = x.reshape(K, -1).t()
        assert torch.equal(flat[cells.long()], z[300 * a:300 * (a + 1)])
        empty = torch.ones(78 * 64, dtype=torch.bool, device=DEV)
        empty[cells.long()] = False
        assert int(empty.sum()) == 78 * 64 - 300 and int((flat[empty] != 0).sum()) == 0
        assert int((flat[empty].view(torch.int32) != 0).sum()) == 0                      # +0.0, not the bias and not -0.0


def _spot_loop(train, val):
    import gridnext_amd as ga
    torch.manual_seed(4)
    model = nn.Sequential(nn.Linear(K, 32), nn.BatchNorm1d(32), nn.ReLU(), nn.Linear(32, C))
    dl = {'train': DataLoader(train, batch_size=64, shuffle=True, generator=torch.Generator().manual_seed(2)),
          'val': DataLoader(val, batch_size=64)}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        model, vh, th = ga.train_spotwise(model, dl, nn.CrossEntropyLoss(), opt, num_epochs=2)
    return th, vh, {k: v.detach().clone() for k, v in model.state_dict().items()}


def _grid_loop(train, val):
    import gridnext_amd as ga
    torch.manual_seed(3)
    f = nn.Sequential(nn.Linear(K, 16), nn.BatchNorm1d(16), nn.ReLU(), nn.Linear(16, C))
    for p in f.parameters():
        p.requires_grad = False
    m = ga.GridNetHexOddr(f, (K,), (78, 64), C)
    dl = {'train': DataLoader(train, batch_size=1, shuffle=True, generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(val, batch_size=1)}
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        m, vh, th = ga.train_gridwise(m, dl, nn.CrossEntropyLoss(), opt, num_epochs=1)
    return th, vh, {k: v.clone() for k, v in m.state_dict().items()}


def _spot_tensors(ds):
    items = ds.__getitems__(range(len(ds)))
    return TensorDataset(torch.stack([x for x, _ in items]), torch.stack([y for _, y in items]).to(DEV))


def _grid_tensors(ds):
    return TensorDataset(torch.stack([ds[k][0] for k in range(len(ds))]), torch.stack([ds[k][1] for k in range(len(ds))]).to(DEV))


def test_training_loops_on_use_pcs_items_equal_the_loops_on_the_same_tensors(monkeypatch):
    import gridnext_amd as ga
    monkeypatch.setenv('GNX_GRAPH', '0')
    dev, _, _ = _recipe()
    pca = dev.subset_arrays(['arr0']).fit_pca()
    classes = ga.SparseCountDataset(dev).classes
    assert len(classes) == C
    train = ga.SparseCountDataset(dev.subset_arrays(['arr0']), classes=classes, use_pcs=K, pca=pca)
    val = ga.SparseCountDataset(dev.subset_arrays(['arr1']), classes=classes, use_pcs=K, pca=pca)
    th0, vh0, sd0 = _spot_loop(_spot_tensors(train), _spot_tensors(val))
    th1, vh1, sd1 = _spot_loop(train, val)
    print("spot loop: tensors", th0, vh0, "use_pcs items", th1, vh1)
    assert len(th0) == 2 and np.isfinite(th0 + vh0).all() and th0 == th1 and vh0 == vh1
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    gtrain = ga.SparseCountGridDataset(dev.subset_arrays(['arr0']), classes=classes, use_pcs=K, pca=pca)
    gval = ga.SparseCountGridDataset(dev.subset_arrays(['arr1']), classes=classes, use_pcs=K, pca=pca)
    th0, vh0, sd0 = _grid_loop(_grid_tensors(gtrain), _grid_tensors(gval))
    th1, vh1, sd1 = _grid_loop(gtrain, gval)
    print("grid loop: tensors", th0, vh0, "use_pcs items", th1, vh1)
    assert len(th0) == 1 and np.isfinite(th0 + vh0).all() and th0 == th1 and vh0 == vh1
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)


def test_fit_holds_no_dense_operand():
    """Two arrays of 4 096 spots x 256 genes at 10 %: the Gram matrix is 256 x 256 x 8 = 512 KB, one array's dense float32
    operand 4 096 x 256 x 4 = 4 MB.  The fit may allocate the Gram matrix, the (G, 2) moments and little else: below 2 MB over
    the base, four times the Gram matrix and half of one array's dense operand."""
    import pandas as pd
    import scipy.sparse as sp
    import gridnext_amd as ga
    N, G = 4096, 256
    X = sp.random(2 * N, G, density=0.10, random_state=7, format='csr', dtype=np.float64)
    X.data = np.random.default_rng(7).integers(1, 50, X.nnz).astype(np.float64)
    obs = pd.DataFrame({'x': np.arange(2 * N) % 64, 'y': (np.arange(2 * N) // 64) % 64, 'array': np.repeat(['a', 'b'], N),
                        'annotation': 'c0'}, index=['s%d' % k for k in range(2 * N)])
    counts = ga.SpotCounts(X, obs, ['g%d' % g for g in range(G)]).to(DEV)
    counts.normalize_total(1e4).log1p()
    first = counts.fit_pca()                                                             # maps and first-call buffers exist now
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    again = counts.fit_pca()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("fit_pca of 2 x %d spots x %d genes: peak %.3f MB over the base; the Gram matrix %.3f MB, one array's dense float32 "
          "operand %.3f MB" % (N, G, peak / 1e6, G * G * 8 / 1e6, N * G * 4 / 1e6))
    assert G * G * 8 <= peak < 2 * 1024 * 1024 <= N * G * 4 // 2
    assert again.components_.shape == (G, G) and torch.equal(first.components_.view(torch.int64), again.components_.view(torch.int64))


def test_a_second_fit_gives_equal_bits():
    dev, _, _ = _recipe()
    first, _ = _fits()
    again = dev.fit_pca()
    for name in ('components_', 'explained_variance_', 'explained_variance_ratio_', 'mean_', 'scale_'):
        assert torch.equal(getattr(first, name).view(torch.int64), getattr(again, name).view(torch.int64)), name
