"""Resident sparse counts on a HIP device against their own host path (tests/test_sparse_counts_ref_host.py pins that to scipy,
numpy and the dense count datasets): the tutorial's recipe (normalise, log1p, moments, the 64 genes with the largest
|mean / std|), the items of `SparseCountDataset` / `SparseCountGridDataset`, the training loops fed by them against the same
loops fed the same tensors, and the number of expand launches.  Fixture: 3 synthetic arrays of about 200 spots x 300 genes
(tests/sparse_counts_ref.py), two for training and one for validation."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

import sparse_counts_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = 64
_made = {}


def _fixture():
    """(host SpotCounts of raw counts, dense raw counts, obs, genes); built once, never modified (users take `_fresh`)."""
    if 'raw' not in _made:
        X, obs, genes = R.synthetic_arrays()
        _made['raw'] = (X, X.toarray(), obs, genes)
    return _made['raw']


def _fresh():
    import gridnext_amd as ga
    X, _, obs, genes = _fixture()
    return ga.SpotCounts(X, obs, genes)


def _recipe():
    """(device counts after normalize_total + log1p, the same values on the host path, the selected view of each); once."""
    if 'recipe' not in _made:
        dev = _fresh().to(DEV)
        dev.normalize_total(1e4).log1p()
        mean, std = dev.gene_moments()
        with np.errstate(divide='ignore', invalid='ignore'):
            score = np.abs(mean.numpy() / std.numpy())
        top = R.top_genes(np.where(np.isfinite(score), score, -np.inf), K)
        host = dev.to('cpu')                                   # the device's values, copied: isolates the expand step
        ids = [dev.gene_ids[g] for g in top]
        _made['recipe'] = (dev, host, dev.subset_genes(ids), host.subset_genes(ids), top)
    return _made['recipe']


def test_the_tutorials_recipe_on_the_device_against_the_host():
    import scipy.sparse as sp
    from gridnext_amd import visium_datasets as V
    _, dense, obs, genes = _fixture()
    host = _fresh()
    dev = _fresh().to(DEV)
    assert dev.device == torch.device(DEV) and host.device is None and dev._s.csr[2].is_cuda
    assert np.array_equal(dev.spot_totals().numpy(), dense.sum(1))                          # integer counts: exact
    assert torch.equal(dev.detection_rate(), host.detection_rate())
    host.normalize_total(1e4)
    dev.normalize_total(1e4)
    assert torch.equal(dev._s.csr[2].cpu(), host._s.csr[2])                                 # the division: numpy's bits
    assert all(torch.equal(d[2].cpu(), h[2]) for d, h in zip(dev._s.csc, host._s.csc))
    x = host._s.csr[2].numpy().copy()
    host.log1p()
    dev.log1p()
    bar, own = R.log1p_bar(x)
    exact = np.log1p(x.astype(np.float64))
    mine = float(R.ulps_of(dev._s.csr[2].cpu().numpy(), exact).max())
    apart = float(R.ulps_of(dev._s.csr[2].cpu().numpy(), host._s.csr[2].numpy().astype(np.float64)).max())
    print("log1p over %d stored values: device %.3f ulp, numpy %.3f ulp, bar %.3f ulp; device against host %.3f ulp"
          % (len(x), mine, own, bar, apart))
    assert mine <= bar and apart <= bar + own
    for a in range(3):                                          # CSR and CSC: the same bits, the function being elementwise
        p, i, v = (t.cpu().numpy() for t in dev._s.csc[a])
        r0, r1 = dev._s.row_start[a], dev._s.row_start[a + 1]
        rows = sp.csr_matrix((dev._s.csr[2].cpu().numpy(), dev._s.csr[1].cpu().numpy(), dev._s.csr[0].cpu().numpy()),
                             shape=dense.shape)[r0:r1]
        assert np.array_equal(sp.csc_matrix((v, i, p), shape=(r1 - r0, 300)).toarray(), rows.toarray())
    # moments: every array's partial sums within the derived bound of fsum over the device's own values ...
    s1, s2, N = np.zeros(300), np.zeros(300), 0
    worst = 0.0
    for a in range(3):
        got = V.line_moments(dev._s.csc[a], None, 300, None, dev.device).numpy()
        p, i, v = (t.cpu().numpy() for t in dev._s.csc[a])
        for g, (f1, f2, cnt, fabs) in enumerate(R.moments_fsum(p, i, v, None, 300)):
            e1, e2 = abs(got[g, 0] - f1), abs(got[g, 1] - f2)
            assert e1 <= R.moments_bound(cnt, fabs) and e2 <= R.moments_bound(cnt, f2), (a, g, cnt, e1, e2)
            worst = max(worst, e1 / max(R.moments_bound(cnt, fabs), 1e-300), e2 / max(R.moments_bound(cnt, f2), 1e-300))
        s1, s2, N = s1 + got[:, 0], s2 + got[:, 1], N + int(dev._s.row_start[a + 1] - dev._s.row_start[a])
    print("gene moments: largest error / bound %.3g" % worst)
    mean, std = dev.gene_moments()                              # ... and (mean, std) the stated formula of those sums, exactly
    assert np.array_equal(mean.numpy(), s1 / N)
    assert np.array_equal(std.numpy(), np.sqrt(np.maximum(s2 / N - (s1 / N) ** 2, 0.0)))
    # the SAME selection as the float64 reference of the host path's values; the fixture keeps the 64th and 65th apart
    ref_y, _ = R.normalise_log1p_dense(dense)
    rmean, rstd, rscore = R.tutorial_scores(ref_y)
    order = R.top_genes(rscore, 65)
    gap = (rscore[order[63]] - rscore[order[64]]) / rscore[order[63]]
    print("score 64 %.12g, score 65 %.12g, relative gap %.3g" % (rscore[order[63]], rscore[order[64]], gap))
    assert gap >= 1e-9
    hmean, hstd = host.gene_moments()
    for m, s in ((mean, std), (hmean, hstd)):
        with np.errstate(divide='ignore', invalid='ignore'):
            score = np.abs(m.numpy() / s.numpy())
        assert set(R.top_genes(np.where(np.isfinite(score), score, -np.inf), K)) == set(order[:K])
    assert np.allclose(mean.numpy(), rmean, rtol=1e-6) and np.allclose(std.numpy(), rstd, rtol=1e-6)


def test_items_of_both_datasets_equal_the_host_path():
    import gridnext_amd as ga
    dev, host, dev_sel, host_sel, top = _recipe()
    two = ['arr2', 'arr0']
    for d, h in ((dev, host), (dev_sel, host_sel), (dev_sel.subset_arrays(two), host_sel.subset_arrays(two))):
        gd, gh = ga.SparseCountGridDataset(d), ga.SparseCountGridDataset(h)
        assert len(gd) == len(gh) == len(d.arrays) and list(gd.classes) == list(gh.classes)
        for k in range(len(gd)):
            (xd, yd), (xh, yh) = gd[k], gh[k]
            assert xd.is_cuda and yd.is_cuda and xd.shape == (d.n_genes, 78, 64) and xd.is_contiguous()
            assert torch.equal(xd.cpu(), xh) and torch.equal(yd.cpu(), yh) and int((yh > 0).sum()) > 150
        sd, sh = ga.SparseCountDataset(d), ga.SparseCountDataset(h)
        assert len(sd) == len(sh) == d.n_spots
        picks = [len(sd) - 1, 0, 7, 7, 250, 3]
        bd, bh = sd.__getitems__(picks), sh.__getitems__(picks)
        assert all(torch.equal(a[0].cpu(), b[0]) and torch.equal(a[1], b[1]) for a, b in zip(bd, bh))
        assert bd[0][0].is_cuda and bd[0][0].shape == (d.n_genes,) and bd[1][0].data_ptr() - bd[0][0].data_ptr() == 4 * d.n_genes
        xb, yb = next(iter(DataLoader(sd, batch_size=33)))
        xh, yh = next(iter(DataLoader(sh, batch_size=33)))
        assert xb.is_cuda and torch.equal(xb.cpu(), xh) and torch.equal(yb.cpu(), yh)
    assert torch.equal(ga.SparseCountDataset(dev_sel)[5][0].cpu(), ga.SparseCountDataset(dev)[5][0].cpu()[torch.from_numpy(top)])


def test_one_expand_launch_per_item_or_batch(monkeypatch):
    import gridnext_amd as ga
    from gridnext_amd import _lib
    _, _, dev_sel, _, _ = _recipe()
    grid, spots = ga.SparseCountGridDataset(dev_sel), ga.SparseCountDataset(dev_sel)
    grid[0], spots[0]                                           # maps and labels exist now
    seen, real = [], _lib.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    grid[0], grid[2]
    assert seen == ['gnx_sparse_expand_f32'] * 2
    del seen[:]
    n = sum(1 for _ in DataLoader(spots, batch_size=100))
    assert n == -(-len(spots) // 100) and seen == ['gnx_sparse_expand_f32'] * n


def test_a_device_dataset_refuses_a_dataloader_worker():
    import gridnext_amd as ga
    _, host, dev_sel, host_sel, _ = _recipe()
    real = torch.utils.data.get_worker_info
    torch.utils.data.get_worker_info = lambda: object()
    try:
        for ds in (ga.SparseCountGridDataset(dev_sel), ga.SparseCountDataset(dev_sel)):
            with pytest.raises(RuntimeError, match="num_workers=0"):
                ds[0]
        assert ga.SparseCountGridDataset(host_sel)[0][0].shape == (K, 78, 64)             # the host path may
    finally:
        torch.utils.data.get_worker_info = real


# ------------------------------------------------------------------------------------------------ the loops
C = 4


def _spot_runs(datasets):
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    runs = []
    for train, val in datasets:
        torch.manual_seed(4)
        f = count_mlp(K, C)
        dl = {'train': DataLoader(train, batch_size=64, shuffle=True, generator=torch.Generator().manual_seed(2)),
              'val': DataLoader(val, batch_size=64)}
        opt = torch.optim.Adam(f.parameters(), lr=1e-3)
        with contextlib.redirect_stdout(io.StringIO()):
            f, vh, th = ga.train_spotwise(f, dl, nn.CrossEntropyLoss(), opt, num_epochs=2)
        runs.append((th, vh, {k: v.clone() for k, v in f.state_dict().items()}))
    return runs


def _tensors(ds):
    return TensorDataset(torch.stack([ds[k][0] for k in range(len(ds))]), torch.stack([ds[k][1] for k in range(len(ds))]).to(DEV))


def test_train_spotwise_from_resident_counts_equals_the_same_batches_from_tensors():
    import gridnext_amd as ga
    _, _, dev_sel, _, _ = _recipe()
    classes = ga.SparseCountDataset(dev_sel).classes
    train = ga.SparseCountDataset(dev_sel.subset_arrays(['arr0', 'arr1']), classes=classes)
    val = ga.SparseCountDataset(dev_sel.subset_arrays(['arr2']), classes=classes)
    assert len(classes) == C and len(train) + len(val) == dev_sel.n_spots
    runs = _spot_runs([(_tensors(train), _tensors(val)), (train, val)])
    print("tensors", runs[0][:2], "counts", runs[1][:2])
    assert len(runs[0][0]) == 2 and all(np.isfinite(v) for v in runs[0][0] + runs[0][1])
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def _grid_loop(train, val, epochs, cached):
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    torch.manual_seed(3)
    f = count_mlp(K, C)
    for p in f.parameters():
        p.requires_grad = False
    m = ga.GridNetHexOddr(f, (K,), (78, 64), C)
    if cached:
        m.enable_f_cache()
    dl = {'train': DataLoader(train, batch_size=1, shuffle=True, generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(val, batch_size=1)}
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        m, vh, th = ga.train_gridwise(m, dl, nn.CrossEntropyLoss(), opt, num_epochs=epochs)
    counts = (m.f_cache.hits, m.f_cache.misses) if cached else None
    return th, vh, {k: v.clone() for k, v in m.state_dict().items()}, counts


def test_train_gridwise_from_resident_counts_equals_the_loop_fed_the_same_tensors(monkeypatch):
    """One epoch fed by SparseCountGridDataset (two arrays to train on, the third to validate) == the loop fed the same grids
    and labels from a TensorDataset: histories and weights.  Three epochs with enable_f_cache() over one set of two arrays in
    both phases, as the slide test: 2 misses - the two arrays' first look-ups, in the first train phase - and the uncached
    results.  The hits depend on how the loop steps.  A count-only f under g is launch-bound, so the loop captures the step per
    phase after `graphs.WARMUP` = 2 eager batches and replays it (a capture bypasses the cache: f runs inside the graph); the
    look-ups are the eager batches alone: 2 in the train phase (the misses), 2 in the val phase (hits).  With GNX_GRAPH=0
    every step is eager: 2 arrays x 2 phases x 3 epochs = 12 look-ups, 2 misses, 10 hits, as with slides."""
    import gridnext_amd as ga
    from gridnext_amd import graphs
    _, _, dev_sel, _, _ = _recipe()
    classes = ga.SparseCountGridDataset(dev_sel).classes
    train = ga.SparseCountGridDataset(dev_sel.subset_arrays(['arr0', 'arr1']), classes=classes)
    val = ga.SparseCountGridDataset(dev_sel.subset_arrays(['arr2']), classes=classes)
    th0, vh0, sd0, _ = _grid_loop(_tensors(train), _tensors(val), 1, False)
    th1, vh1, sd1, _ = _grid_loop(train, val, 1, False)
    print("tensors", th0, vh0, "counts", th1, vh1)
    assert len(th0) == 1 and np.isfinite(th0[0]) and th0 == th1 and vh0 == vh1
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    th2, vh2, sd2, _ = _grid_loop(train, train, 3, False)
    th3, vh3, sd3, counts = _grid_loop(train, train, 3, True)
    print("3 epochs: uncached", th2, vh2, "cached", th3, vh3, "(hits, misses)", counts)
    assert th2 == th3 and vh2 == vh3 and all(torch.equal(sd2[k], sd3[k]) for k in sd2)
    assert graphs.WARMUP == 2 and counts == (2, 2)
    monkeypatch.setenv('GNX_GRAPH', '0')
    th4, vh4, sd4, counts = _grid_loop(train, train, 3, True)
    print("3 epochs, every step eager: cached", th4, vh4, "(hits, misses)", counts)
    assert counts == (10, 2) and len(th4) == 3
