"""`SpotCounts.highly_variable_genes` with the counts resident on a HIP device, on the fixture of tests/hvg_ref.py: resident
against host against restatement - equal masks, ranks and batch counts, variances_norm within the bars propagated from the two
kernels - the launches per batch, the selected view as a dataset, the raw-flag refusal and the memory condition."""
import numpy as np
import pytest
import torch

import hvg_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_TOP = R.N_TOP
_made = {}


def _pair():
    if 'p' not in _made:
        import gridnext_amd as ga
        X, obs, genes, _ = R.fixture()
        host = ga.SpotCounts(X, obs, genes)
        _made['p'] = (host.to(DEV), host)
    return _made['p']


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


@pytest.mark.parametrize("batch", [None, 'array'])
def test_resident_against_host_against_restatement(monkeypatch, batch):
    dev, host = _pair()
    got, seen = _recorded(monkeypatch, lambda: dev.highly_variable_genes(n_top_genes=N_TOP, span=0.3, batch=batch))
    batches = 1 if batch is None else 2
    assert seen.count('gnx_loess_fit_f64') == batches                                # exactly one loess launch per batch
    assert seen.count('gnx_sparse_line_clip_moments_f64') == 2                        # one per array of every batch
    assert seen.count('gnx_sparse_line_moments_f64') == 2 and 'gnx_sparse_expand_f32' not in seen
    assert len(seen) == batches + 4
    R.check_against_reference(got, batch, "resident counts")
    on_host = host.highly_variable_genes(n_top_genes=N_TOP, span=0.3, batch=batch)
    assert np.array_equal(got.highly_variable, on_host.highly_variable)
    assert np.array_equal(got.highly_variable_rank, on_host.highly_variable_rank, equal_nan=True)
    assert np.array_equal(got.highly_variable_nbatches, on_host.highly_variable_nbatches)
    assert np.array_equal(got.means, on_host.means) and np.array_equal(got.variances, on_host.variances)   # integer sums: exact
    again = dev.highly_variable_genes(n_top_genes=N_TOP, span=0.3, batch=batch)
    assert np.array_equal(got.variances_norm.view(np.int64), again.variances_norm.view(np.int64))           # equal bits


def test_views_and_the_selected_view_as_a_dataset():
    import gridnext_amd as ga
    dev, host = _pair()
    picks = [host.gene_ids[g] for g in np.random.default_rng(3).permutation(300)[:120]]
    d, h = dev.subset_genes(picks).subset_arrays(['arr1']), host.subset_genes(picks).subset_arrays(['arr1'])
    got, want = d.highly_variable_genes(n_top_genes=20), h.highly_variable_genes(n_top_genes=20)
    assert np.array_equal(got.highly_variable, want.highly_variable) and got.highly_variable.sum() == 20
    assert np.array_equal(got.highly_variable_rank, want.highly_variable_rank, equal_nan=True)
    assert np.allclose(got.variances_norm, want.variances_norm, rtol=1e-9, atol=0)
    hvg = dev.highly_variable_genes(n_top_genes=N_TOP)
    chosen = dev.subset_genes(hvg.highly_variable)
    assert chosen.n_genes == N_TOP and list(chosen.gene_ids) == list(host.gene_ids[hvg.highly_variable])
    items = ga.SparseCountDataset(chosen).__getitems__([0, 200, 400])
    dense = R.fixture()[3]
    for (x, _), row in zip(items, (0, 200, 400)):
        assert x.is_cuda and x.shape == (N_TOP,) and np.array_equal(x.cpu().numpy(), dense[row][hvg.highly_variable].astype(np.float32))


def test_the_raw_flag_on_a_device():
    import gridnext_amd as ga
    X, obs, genes, _ = R.fixture()
    dev = ga.SpotCounts(X, obs, genes).to(DEV)
    assert dev._s.raw
    dev.subset_arrays(['arr0']).normalize_total(1e4)
    with pytest.raises(ValueError, match="rewritten by normalize_total"):
        dev.highly_variable_genes(n_top_genes=10)
    dev.log1p()
    with pytest.raises(ValueError, match="rewritten by log1p"):
        dev.to('cpu').highly_variable_genes(n_top_genes=10)                           # to() carries the flag
    host = ga.SpotCounts(X, obs, genes).normalize_total(1e4)
    with pytest.raises(ValueError, match="rewritten by normalize_total"):
        host.to(DEV).highly_variable_genes(n_top_genes=10)


def test_selection_holds_no_dense_operand():
    """Two arrays of 4 096 spots x 256 genes at 10 %: one array's dense float32 operand is 4 096 x 256 x 4 = 4 MB.  The selection
    allocates per-gene vectors alone - moments, bounds, the loess's six inputs and its output, a few KB each: below half of the
    dense operand, the bar, by orders."""
    import pandas as pd
    import scipy.sparse as sp
    import gridnext_amd as ga
    N, G = 4096, 256
    X = sp.random(2 * N, G, density=0.10, random_state=7, format='csr', dtype=np.float64)
    X.data = np.random.default_rng(7).integers(1, 50, X.nnz).astype(np.float64)
    obs = pd.DataFrame({'x': np.arange(2 * N) % 64, 'y': (np.arange(2 * N) // 64) % 64, 'array': np.repeat(['a', 'b'], N),
                        'annotation': 'c0'}, index=['s%d' % k for k in range(2 * N)])
    counts = ga.SpotCounts(X, obs, ['g%d' % g for g in range(G)]).to(DEV)
    first = counts.highly_variable_genes(n_top_genes=64, batch='array')                  # first-call buffers exist now
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    again = counts.highly_variable_genes(n_top_genes=64, batch='array')
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("highly_variable_genes of 2 x %d spots x %d genes: peak %.4f MB over the base; one array's dense float32 operand "
          "%.3f MB" % (N, G, peak / 1e6, N * G * 4 / 1e6))
    assert 0 < peak < N * G * 4 // 2
    assert again.highly_variable.sum() == 64 and np.array_equal(first.variances_norm.view(np.int64), again.variances_norm.view(np.int64))
