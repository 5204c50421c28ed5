"""The view vocabulary of `SpotCounts` - `array_span`, `view_rows`, `host_csr`, `_array_ids`, `bound_csc` - on a view with a gene
selection and a reordered array subset, and on the empty view, against the hand-written forms they replaced."""
import numpy as np
import torch

import sparse_counts_ref as R


def _views():
    import gridnext_amd as ga
    X, obs, genes = R.synthetic_arrays(seed=3, n_arrays=3, n_spots=40)
    c = ga.SpotCounts(X, obs, genes)
    c.normalize_total(1e4).log1p()
    pick = [genes[g] for g in np.random.default_rng(3).permutation(300)[:50]]
    return c, c.subset_genes(pick).subset_arrays(['arr2', 'arr0']), c.subset_genes(pick).subset_arrays([])


def _by_hand(v):
    """The three spellings as they stood in count_pca.gram, sparse_linear._host_rows and SparseCountDataset."""
    import scipy.sparse as sp
    s = v._s
    spans = [(int(s.row_start[a]), int(s.row_start[a + 1])) for a in v._arrays]
    rows = np.concatenate([np.arange(s.row_start[a], s.row_start[a + 1]) for a in v._arrays] or [np.zeros(0, np.int64)])
    ptr, idx, val = (t.numpy() for t in s.csr)
    X = sp.csr_matrix((val, idx, ptr), shape=(len(ptr) - 1, len(s.gene_ids)), copy=False)
    return spans, rows, lambda lines, dtype: (X[lines] if v._genes is None else X[lines][:, v._genes]).astype(dtype)


def _same(A, B):
    A, B = A.tocsr(), B.tocsr()
    return A.dtype == B.dtype and A.shape == B.shape and all(np.array_equal(getattr(A, k), getattr(B, k))
                                                             for k in ('indptr', 'indices', 'data'))


def test_vocabulary_equals_the_hand_written_forms():
    full, view, empty = _views()
    for v in (full, view, empty):
        spans, rows, host = _by_hand(v)
        assert [v.array_span(a) for a in v._arrays] == spans
        assert all(type(x) is int for span in map(v.array_span, v._arrays) for x in span)
        got = v.view_rows()
        assert got.dtype == np.int64 and got.shape == rows.shape and np.array_equal(got, rows) and v.n_spots == len(rows)
        for dtype in (np.float32, np.float64):
            assert _same(v.host_csr(rows, dtype), host(rows, dtype))
        some = rows[::3][::-1].copy()
        assert _same(v.host_csr(some), host(some, np.float32))
        assert _same(v.host_csr(), host(np.arange(full.n_spots), np.float32))
        assert v._array_ids() == v._arrays and v._array_ids(['arr1', 'arr0']) == [1, 0]
        walk = list(v.bound_csc())
        assert [(k, a, r0) for k, a, _, r0 in walk] == [(k, a, spans[k][0]) for k, a in enumerate(v._arrays)]
        assert all(trio is v._s.csc[a] for _, a, trio, _ in walk)
        assert [a for _, a, _, _ in v.bound_csc(['arr1'])] == [1]
    assert view._arrays == [2, 0] and len(view.view_rows()) and view.view_rows()[0] == view.array_span(2)[0]
    assert empty.view_rows().shape == (0,) and list(empty.bound_csc()) == [] and empty.host_csr(empty.view_rows()).shape == (0, 50)


def test_host_csr_sees_a_later_transform_and_same_device():
    import gridnext_amd as ga
    from gridnext_amd.visium_datasets import same_device
    X, obs, genes = R.synthetic_arrays(seed=4, n_arrays=2, n_spots=30)
    c = ga.SpotCounts(X, obs, genes)
    before = c.host_csr(c.view_rows()).toarray()
    c.log1p()
    assert np.array_equal(c.host_csr(c.view_rows()).toarray(), np.log1p(before))
    assert same_device(None, 'cpu') and same_device(torch.device('cpu'), None) and same_device('cuda', 'cuda:0')
    assert not same_device(None, 'cuda:0') and not same_device('cuda:1', 'cuda') and not same_device('meta', 'cpu')
    assert c.to(None) is c and c.to('cpu') is c
