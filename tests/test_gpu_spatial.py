"""`SpotCounts.spatial_autocorr` with the counts resident on a HIP device, on the fixture of tests/spatial_ref.py: resident against
host against restatement - sums and statistics within the bars, equal top-16 masks (all planted), equal pval_sim - the launches
per call, gene and array views, n_rings=2, the cap's refusal and the memory condition."""
import math

import numpy as np
import pytest
import torch

import sparse_counts_ref as CR
import spatial_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_made = {}


def _pair():
    """(resident, host): the fixture normalised + log1p on the host, then uploaded - the same stored bits on both sides."""
    if 'p' not in _made:
        import gridnext_amd as ga
        f = R.fixture()
        host = ga.SpotCounts(f['X'], f['obs'], f['genes']).normalize_total(CR.TARGET).log1p()
        assert np.array_equal(np.asarray(host.host_csr().todense()), f['dense'])
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


def test_sums_within_their_bars():
    from gridnext_amd import spatial as S
    dev, ref = _pair()[0], R.reference()
    worst = 0.0
    for (_, _, trio, _), table, want in zip(dev.bound_csc(), dev.spot_neighbors(), ref['per']):
        assert table.is_cuda and table.dtype == torch.int32
        pdq = S.line_spatial(trio, dev.gene_lines(), dev.n_genes, table.shape[0], table[None], dev.device)[0]
        for c, name in enumerate(('P', 'D', 'Q')):
            err = np.abs(pdq[:, c] - want[name])
            assert (err <= want[name + '_bar']).all(), name
            worst = max(worst, float((err / want[name + '_bar']).max()))
    print("resident sums P, D, Q: largest |err| / bar %.3g" % worst)


def test_resident_against_host_against_restatement(monkeypatch):
    dev, host = _pair()
    ref, planted = R.reference(), R.fixture()['planted']
    R.check_fixture()
    got, seen = _recorded(monkeypatch, lambda: dev.spatial_autocorr())
    assert seen.count('gnx_sparse_line_moments_f64') == 2 and seen.count('gnx_sparse_line_spatial_f64') == 2 and len(seen) == 4
    R.check_result(got, ref, "resident")
    on_host = host.spatial_autocorr()
    assert np.array_equal(got.top(16), planted) and np.array_equal(on_host.top(16), planted)
    assert np.array_equal(got.top(16), R.top_mask(ref['I'], 16, True))
    assert np.array_equal(got.top(16, by='C'), on_host.top(16, by='C')) and np.array_equal(got.top(16, by='C'), R.top_mask(ref['C'], 16, False))
    assert np.array_equal(np.argsort(-got.I, kind='stable'), np.argsort(-on_host.I, kind='stable'))          # equal ranks
    assert np.array_equal(np.argsort(-got.I, kind='stable'), np.argsort(-ref['I'], kind='stable'))
    again = dev.spatial_autocorr()
    assert np.array_equal(got.I.view(np.int64), again.I.view(np.int64)) and np.array_equal(got.C.view(np.int64), again.C.view(np.int64))
    picked = dev.subset_genes(got.top(16))
    assert picked.n_genes == 16 and list(picked.gene_ids) == list(host.gene_ids[planted])


def test_permutations_resident_against_host_against_restatement(monkeypatch):
    from gridnext_amd import spatial as S
    dev, host = _pair()
    ref = R.reference()
    got, seen = _recorded(monkeypatch, lambda: dev.spatial_autocorr(n_perms=R.N_PERMS, seed=R.SEED))
    per_array = [math.ceil((R.N_PERMS + 1) * t.numel() * 4 / (64 << 20)) for t in dev.spot_neighbors()]
    assert per_array == [1, 1] and seen.count('gnx_sparse_line_spatial_f64') == sum(per_array)
    assert seen.count('gnx_sparse_line_moments_f64') == 2 and 'gnx_sparse_expand_f32' not in seen and len(seen) == 4
    R.check_result(got, ref, "resident, 49 permutations", R.simulations())
    on_host = host.spatial_autocorr(n_perms=R.N_PERMS, seed=R.SEED)
    assert np.array_equal(got.pval_sim_I, on_host.pval_sim_I) and np.array_equal(got.pval_sim_C, on_host.pval_sim_C)
    assert list(got.to_frame().columns) == S.COLUMNS + S.SIM_COLUMNS
    # tables in chunks: the same bits from launches of at most 4 tables
    monkeypatch.setattr(S, 'TABLE_CHUNK_BYTES', 4 * max(t.numel() for t in dev.spot_neighbors()) * 4)
    chunked, seen = _recorded(monkeypatch, lambda: dev.spatial_autocorr(n_perms=R.N_PERMS, seed=R.SEED))
    assert seen.count('gnx_sparse_line_spatial_f64') == 13 + 13                       # ceil(50 / 4) per array
    assert np.array_equal(chunked.sim_I.view(np.int64), got.sim_I.view(np.int64))
    assert np.array_equal(chunked.sim_C.view(np.int64), got.sim_C.view(np.int64)) and np.array_equal(chunked.I.view(np.int64), got.I.view(np.int64))


def test_gene_and_array_views():
    dev, host = _pair()
    genes = [int(g) for g in np.random.default_rng(4).permutation(96)[:40]]
    picks = [host.gene_ids[g] for g in genes]
    d, h = dev.subset_genes(picks).subset_arrays(['arr1']), host.subset_genes(picks).subset_arrays(['arr1'])
    ref = R.reference(arrays=(1,), genes=genes)                                      # the fixture restricted to that array
    got = d.spatial_autocorr(n_perms=9, seed=1)
    R.check_result(got, ref, "resident view: 40 genes of arr1")
    assert list(got.gene_ids) == picks and got.n_spots == ref['N']
    want = h.spatial_autocorr(n_perms=9, seed=1)
    assert np.array_equal(got.pval_sim_I, want.pval_sim_I) and np.array_equal(got.top(5), want.top(5))
    assert (np.abs(got.sim_I - want.sim_I) <= 2 * ref['sim_I_bar'][None, :]).all()
    both = dev.subset_arrays(['arr1', 'arr0']).spatial_autocorr()                    # view order is the order of the sums alone
    whole = R.reference()
    assert (np.abs(both.I - whole['I']) <= whole['I_bar']).all() and (np.abs(both.C - whole['C']) <= whole['C_bar']).all()


def test_two_rings():
    dev, host = _pair()
    ref = R.reference(n_rings=2)
    got = dev.spatial_autocorr(n_rings=2)
    R.check_result(got, ref, "resident, n_rings=2")
    assert dev.spot_neighbors(2)[0].shape[1] == 18 and got.total_weight > 2 * R.reference()['W']
    assert np.array_equal(got.top(16), host.spatial_autocorr(n_rings=2).top(16))


def test_an_array_above_the_cap_is_refused_before_any_launch(monkeypatch):
    import pandas as pd
    import scipy.sparse as sp
    import gridnext_amd as ga
    n = 32769
    rows, cols = np.divmod(np.arange(n), 256)
    obs = pd.DataFrame({'x': 2 * cols + rows % 2, 'y': rows, 'array': 'big', 'annotation': 'c0'}, index=['s%d' % k for k in range(n)])
    X = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) % 3)), shape=(n, 3))
    counts = ga.SpotCounts(X, obs, ['g0', 'g1', 'g2'])
    with pytest.raises(ValueError, match="big has 32769 spots.*device=None"):
        _recorded(monkeypatch, lambda: counts.to(DEV).spatial_autocorr())
    assert np.isfinite(counts.spatial_autocorr().I).all()                             # the host path has no cap


def test_a_call_holds_no_dense_operand():
    """Two arrays of 4 096 spots x 256 genes: one array's dense float32 operand is 4 096 x 256 x 4 = 4 MB.  A call allocates the
    per-gene sums (2 + 3 doubles per gene) and, with permutations, a chunk of tables (4 096 x 6 x 4 = 98 KB each): below half of
    the dense operand, the HVG test's bar."""
    import pandas as pd
    import scipy.sparse as sp
    import gridnext_amd as ga
    N, G = 4096, 256
    X = sp.random(2 * N, G, density=0.10, random_state=7, format='csr', dtype=np.float64)
    X.data = np.random.default_rng(7).integers(1, 50, X.nnz).astype(np.float64)
    rows, cols = np.divmod(np.arange(2 * N) % N, 64)
    obs = pd.DataFrame({'x': 2 * cols + rows % 2, 'y': rows, 'array': np.repeat(['a', 'b'], N), 'annotation': 'c0'},
                       index=['s%d' % k for k in range(2 * N)])
    counts = ga.SpotCounts(X, obs, ['g%d' % g for g in range(G)]).to(DEV)
    first = counts.spatial_autocorr(n_perms=4)                                        # the resident tables exist now
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    again = counts.spatial_autocorr(n_perms=4)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("spatial_autocorr(n_perms=4) of 2 x %d spots x %d genes: peak %.4f MB over the base; one array's dense float32 operand "
          "%.3f MB" % (N, G, peak / 1e6, N * G * 4 / 1e6))
    assert 0 < peak < N * G * 4 // 2
    assert np.array_equal(first.sim_I.view(np.int64), again.sim_I.view(np.int64)) and np.isfinite(again.I).all()
