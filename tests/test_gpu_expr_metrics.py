"""`ExpressionMetrics` on resident counts: the fixture of tests/test_expr_metrics_host.py on the device against the fsum
restatement, np.corrcoef and the dense mean (the host test's bound and tolerances, unchanged), the launches an update makes,
a gene subset and an array subset, the refusals before any launch, and `evaluate_expression` over a `SlideCountDataset` with
the tiny DenseNet of tests/test_gpu_expression.py.  `SparseMSELoss` on resident counts still raises."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import expr_metrics_ref as E
from test_expr_metrics_host import _fixture

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DENSE, SPARSE = 'gnx_act_col_moments_f64', 'gnx_sparse_pred_moments_f64'


@pytest.fixture
def launches(monkeypatch):
    """The names that go through _lib.call, in order."""
    from gridnext_amd import _lib
    seen, real = [], _lib.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    return seen


def test_resident_sums_and_statistics_hold_the_host_tests_bounds(launches):
    import gridnext_amd as ga
    counts, scale, z, t, stored, (S, A, N) = _fixture()
    n = 401
    dev = counts.to(DEV)
    m = ga.ExpressionMetrics(dev, gene_scale=scale)
    zd = torch.from_numpy(z).to(DEV)
    order = torch.from_numpy(np.random.default_rng(5).permutation(n))
    del launches[:]
    for k, b in enumerate(range(0, n, 64)):                                          # 7 shuffled batches; rows on the device, then on the CPU
        rows = order[b:b + 64]
        m.update(zd[rows.to(DEV)], rows.to(DEV) if k % 2 else rows)
    assert launches == [DENSE, SPARSE, SPARSE] * 7 and m.n == n                       # both arrays every time: shuffled rows touch both
    assert m.table.is_cuda and m.table.dtype == torch.float64 and m.table.shape == (300, 5)
    got = m.table.cpu().numpy()
    calls = np.array([7, 7, 14, 14, 14])
    print("resident sums: largest |err| / (2^-53 sum|term|) per column", (np.abs(got - S) / (E.U * A)).max(0))
    assert bool((np.abs(got - S) <= E.bound(N, A, calls)).all())
    host = ga.ExpressionMetrics(counts, gene_scale=scale).update(torch.from_numpy(z), torch.arange(n))
    assert bool((np.abs(got - host.table.numpy()) <= E.bound(N, A, calls) + E.bound(N, A, 1)).all())
    out = m.compute()
    p, t64 = E.predictions(z, 1), t.astype(np.float64)
    sp, st = p.std(0), t64.std(0)
    tol = 3 * (n + 16) * E.U * (1 / (sp * st) + 1 / (2 * sp * sp) + 1 / (2 * st * st))
    assert tol.max() < 1e-10
    want = np.array([np.corrcoef(p[:, g], t64[:, g])[0, 1] for g in range(300)])
    mse = ((p - t64) ** 2).mean(0)
    mtol = 2 * (n + 16) * E.U * (S[:, 1] + 2 * S[:, 4] + S[:, 3]) / n
    print("resident pearson: largest |difference| to corrcoef %.3g (tolerance <= %.3g); mse: largest relative difference %.3g"
          % (np.abs(out['pearson'] - want).max(), tol.max(), (np.abs(out['mse'] - mse) / mse).max()))
    assert bool((np.abs(out['pearson'] - want) <= tol).all()) and bool((np.abs(out['mse'] - mse) <= mtol).all())
    assert out['n'] == n and abs(out['loss'] - mse.mean()) <= 1e-12 * mse.mean()
    # a second pass gives equal bits
    first = m.table.clone()
    m.reset()
    for b in range(0, n, 64):
        m.update(zd[order[b:b + 64].to(DEV)], order[b:b + 64])
    assert torch.equal(m.table, first)


def test_cpu_rows_launch_only_the_arrays_the_batch_touches(launches):
    import gridnext_amd as ga
    counts, scale, z, t, stored, _ = _fixture()
    dev = counts.to(DEV)
    r0 = int(counts._s.row_start[1])
    zd = torch.from_numpy(z).to(DEV)
    m = ga.ExpressionMetrics(dev, gene_scale=scale)
    del launches[:]
    m.update(zd[r0 + 3:r0 + 40], torch.arange(r0 + 3, r0 + 40))                      # CPU rows of the second array alone
    assert launches == [DENSE, SPARSE]
    S, A, N = E.sums(z[r0 + 3:r0 + 40, :50], t[r0 + 3:r0 + 40, :50], stored[r0 + 3:r0 + 40, :50], 1)
    assert bool((np.abs(m.table.cpu().numpy()[:50] - S) <= E.bound(N, A, 1)).all())
    both = ga.ExpressionMetrics(dev, gene_scale=scale).update(zd[r0 + 3:r0 + 40], torch.arange(r0 + 3, r0 + 40, device=DEV))
    assert launches == [DENSE, SPARSE, DENSE, SPARSE, SPARSE]                        # rows on the device: every bound array
    assert torch.equal(both.table, m.table)                                          # the untouched array adds +0.0
    del launches[:]
    m.update(zd[r0 - 2:r0 + 2], torch.arange(r0 - 2, r0 + 2).int())                  # int32 rows across the boundary
    assert launches == [DENSE, SPARSE, SPARSE] and m.n == 41


def test_a_gene_subset_and_an_array_subset(launches):
    import gridnext_amd as ga
    counts, scale, z, t, stored, _ = _fixture()
    genes = list(counts.gene_ids)
    pick = [int(g) for g in np.random.default_rng(8).permutation(300)[:37]]
    r0 = int(counts._s.row_start[1])
    view = counts.subset_genes([genes[g] for g in pick]).subset_arrays(['arr1'])
    sub_scale = scale[pick]
    for activation in ('sigmoid', None):
        m = ga.ExpressionMetrics(view.to(DEV), activation=activation, gene_scale=sub_scale)
        zs = np.ascontiguousarray(z[r0:, pick])
        rows = torch.arange(r0, 401)
        del launches[:]
        m.update(torch.from_numpy(zs).to(DEV), rows.to(DEV))
        assert launches == [DENSE, SPARSE]                                           # one bound array
        S, A, N = E.sums(zs, t[r0:, pick], stored[r0:, pick], 1 if activation else 0)
        got = m.table.cpu().numpy()
        assert got.shape == (37, 5) and bool((np.abs(got - S) <= E.bound(N, A, 1)).all())
        host = ga.ExpressionMetrics(view, activation=activation, gene_scale=sub_scale).update(torch.from_numpy(zs), rows)
        assert bool((np.abs(got - host.table.numpy()) <= 2 * E.bound(N, A, 1)).all())
        # a z that is a column slice of a wider tensor: its leading dimension goes to the kernels
        wide = torch.from_numpy(z[r0:]).to(DEV)
        lo = min(min(pick), 295)
        m2 = ga.ExpressionMetrics(counts.subset_genes(genes[lo:lo + 5]).subset_arrays(['arr1']).to(DEV), activation=activation)
        m3 = ga.ExpressionMetrics(counts.subset_genes(genes[lo:lo + 5]).subset_arrays(['arr1']).to(DEV), activation=activation)
        m2.update(wide[:, lo:lo + 5], rows)
        m3.update(wide[:, lo:lo + 5].contiguous(), rows)
        assert torch.equal(m2.table, m3.table)


def test_refusals_come_before_any_launch(launches):
    import gridnext_amd as ga
    counts, scale, z, _, _, _ = _fixture()
    dev = counts.to(DEV)
    r0 = int(counts._s.row_start[1])
    m = ga.ExpressionMetrics(dev.subset_arrays(['arr1']), gene_scale=scale)
    zd = torch.from_numpy(z[:3]).to(DEV)
    del launches[:]
    for where in (DEV, 'cpu'):
        with pytest.raises(ValueError, match="distinct storage rows of the bound arrays"):
            m.update(zd, torch.tensor([r0, r0 + 1, r0], device=where))               # a repeat
        with pytest.raises(ValueError, match="bound arrays"):
            m.update(zd, torch.tensor([r0, r0 + 1, r0 - 1], device=where))           # a row of arr0
        with pytest.raises(ValueError, match="bound arrays"):
            m.update(zd, torch.tensor([r0, r0 + 1, 401], device=where))              # outside the storage
    with pytest.raises(ValueError, match=r"z must be \(B, 300\), one column per selected gene, got \(3, 299\)"):
        m.update(zd[:, :299], torch.tensor([r0, r0 + 1, r0 + 2]))
    with pytest.raises(ValueError, match="z must be float32 with the counts on cuda:0, got torch.float64"):
        m.update(zd.double(), torch.tensor([r0, r0 + 1, r0 + 2]))
    with pytest.raises(ValueError, match="z is on cpu, the counts are on cuda:0"):
        m.update(zd.cpu(), torch.tensor([r0, r0 + 1, r0 + 2]))
    assert launches == [] and m.n == 0 and not m.table.any()
    m.update(zd, torch.tensor([r0, r0 + 1, r0 + 2]))
    assert launches == [DENSE, SPARSE] and m.n == 3
    with pytest.raises(RuntimeError, match="the counts are on cuda:0; the criterion has no device form"):
        ga.SparseMSELoss(dev)


def test_evaluate_expression_over_a_slide_count_dataset_equals_manual_updates():
    import gridnext_amd as ga
    from slide_fixture import SLIDE, SR1, SR2
    from test_gpu_expression import TINY, _slide_counts
    counts, _ = _slide_counts()
    dev = counts.to(DEV)
    ds = ga.SlideCountDataset([SLIDE, SLIDE], [SR1, SR2], dev, patch_size=16, window_size=20, device=DEV, raw_uint8=False)
    loader = DataLoader(ds, batch_size=8)
    torch.manual_seed(7)
    model = ga.ExpressionNet(ga.DenseNet(**TINY), counts.n_genes).to(DEV).train()
    scale = ga.SparseMSELoss.unit_scale(dev)
    m = ga.ExpressionMetrics(dev, gene_scale=scale)
    out = ga.evaluate_expression(model, loader, m)
    assert model.training and out['n'] == len(ds) == counts.n_spots
    model.eval()
    ref = ga.ExpressionMetrics(dev, gene_scale=scale)
    dense = []
    with torch.no_grad():
        for x, rows, _ in loader:
            zb = model(x)
            ref.update(zb, rows)
            dense.append((zb.cpu().numpy(), rows.numpy()))
    assert torch.equal(m.table, ref.table)                                           # bit for bit
    want = ref.compute()
    assert all(np.array_equal(out[k], want[k], equal_nan=True) for k in want)
    # and the loss is the mean squared error of the pass, by the restatement
    zall, rall = np.concatenate([d[0] for d in dense]), np.concatenate([d[1] for d in dense])
    t, _ = E.stored_targets(*(x.numpy() for x in counts._s.csr), rall, len(rall), counts.n_spots, None, scale.numpy(), counts.n_genes)
    mse = ((E.predictions(zall, 1) - t.astype(np.float64)) ** 2).mean()
    print("evaluate_expression: loss %.12g, dense float64 %.12g" % (out['loss'], mse))
    assert abs(out['loss'] - mse) <= 1e-12 * mse
