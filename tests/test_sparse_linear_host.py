"""The sparse first layer without a GPU: the numpy restatement of csrc/sparse_linear.hip (tests/sparse_linear_ref.py) against
scipy.sparse float64 products, the host path of `SparseCountLinear` against nn.Linear on expanded rows, its conversions and
refusals, the two dataset keywords, and the spot loop on the CPU.  Fixture: tests/sparse_counts_ref.py's synthetic arrays."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

import sparse_counts_ref as R
import sparse_linear_ref as SL

F, K = 24, 64
_made = {}


def _counts():
    """(host SpotCounts after the tutorial's recipe, a 64-gene view of it); built once, never modified."""
    if 'c' not in _made:
        import gridnext_amd as ga
        X, obs, genes = R.synthetic_arrays(n_spots=60)
        c = ga.SpotCounts(X, obs, genes)
        c.normalize_total(1e4).log1p()
        pick = [genes[g] for g in np.random.default_rng(0).permutation(300)[:K]]
        _made['c'] = (c, c.subset_genes(pick))
    return _made['c']


def _dense_rows(view, rows):
    import gridnext_amd as ga
    ds = ga.SparseCountDataset(view.subset_arrays(view._s.array_names))
    at = {int(r): k for k, r in enumerate(ds.rows)}
    return torch.stack([ds[at[int(r)]][0] for r in rows])


def test_restatement_equals_scipy_products_in_float64():
    rng = np.random.default_rng(1)
    lengths = [0, 1, 63, 64, 65, 257, 0, 300]
    ptr, idx, val = R.random_lines(rng, lengths, 400, integer=False)
    chan = np.full(400, -1, dtype=np.int32)
    kept = rng.choice(400, size=300, replace=False)
    chan[kept] = rng.permutation(300)
    W, bias = rng.standard_normal((300, 37)).astype(np.float32), rng.standard_normal(37).astype(np.float32)
    lines = np.array([7, 5, 5, -1, 0, 3, 2, 1], dtype=np.int32)
    X = SL.to_scipy(ptr, idx, val, 400).tocsc()[:, np.argsort(np.where(chan < 0, 10 ** 6, chan), kind='stable')[:300]].tocsr()
    want = np.zeros((len(lines), 37))
    want[lines >= 0] = X[lines[lines >= 0]] @ W.astype(np.float64)
    want += bias.astype(np.float64)
    out, T, n = SL.fwd64(ptr, idx, val, lines, len(lines), chan, W, bias)
    assert np.allclose(out, want, rtol=0, atol=1e-12 * T.max())
    assert list(n) == [int((chan[idx[ptr[l]:ptr[l + 1]]] >= 0).sum()) if l >= 0 else 0 for l in lines]
    out32 = SL.fwd32(ptr, idx, val, lines, len(lines), chan, W, bias)
    assert (np.abs(out32 - out) <= SL.gamma(n)[:, None] * T).all()
    assert np.array_equal(out32[3], bias)
    # weight gradient: lines are genes, idx the spots of one array, pos the spot's place in the batch
    n_spots, B = 350, 120
    gptr, gidx, gval = R.random_lines(rng, lengths + [40] * 12, n_spots, integer=False)
    pos = np.full(n_spots, -1, dtype=np.int32)
    pos[rng.choice(n_spots, size=B, replace=False)] = rng.permutation(B)
    dY = rng.standard_normal((B, 37)).astype(np.float32)
    Xa = SL.to_scipy(gptr, gidx, gval, n_spots)                                      # genes x spots of the array
    in_batch = np.flatnonzero(pos >= 0)
    want = Xa[:, in_batch] @ dY.astype(np.float64)[pos[in_batch]]
    dW, T, n = SL.wgrad64(gptr, gidx, gval, None, len(gptr) - 1, pos, dY)
    assert np.allclose(dW, want, rtol=0, atol=1e-12 * T.max())
    dW32 = SL.wgrad32(gptr, gidx, gval, None, len(gptr) - 1, pos, dY)
    assert (np.abs(dW32 - dW) <= SL.gamma(n)[:, None] * T).all()
    ones = SL.fwd32(ptr, idx, np.ones_like(val), None, len(lengths), None, np.ones((400, 5), np.float32), np.full(5, 2, np.float32))
    assert np.array_equal(ones, np.array(lengths, dtype=np.float32)[:, None] + 2 + np.zeros((1, 5), np.float32))


def test_fma32_rounds_once():
    a = np.array([1 + 2.0 ** -12, 3, 1], dtype=np.float32)
    b = np.array([1 + 2.0 ** -12, 2.0 ** -25, 2.0 ** -24], dtype=np.float32)
    c = np.array([2.0 ** -30, 1, 1], dtype=np.float32)
    exact = [float(x) * float(y) + float(z) for x, y, z in zip(a, b, c)]               # exact in Python floats here
    assert np.array_equal(SL.fma32(a, b, c), np.array(exact).astype(np.float32))
    # 8392705 * 8384513 = 2^46 + 1: the product is 2^-24 + 2^-70, and 1 + 2^-24 + 2^-70 lies just above the float32 tie.
    # float64 rounds the sum to the tie itself, whose float32 rounding goes to even (1.0); the fused instruction rounds up
    a, b, c = np.array([8392705], np.float32), np.array([8384513 * 2.0 ** -70], np.float32), np.array([1], np.float32)
    assert float(a[0]) * float(b[0]) == 2.0 ** -24 + 2.0 ** -70
    assert np.float32(float(a[0]) * float(b[0]) + 1.0) == np.float32(1)                # rounded twice
    assert SL.fma32(a, b, c)[0] == np.float32(1 + 2.0 ** -23)
    assert SL.fma32(a, -b, -c)[0] == np.float32(-1 - 2.0 ** -23)


def test_same_seed_initialisation_and_state_dict():
    import gridnext_amd as ga
    _, view = _counts()
    torch.manual_seed(5)
    layer = ga.SparseCountLinear(view, F)
    after_sparse = torch.rand(1)
    torch.manual_seed(5)
    lin = nn.Linear(K, F)
    assert torch.equal(after_sparse, torch.rand(1))                                    # the same number of draws
    assert layer.weight.shape == (K, F) and torch.equal(layer.weight, lin.weight.t()) and torch.equal(layer.bias, lin.bias)
    assert list(layer.state_dict().keys()) == ['weight', 'bias']
    assert ga.SparseCountLinear(view, F, bias=False).bias is None
    back = layer.to_linear()
    assert torch.equal(back.weight, lin.weight) and torch.equal(back.bias, lin.bias)
    again = ga.SparseCountLinear.from_linear(back, view)
    assert torch.equal(again.weight, layer.weight) and torch.equal(again.bias, layer.bias)
    lin.load_state_dict(again.to_linear().state_dict())
    with pytest.raises(ValueError, match="genes"):
        ga.SparseCountLinear.from_linear(nn.Linear(K + 1, F), view)


@pytest.mark.parametrize("selected", [False, True])
def test_host_layer_equals_linear_on_expanded_rows_in_float64(selected):
    import gridnext_amd as ga
    whole, view = _counts()
    c = view if selected else whole
    torch.manual_seed(6)
    layer = ga.SparseCountLinear(c, F).double()
    lin = layer.to_linear()
    assert lin.weight.dtype == torch.float64
    rows = torch.from_numpy(np.random.default_rng(2).permutation(c.n_spots)[:50].astype(np.int64))
    x = _dense_rows(c, rows).double()
    dy = torch.randn(50, F, dtype=torch.float64)
    out, ref = layer(rows), lin(x)
    assert out.dtype == torch.float64 and torch.allclose(out, ref, rtol=0, atol=1e-12 * float(ref.detach().abs().max()))
    (out * dy).sum().backward()
    (ref * dy).sum().backward()
    assert torch.allclose(layer.weight.grad, lin.weight.grad.t(), rtol=0, atol=1e-12 * float(lin.weight.grad.abs().max()))
    assert torch.allclose(layer.bias.grad, lin.bias.grad, rtol=0, atol=1e-12 * float(lin.bias.grad.abs().max()))
    assert float(layer.weight.grad.abs().max()) > 0
    # float32 module: the same function within the derived bound of its own float64 value
    layer32 = ga.SparseCountLinear.from_linear(lin.float(), c)
    got = layer32(rows.int()).detach().numpy()
    n = np.array([(x[k] != 0).sum() for k in range(50)])
    T = (x.abs() @ lin.weight.double().abs().t() + lin.bias.double().abs()).detach().numpy()
    assert got.dtype == np.float32 and (np.abs(got - ref.detach().numpy()) <= (SL.gamma(n)[:, None] + SL.U) * T + 1e-30).all()


def test_from_affine_evaluates_a_pca_projection():
    import gridnext_amd as ga
    _, view = _counts()
    rng = np.random.default_rng(3)
    rows = torch.arange(0, view.n_spots, 3)
    x = _dense_rows(view, rows).double().numpy()
    mean = x.mean(0)
    V = np.linalg.svd(x - mean, full_matrices=False)[2][:7].T                         # (G, 7): components_.T
    layer = ga.SparseCountLinear.from_affine(view, V, -mean @ V)
    assert not any(p.requires_grad for p in layer.parameters()) and layer.weight.shape == (K, 7)
    got = layer(rows)
    assert not got.requires_grad
    want = (x - mean) @ V
    T = np.abs(x) @ np.abs(V) + np.abs(mean @ V)
    n = (x != 0).sum(1)
    # the affine form in fp32: the layer's own bound plus the rounding of V and the bias to float32 (one u each)
    assert (np.abs(got.numpy() - want) <= (SL.gamma(n)[:, None] + 2 * SL.U) * T).all()
    assert rng is not None


def test_refusals_name_what_they_refuse():
    import gridnext_amd as ga
    whole, view = _counts()
    torch.manual_seed(7)
    two = view.subset_arrays(['arr0', 'arr2'])
    layer = ga.SparseCountLinear(two, F)
    r1 = int(whole._s.row_start[1])
    ok = torch.tensor([0, 5, int(whole._s.row_start[2]) + 1])
    layer(ok).sum().backward()
    with pytest.raises(ValueError, match="repeated row"):
        layer(torch.tensor([3, 4, 3]))
    with pytest.raises(ValueError, match="unbound"):
        layer(torch.tensor([0, r1 + 2]))
    with pytest.raises(ValueError, match="outside the storage"):
        layer(torch.tensor([0, whole.n_spots]))
    with torch.no_grad():
        assert layer(torch.tensor([3, 4, 3, r1 + 2])).shape == (4, F)                 # nothing to lose without a gradient
    unchecked = ga.SparseCountLinear(two, F, check_rows=False)
    assert unchecked(torch.tensor([3, 4, 3])).shape == (3, F)
    with pytest.raises(TypeError, match="int64 or int32"):
        layer(torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="arr1"):
        layer.array_rows('arr1', torch.zeros(1, dtype=torch.int32), 4)
    # the grid dataset's keyword
    with pytest.raises(ValueError, match="requires grad"):
        ga.SparseCountGridDataset(two, first_layer=layer)
    for p in layer.parameters():
        p.requires_grad = False
    ga.SparseCountGridDataset(two, first_layer=layer)
    X, obs, genes = R.synthetic_arrays(n_spots=60)
    other = ga.SpotCounts(X, obs, genes)
    with pytest.raises(ValueError, match="another storage"):
        ga.SparseCountGridDataset(other, first_layer=layer)
    with pytest.raises(ValueError, match="gene selection"):
        ga.SparseCountGridDataset(whole, first_layer=layer)
    with pytest.raises(TypeError, match="SparseCountLinear"):
        ga.SparseCountMLP(nn.Linear(K, F), nn.Sequential())
    with pytest.raises(TypeError, match="SpotCounts"):
        ga.SparseCountLinear(X, F)


def test_dataset_keywords_and_their_defaults():
    import gridnext_amd as ga
    from gridnext_amd import visium_datasets as V
    _, view = _counts()
    ds, as_rows = ga.SparseCountDataset(view), ga.SparseCountDataset(view, as_rows=True)
    assert len(ds) == len(as_rows) and not ds.as_rows
    items = [as_rows[k] for k in range(len(as_rows))]
    assert all(x.dtype == torch.int64 and x.dim() == 0 and y.dtype == torch.int64 for x, y in items)
    assert np.array_equal(np.array([int(x) for x, _ in items]), ds.rows)
    assert all(torch.equal(y, ds[k][1]) for k, (_, y) in enumerate(items))
    xb, yb = next(iter(DataLoader(as_rows, batch_size=7)))
    assert xb.dtype == torch.int64 and xb.shape == (7,) and np.array_equal(xb.numpy(), ds.rows[:7])
    # the defaults yield what the path without the keywords yields: the expand of the same lines
    picks = [4, 0, 9]
    buf = torch.empty((3, K))
    V.expand(view._s.csr, torch.from_numpy(ds.rows[picks]), 3, view.gene_channel(), buf, K)
    assert all(torch.equal(ds.__getitems__(picks)[k][0], buf[k]) for k in range(3))
    grid = ga.SparseCountGridDataset(view)
    x, y = grid[1]
    cells, labels = grid._array(1)
    out = torch.empty((K, 78 * 64))
    V.expand(view._s.csc[1], view.gene_lines(), K, cells, out, 78 * 64)
    assert grid.first_layer is None and torch.equal(x, out.view(K, 78, 64)) and torch.equal(y, labels)
    # with a first layer: the layer's rows at the occupied cells, its bias elsewhere
    torch.manual_seed(8)
    layer = ga.SparseCountLinear(view, F).requires_grad_(False)
    feats, y2 = ga.SparseCountGridDataset(view, first_layer=layer)[1]
    assert feats.shape == (F, 78, 64) and feats.dtype == torch.float32 and torch.equal(y2, y)
    rows = torch.arange(int(view._s.row_start[1]), int(view._s.row_start[2]))
    flat = feats.reshape(F, -1).t()
    assert torch.equal(flat[cells.long()], layer(rows))
    empty = torch.ones(78 * 64, dtype=torch.bool)
    empty[cells.long()] = False
    assert int(empty.sum()) > 4000 and torch.equal(flat[empty], layer.bias.expand(int(empty.sum()), F))
    dense = layer.to_linear()(x.reshape(K, -1).t().contiguous()).detach()
    assert torch.allclose(flat, dense, rtol=0, atol=1e-5 * float(dense.abs().max()))


def test_train_spotwise_on_the_cpu_over_rows(monkeypatch):
    import gridnext_amd as ga
    from gridnext_amd import distributed
    from gridnext_amd.synthetic import count_mlp
    monkeypatch.setattr(distributed, 'default_device', lambda: torch.device('cpu'))    # the host path, also beside a GPU
    _, view = _counts()
    classes = ga.SparseCountDataset(view).classes
    train = ga.SparseCountDataset(view.subset_arrays(['arr0', 'arr1']), classes=classes, as_rows=True)
    val = ga.SparseCountDataset(view.subset_arrays(['arr2']), classes=classes, as_rows=True)
    torch.manual_seed(9)
    dense = count_mlp(K, len(classes))
    model = ga.SparseCountMLP(ga.SparseCountLinear.from_linear(dense[0], view), nn.Sequential(*list(dense)[1:]))
    before = model.first.weight.detach().clone()
    dl = {'train': DataLoader(train, batch_size=32, shuffle=True, generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(val, batch_size=32)}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        model, vh, th = ga.train_spotwise(model, dl, nn.CrossEntropyLoss(), opt, num_epochs=2)
    assert len(vh) == len(th) == 2 and all(np.isfinite(v) for v in vh + th)
    assert not model.first.weight.is_cuda and not torch.equal(model.first.weight.detach(), before)


def test_new_symbols_are_declared_and_exported():
    import gridnext_amd as ga
    from gridnext_amd import _lib
    for name in ('gnx_sparse_linear_fwd_f32', 'gnx_sparse_linear_wgrad_f32', 'gnx_sparse_linear_max_f'):
        assert name in _lib.SIGNATURES
    assert _lib.PARAMS['gnx_sparse_linear_fwd_f32'] == ['lineptr', 'idx', 'val', 'lines', 'n_lines', 'chan_of_idx', 'W', 'ldw',
                                                        'bias', 'out', 'ld_out', 'F', 'stream']
    assert _lib.PARAMS['gnx_sparse_linear_wgrad_f32'] == ['lineptr', 'idx', 'val', 'gene_lines', 'n_channels', 'pos_of_idx', 'dY',
                                                          'ld_dy', 'dW', 'ldw', 'F', 'accumulate', 'stream']
    assert ga.SparseCountLinear is ga.sparse_linear.SparseCountLinear and ga.SparseCountMLP is ga.sparse_linear.SparseCountMLP
