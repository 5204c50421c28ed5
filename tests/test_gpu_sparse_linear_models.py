"""`SparseCountLinear` / `SparseCountMLP` on a HIP device: against the float64 host restatement within the derived bound, against
the dense layer on expanded rows (each held to float64 with its own bar), the checks, the tape's memory, the spot loop against
the dense tutorial MLP, the native Adam, and `SparseCountGridDataset(first_layer=)` under the grid loop.  Fixture: 3 synthetic
arrays of about 200 spots x 300 genes (tests/sparse_counts_ref.py) after normalize_total(1e4).log1p(), a 64-gene view.

Bounds (u = 2^-24, gamma(n) = (n + 1) u / (1 - (n + 1) u), tests/sparse_linear_ref.py): the sparse forward gamma(n_b) T with n_b
the row's stored entries among the selected genes and T = |bias| + |x| |W|; weight.grad gamma(n_c) T with n_c the batch rows
that store gene c and T = |X|^T |dY|; bias.grad, a sum of B terms in some order, gamma(B) sum |dY|.  The dense GEMM adds all G
terms of a row in an order of its own, products and sums rounded separately at worst: gamma(2 G) T.

Measured on an MI355X (printed by the tests): see the README's sparse-linear section."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

import sparse_counts_ref as R
import sparse_linear_ref as SL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K, C, F1 = 64, 4, 500
_made = {}


def _recipe():
    """(device counts after the recipe, the same values on the host, the 64-gene view of each); built once, never modified."""
    if 'r' not in _made:
        import gridnext_amd as ga
        X, obs, genes = R.synthetic_arrays()
        dev = ga.SpotCounts(X, obs, genes).to(DEV)
        dev.normalize_total(1e4).log1p()
        mean, std = dev.gene_moments()
        with np.errstate(divide='ignore', invalid='ignore'):
            score = np.abs(mean.numpy() / std.numpy())
        ids = [dev.gene_ids[g] for g in R.top_genes(np.where(np.isfinite(score), score, -np.inf), K)]
        host = dev.to('cpu')
        _made['r'] = (dev, host, dev.subset_genes(ids), host.subset_genes(ids))
    return _made['r']


def _expanded(view, rows):
    """(B, G) float32 on the view's device: the rows densified by the existing expand."""
    from gridnext_amd import visium_datasets as V
    dev = 'cpu' if view.device is None else view.device
    out = torch.empty((len(rows), view.n_genes), dtype=torch.float32, device=dev)
    V.expand(view._s.csr, rows.to(torch.int32).to(dev), len(rows), view.gene_channel(), out, view.n_genes)
    return out


def _within(got, want64, bound):
    err = (got.detach().double().cpu() - want64).abs()
    return bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def test_device_layer_against_the_float64_host_layer_and_the_dense_layer():
    import gridnext_amd as ga
    from gridnext_amd import functional as GF
    _, _, dsel, hsel = _recipe()
    torch.manual_seed(11)
    layer = ga.SparseCountLinear(dsel, F1).to(DEV)
    ref = ga.SparseCountLinear.from_linear(layer.to_linear().cpu(), hsel).double()
    rows = torch.from_numpy(np.random.default_rng(1).permutation(dsel.n_spots)[:150].astype(np.int64))
    dy = torch.randn(150, F1)
    out = layer(rows.to(DEV))
    out.backward(dy.to(DEV))
    want = ref(rows)
    want.backward(dy.double())
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == (150, F1)
    x = _expanded(hsel, rows).double()
    W, b = ref.weight.detach(), ref.bias.detach()
    n_b, n_c = (x != 0).sum(1).numpy(), (x != 0).sum(0).numpy()
    T_out, T_dw = x.abs() @ W.abs() + b.abs(), x.abs().t() @ dy.double().abs()
    g = lambda n: torch.from_numpy(SL.gamma(n))                                           # noqa: E731
    ok_o, r_o = _within(out, want.detach(), g(n_b)[:, None] * T_out)
    ok_w, r_w = _within(layer.weight.grad, ref.weight.grad, g(n_c)[:, None] * T_dw)
    ok_b, r_b = _within(layer.bias.grad, ref.bias.grad, float(SL.gamma(150)) * dy.double().abs().sum(0))
    print("sparse layer against float64, largest |err| / bound: forward %.3f, weight.grad %.3f, bias.grad %.3f" % (r_o, r_w, r_b))
    assert ok_o and ok_w and ok_b
    # the dense layer on the expanded rows: to float64 with its own bar
    lin_w = layer.weight.detach().t().contiguous().requires_grad_(True)
    lin_b = layer.bias.detach().clone().requires_grad_(True)
    dense = GF.linear(_expanded(dsel, rows), lin_w, lin_b)
    dense.backward(dy.to(DEV))
    gd = float(SL.gamma(2 * K))
    ok_do, r_do = _within(dense, want.detach(), gd * T_out)
    ok_dw, r_dw = _within(lin_w.grad.t(), ref.weight.grad, float(SL.gamma(2 * 150)) * T_dw)
    print("dense layer against float64, largest |err| / its bound: forward %.3f, weight.grad %.3f" % (r_do, r_dw))
    assert ok_do and ok_dw


def test_views_share_a_layer_and_the_checks():
    import gridnext_amd as ga
    _, _, dsel, hsel = _recipe()
    classes = ga.SparseCountDataset(dsel).classes
    train = ga.SparseCountDataset(dsel.subset_arrays(['arr0', 'arr1']), classes=classes, as_rows=True)
    val = ga.SparseCountDataset(dsel.subset_arrays(['arr2']), classes=classes, as_rows=True)
    torch.manual_seed(12)
    layer = ga.SparseCountLinear(dsel, 40).to(DEV)
    host = ga.SparseCountLinear.from_linear(layer.to_linear().cpu(), hsel).double()
    for ds in (train, val):
        rows, _ = next(iter(DataLoader(ds, batch_size=50, shuffle=True, generator=torch.Generator().manual_seed(3))))
        got = layer(rows.to(DEV))
        assert rows.min() >= ds.rows.min() and torch.allclose(got.double().cpu(), host(rows), rtol=0, atol=1e-4)
    assert int(val.rows.min()) == int(dsel._s.row_start[2])
    twice = torch.tensor([3, 9, 3], device=DEV)
    with pytest.raises(ValueError, match="repeated row"):
        layer(twice)
    with torch.no_grad():
        out = layer(twice)
    assert torch.equal(out[0], out[2])
    with pytest.raises(ValueError, match="outside the storage"):
        layer(torch.tensor([0, dsel._s.row_start[-1]], device=DEV))
    part = ga.SparseCountLinear(dsel.subset_arrays(['arr0']), 8).to(DEV)
    with pytest.raises(ValueError, match="unbound"):
        part(torch.tensor([0, int(dsel._s.row_start[1])], device=DEV))
    with pytest.raises(RuntimeError, match="cpu.*cuda|cuda.*cpu"):
        ga.SparseCountLinear(dsel, 8)(torch.tensor([0]))                                # the weight still on the CPU
    with pytest.raises(RuntimeError, match="cpu.*cuda|cuda.*cpu"):
        ga.SparseCountLinear(hsel, 8).to(DEV)(torch.tensor([0]))
    real = torch.utils.data.get_worker_info
    torch.utils.data.get_worker_info = lambda: object()
    try:
        with pytest.raises(RuntimeError, match="num_workers=0"):
            layer(torch.tensor([0], device=DEV))
    finally:
        torch.utils.data.get_worker_info = real


def test_weight_grad_is_unchanged_under_a_shuffle_of_the_batch():
    import gridnext_amd as ga
    _, _, dsel, _ = _recipe()
    torch.manual_seed(13)
    layer = ga.SparseCountLinear(dsel, 33).to(DEV)
    rows = torch.from_numpy(np.random.default_rng(2).permutation(dsel.n_spots)[:128].astype(np.int64)).to(DEV)
    dy = torch.randn(128, 33, device=DEV)
    grads = []
    for perm in (torch.arange(128), torch.randperm(128), torch.arange(128)):
        layer.weight.grad = None
        layer(rows[perm.to(DEV)]).backward(dy[perm.to(DEV)])
        grads.append(layer.weight.grad.clone())
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32)) and torch.equal(grads[0], grads[2])


def test_the_tape_holds_no_dense_operand():
    """G = 20 000 genes at 2 % non-zeros, B = 256: a dense operand would be B x G x 4 = 20.5 MB.  Forward + backward may
    allocate weight.grad (G x F), the output and its gradient (B x F each; twice that for contiguous copies), bias.grad, the
    column-sum workspace and the int32 / int64 copies of the rows - all but weight.grad far below 1 MiB - and not 20 MB more."""
    import pandas as pd
    import scipy.sparse as sp
    import gridnext_amd as ga
    G, B, F, N = 20000, 256, 100, 300
    X = sp.random(N, G, density=0.02, random_state=5, format='csr', dtype=np.float64)
    X.data = np.random.default_rng(5).integers(1, 50, X.nnz).astype(np.float64)
    obs = pd.DataFrame({'x': np.arange(N) % 60, 'y': np.arange(N) // 60, 'array': 'a', 'annotation': 'c0'},
                       index=['s%d' % k for k in range(N)])
    counts = ga.SpotCounts(X, obs, ['g%d' % g for g in range(G)]).to(DEV)
    torch.manual_seed(14)
    layer = ga.SparseCountLinear(counts, F).to(DEV)
    rows = torch.arange(B, device=DEV)
    layer(rows).sum().backward()                                                        # buffers of the first call exist now
    layer.weight.grad = layer.bias.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = layer(rows)
    out.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    dense_operand = B * G * 4
    allowance = G * F * 4 + 4 * B * F * 4 + (1 << 20)
    print("forward + backward at G=%d, B=%d, F=%d: peak %.2f MB over the base; weight.grad %.2f MB, allowance %.2f MB, a dense "
          "operand would add %.2f MB" % (G, B, F, peak / 1e6, G * F * 4 / 1e6, allowance / 1e6, dense_operand / 1e6))
    assert layer.weight.grad.shape == (G, F) and peak >= G * F * 4
    assert allowance < G * F * 4 + dense_operand // 4 and peak <= allowance


def _rest():
    return nn.Sequential(nn.Linear(F1, 100), nn.BatchNorm1d(100), nn.ReLU(), nn.Linear(100, 100), nn.Linear(100, 50),
                         nn.BatchNorm1d(50), nn.ReLU(), nn.Linear(50, C))


def _loaders(train, val):
    return {'train': DataLoader(train, batch_size=64, shuffle=True, generator=torch.Generator().manual_seed(2)),
            'val': DataLoader(val, batch_size=64)}


def _loop(model, train, val, epochs=2):
    import gridnext_amd as ga
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        model, vh, th = ga.train_spotwise(model, _loaders(train, val), nn.CrossEntropyLoss(), opt, num_epochs=epochs)
    return th, vh, {k: v.detach().clone() for k, v in model.state_dict().items()}


def _float64_loop(model, train, val, epochs=2):
    """The spot loop of training.py restated on the CPU in float64: the same batches, torch's Adam, the epoch's loss as the
    mean over its items."""
    model = model.double()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit, dl = nn.CrossEntropyLoss(), _loaders(train, val)
    th, vh = [], []
    for _ in range(epochs):
        for phase, hist in (('train', th), ('val', vh)):
            model.train(phase == 'train')
            total = 0.0
            for x, y in dl[phase]:
                opt.zero_grad()
                with torch.set_grad_enabled(phase == 'train'):
                    loss = crit(model(x.double()), y)
                    if phase == 'train':
                        loss.backward()
                        opt.step()
                total += float(loss.detach()) * len(y)
            hist.append(total / len(dl[phase].dataset))
    return th, vh


def test_train_spotwise_sparse_against_the_dense_tutorial_mlp(monkeypatch):
    """The sparse and the dense first layer sum in different orders: the histories are not equal bits.  Both are held to a
    float64 CPU run of the dense model over the same batches: the sparse run's per-epoch losses within 4 x the largest distance
    of the fp32 dense GPU run from float64 (the margin of tests/test_gpu_input_grad.py, for the same reason)."""
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    monkeypatch.setenv('GNX_GRAPH', '0')
    _, _, dsel, hsel = _recipe()
    classes = ga.SparseCountDataset(dsel).classes
    sets = {}
    for name, view, kw in (('dense', dsel, {}), ('host', hsel, {}), ('rows', dsel, dict(as_rows=True))):
        sets[name] = (ga.SparseCountDataset(view.subset_arrays(['arr0', 'arr1']), classes=classes, **kw),
                      ga.SparseCountDataset(view.subset_arrays(['arr2']), classes=classes, **kw))

    def sparse_model():
        torch.manual_seed(4)
        return ga.SparseCountMLP(ga.SparseCountLinear(dsel, F1), _rest())

    torch.manual_seed(4)
    dense = count_mlp(K, C)
    same = sparse_model()
    assert torch.equal(same.first.weight, dense[0].weight.t()) and torch.equal(same.first.bias, dense[0].bias)
    assert all(torch.equal(a, b) for a, b in zip(same.rest.state_dict().values(), list(dense.state_dict().values())[2:]))
    torch.manual_seed(4)
    th64, vh64 = _float64_loop(count_mlp(K, C), *sets['host'])
    thd, vhd, _ = _loop(dense, *sets['dense'])
    ths, vhs, sds = _loop(sparse_model(), *sets['rows'])
    ths2, vhs2, sds2 = _loop(sparse_model(), *sets['rows'])
    ref, d_dense, d_sparse = np.array(th64 + vh64), np.abs(np.array(thd + vhd) - np.array(th64 + vh64)), \
        np.abs(np.array(ths + vhs) - np.array(th64 + vh64))
    print("float64", th64, vh64, "\ndense fp32", thd, vhd, "\nsparse", ths, vhs)
    print("per-epoch losses against float64: dense fp32 GPU run at most %.3g, sparse run at most %.3g (bar 4 x %.3g)"
          % (d_dense.max(), d_sparse.max(), d_dense.max()))
    assert np.isfinite(ref).all() and len(ths) == len(vhs) == 2
    assert (d_sparse <= 4 * d_dense.max()).all()
    assert ths == ths2 and vhs == vhs2 and all(torch.equal(sds[k], sds2[k]) for k in sds)   # the same seed: the same run
    assert sorted(sds)[:2] == ['first.bias', 'first.weight']


def test_native_adam_steps_the_layer_and_the_state_dict_loads_into_a_linear():
    import gridnext_amd as ga
    from gridnext_amd import optim
    _, _, dsel, _ = _recipe()
    torch.manual_seed(15)
    src = nn.Linear(K, 20).to(DEV)
    layer = ga.SparseCountLinear.from_linear(src, dsel)
    assert layer.weight.is_cuda and torch.equal(layer.weight, src.weight.t())
    opt = optim.Adam(layer.parameters(), lr=1e-2)
    before, v0 = layer.weight.detach().clone(), layer.weight._version
    layer(torch.arange(100, device=DEV)).square().sum().backward()
    opt.step()
    torch.cuda.synchronize()
    assert layer.weight._version > v0 and not torch.equal(layer.weight, before) and torch.isfinite(layer.weight).all()
    assert float((layer.weight - before).abs().max()) <= 1.01e-2                       # Adam's first step: lr at most
    src.load_state_dict(layer.to_linear().state_dict())
    assert torch.equal(src.weight, layer.weight.t()) and torch.equal(src.bias, layer.bias)
    assert list(layer.state_dict()) == ['weight', 'bias']


# ------------------------------------------------------------------------------------------------ the grid stage
F2 = 32


def _frozen_first():
    import gridnext_amd as ga
    _, _, dsel, _ = _recipe()
    torch.manual_seed(16)
    return ga.SparseCountLinear(dsel, F2).to(DEV).requires_grad_(False)


def test_grid_items_from_a_first_layer(monkeypatch):
    import gridnext_amd as ga
    from gridnext_amd import _lib
    _, _, dsel, hsel = _recipe()
    first = _frozen_first()
    ref = ga.SparseCountLinear.from_linear(first.to_linear().cpu(), hsel).double()
    grid, plain = ga.SparseCountGridDataset(dsel, first_layer=first), ga.SparseCountGridDataset(hsel)
    grid[0]
    seen, real = [], _lib.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    items = [grid[k] for k in range(3)]
    assert seen == ['gnx_sparse_linear_fwd_f32'] * 3                                    # one forward launch per item
    monkeypatch.setattr(_lib, 'call', real)
    worst = 0.0
    for k, (feats, labels) in enumerate(items):
        x, y = plain[k]
        assert feats.is_cuda and feats.shape == (F2, 78, 64) and torch.equal(labels.cpu(), y)
        flat, xd = feats.reshape(F2, -1).t().cpu(), x.reshape(K, -1).t().double()
        occupied = (y > 0).reshape(-1)
        assert 150 < int(occupied.sum()) < 78 * 64 and torch.equal(flat[~occupied], first.bias.cpu().expand(int((~occupied).sum()), F2))
        want = xd @ ref.weight.detach() + ref.bias.detach()
        T = xd.abs() @ ref.weight.detach().abs() + ref.bias.detach().abs()
        ok, ratio = _within(flat[occupied], want[occupied], torch.from_numpy(SL.gamma((xd != 0).sum(1).numpy()))[occupied][:, None] * T[occupied])
        assert ok
        worst = max(worst, ratio)
    print("grid items against float64 at the occupied cells: largest |err| / bound %.3f" % worst)


def _tensors(ds):
    return TensorDataset(torch.stack([ds[k][0] for k in range(len(ds))]), torch.stack([ds[k][1] for k in range(len(ds))]).to(DEV))


def _grid_loop(train, val, epochs, cached):
    import gridnext_amd as ga
    torch.manual_seed(3)
    f = nn.Sequential(nn.Linear(F2, 16), nn.BatchNorm1d(16), nn.ReLU(), nn.Linear(16, C))
    for p in f.parameters():
        p.requires_grad = False
    m = ga.GridNetHexOddr(f, (F2,), (78, 64), C)
    if cached:
        m.enable_f_cache()
    dl = {'train': DataLoader(train, batch_size=1, shuffle=True, generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(val, batch_size=1)}
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        m, vh, th = ga.train_gridwise(m, dl, nn.CrossEntropyLoss(), opt, num_epochs=epochs)
    counts = (m.f_cache.hits, m.f_cache.misses) if cached else None
    return th, vh, {k: v.clone() for k, v in m.state_dict().items()}, counts


def test_train_gridwise_on_first_layer_features(monkeypatch):
    """The grid loop fed by SparseCountGridDataset(first_layer=) == the loop fed the same feature tensors from a TensorDataset;
    with enable_f_cache() and GNX_GRAPH=0 the look-ups are those of the count-grid dataset's test
    (tests/test_gpu_sparse_count_datasets.py): 2 arrays x 2 phases x 3 epochs = 12, 2 misses, 10 hits."""
    import gridnext_amd as ga
    _, _, dsel, _ = _recipe()
    first = _frozen_first()
    classes = ga.SparseCountGridDataset(dsel).classes
    train = ga.SparseCountGridDataset(dsel.subset_arrays(['arr0', 'arr1']), classes=classes, first_layer=first)
    val = ga.SparseCountGridDataset(dsel.subset_arrays(['arr2']), classes=classes, first_layer=first)
    th0, vh0, sd0, _ = _grid_loop(_tensors(train), _tensors(val), 1, False)
    th1, vh1, sd1, _ = _grid_loop(train, val, 1, False)
    print("tensors", th0, vh0, "first-layer items", th1, vh1)
    assert len(th0) == 1 and np.isfinite(th0[0]) and th0 == th1 and vh0 == vh1
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    monkeypatch.setenv('GNX_GRAPH', '0')
    th2, vh2, _, counts = _grid_loop(train, train, 3, True)
    print("3 epochs, every step eager: cached", th2, vh2, "(hits, misses)", counts)
    assert counts == (10, 2) and len(th2) == 3
