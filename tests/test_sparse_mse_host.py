"""Expression from patches on the host: the numpy restatement (tests/sparse_mse_ref.py) against torch's float64 composition,
`SparseMSELoss` on host counts against the composition it replaces (bit for bit), `SpotCounts.gene_max` and `unit_scale`
against scipy, `SlideCountDataset` over a written Spaceranger-like tree, `train_expression` against a hand-written loop, and
every refusal.  No GPU."""
import copy
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

import sparse_counts_ref as CR
import sparse_mse_ref as R
from test_sparse_counts_ref_host import _trees, _write_annots

CPU = torch.device('cpu')


def _dense(counts):
    """float32 (storage rows, selected genes) of a host SpotCounts, by scipy."""
    ptr, idx, val = (t.numpy() for t in counts._s.csr)
    X = sp.csr_matrix((val, idx, ptr), shape=(len(ptr) - 1, len(counts._s.gene_ids))).toarray()
    return X if counts._genes is None else X[:, counts._genes]


def _counts(n_arrays=2, n_genes=40, n_spots=30, normalise=True):
    import gridnext_amd as ga
    X, obs, genes = CR.synthetic_arrays(seed=4, n_arrays=n_arrays, n_genes=n_genes, n_spots=n_spots)
    counts = ga.SpotCounts(X, obs, genes)
    if normalise:
        counts.normalize_total(1e4).log1p()
    return counts, genes


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("activation", [0, 1])
@pytest.mark.parametrize("reduction", ['mean', 'sum'])
def test_restatement_is_torchs_float64_composition(activation, reduction):
    rng = np.random.default_rng(1)
    ptr, idx, val = CR.random_lines(rng, [0, 1, 63, 64, 65, 20], 70, integer=False)
    pos = rng.permutation(70).astype(np.int32)
    pos[rng.random(70) < 0.2] = -1
    scale = (rng.random(70) * 0.2).astype(np.float32)
    rows = np.array([5, 4, 4, 0, 9, -1, 2], dtype=np.int32)                       # a repeat, two rows outside the storage
    t = R.targets(ptr, idx, val, rows, 7, 6, pos, scale, 70)
    assert not t[4].any() and not t[5].any() and np.array_equal(t[1], t[2])
    dense = CR.expand(ptr, idx, val, np.array([5, 4, 4, 0, 2], dtype=np.int32), 5, pos, 70)
    assert np.array_equal(t[[0, 1, 2, 3, 6]], dense * scale)
    z = (rng.standard_normal((7, 70)) * 3).astype(np.float32)
    loss, dz = R.loss_and_grad_f64(z, t, activation, reduction, dloss=0.5)
    assert loss == R.loss_and_grad_f64(z, t, activation, reduction)[0]                # dloss scales the gradient alone
    zt = torch.from_numpy(z).double().requires_grad_()
    p = torch.sigmoid(zt) if activation else zt
    want = F.mse_loss(p, torch.from_numpy(t).double(), reduction=reduction)
    (0.5 * want).backward()
    assert abs(loss - float(want.detach())) <= 1e-14 * abs(float(want.detach()))
    assert np.allclose(dz, zt.grad.numpy(), rtol=1e-13, atol=1e-300)


def test_restated_line_max():
    rng = np.random.default_rng(2)
    ptr, idx, val = CR.random_lines(rng, [0, 1, 63, 64, 65, 257], 300)
    dense = CR.expand(ptr, idx, val, None, 6, None, 300)
    assert np.array_equal(R.line_max(ptr, idx, val, None, 6), dense.max(1))
    mask = (rng.random(300) < 0.5).astype(np.uint8)
    lines = np.array([5, 0, 5, 3], dtype=np.int32)
    assert np.array_equal(R.line_max(ptr, idx, val, lines, 4, mask), (dense * mask)[lines].max(1))


# ------------------------------------------------------------------------------------------------ the criterion on host counts
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("reduction", ['mean', 'sum'])
def test_host_criterion_is_the_composition_bit_for_bit(dtype, reduction):
    import gridnext_amd as ga
    counts, genes = _counts()
    rng = np.random.default_rng(3)
    picked = [genes[g] for g in rng.permutation(40)[:17]]                           # a subset, in a permuted order
    for view in (counts, counts.subset_genes(picked), counts.subset_genes(picked).subset_arrays(['arr1'])):
        dense = torch.from_numpy(_dense(view))
        scale = ga.SparseMSELoss.unit_scale(view)
        lo = int(view._s.row_start[view._arrays[0]])
        rows = torch.from_numpy(rng.integers(lo, lo + 20, 9))
        for act, sc in (('sigmoid', scale), ('sigmoid', None), (None, scale)):
            crit = ga.SparseMSELoss(view, activation=act, gene_scale=sc, reduction=reduction)
            z = torch.from_numpy(rng.standard_normal((9, view.n_genes))).to(dtype).requires_grad_()
            loss = crit(z, rows)
            loss.backward()
            z2 = z.detach().clone().requires_grad_()
            target = dense[rows].to(dtype)
            if sc is not None:
                target = target * sc.to(dtype)
            want = F.mse_loss(torch.sigmoid(z2) if act else z2, target, reduction=reduction)
            want.backward()
            assert loss.dtype == dtype and loss.dim() == 0 and torch.equal(loss, want) and torch.equal(z.grad, z2.grad)
            assert torch.equal(crit.activate(z.detach()), torch.sigmoid(z.detach()) if act else z.detach())
        assert torch.equal(crit(z.detach(), rows.int()), crit(z.detach(), rows))                 # int32 rows
    # the restatement's targets are the module's
    view = counts.subset_genes(picked)
    t = R.targets(*(x.numpy() for x in view._s.csr), rows.numpy(), 9, int(view._s.row_start[-1]), view.gene_channel().numpy(),
                  None, 17)
    assert np.array_equal(t, _dense(view)[rows.numpy()])
    sc = ga.SparseMSELoss.unit_scale(view).numpy()
    t = R.targets(*(x.numpy() for x in view._s.csr), rows.numpy(), 9, int(view._s.row_start[-1]), view.gene_channel().numpy(), sc, 17)
    assert np.array_equal(t, _dense(view)[rows.numpy()] * sc)


def test_gene_max_and_unit_scale_against_scipy():
    import gridnext_amd as ga
    counts, genes = _counts(normalise=False)
    dense = _dense(counts)
    none = int(np.flatnonzero(dense.max(0) == 0)[0]) if (dense.max(0) == 0).any() else None
    if none is None:                                                                # make sure one gene has no entry at all
        X, obs, genes = CR.synthetic_arrays(seed=4, n_arrays=2, n_genes=40, n_spots=30)
        X = X.tolil()
        X[:, 7] = 0
        counts, none = ga.SpotCounts(X.tocsr(), obs, genes), 7
        dense = _dense(counts)
    counts.normalize_total(1e4).log1p()
    dense = _dense(counts)
    m = counts.gene_max()
    assert m.dtype == torch.float32 and m.device == CPU and m[none] == 0
    assert np.array_equal(m.numpy(), sp.csc_matrix(dense).max(axis=0).toarray().ravel())
    view = counts.subset_genes([genes[g] for g in (9, 3, none, 21)])
    assert np.array_equal(view.gene_max().numpy(), dense[:, [9, 3, none, 21]].max(0))
    r0, r1 = (int(v) for v in counts._s.row_start[1:3])
    assert np.array_equal(view.gene_max(arrays=['arr1']).numpy(), dense[r0:r1][:, [9, 3, none, 21]].max(0))
    assert np.array_equal(view.subset_arrays(['arr1']).gene_max().numpy(), view.gene_max(arrays=['arr1']).numpy())
    scale = ga.SparseMSELoss.unit_scale(counts)
    assert scale.dtype == torch.float32 and scale[none] == 1
    target = dense * scale.numpy()
    assert target.min() >= 0 and target.max() <= 1
    mx = m.numpy()
    has = mx > 0
    assert np.array_equal(target.max(0)[has], (mx[has] * (np.float32(1) / mx[has])).astype(np.float32))


def test_criterion_refusals():
    import gridnext_amd as ga
    counts, genes = _counts()
    view = counts.subset_arrays(['arr1'])
    crit = ga.SparseMSELoss(view)
    r0, r1 = (int(v) for v in counts._s.row_start[1:3])
    z = torch.zeros(2, 40)
    crit(z, torch.tensor([r0, r1 - 1]))
    with pytest.raises(ValueError, match="bound arrays"):
        crit(z, torch.tensor([r0, r0 - 1]))                                         # a row of arr0: not of the bound view
    with pytest.raises(ValueError, match="bound arrays"):
        crit(z, torch.tensor([r0, int(counts._s.row_start[-1])]))                   # outside the storage
    with pytest.raises(ValueError, match="bound arrays"):
        crit(z, torch.tensor([-1, r0]))
    with pytest.raises(ValueError, match=r"\(B, 40\)"):
        crit(torch.zeros(2, 39), torch.tensor([r0, r0]))
    with pytest.raises(ValueError, match="floating point"):
        crit(torch.zeros(2, 40, dtype=torch.int64), torch.tensor([r0, r0]))
    with pytest.raises(ValueError, match="rows must be"):
        crit(z, torch.tensor([r0]))
    with pytest.raises(ValueError, match="rows must be"):
        crit(z, torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="z is on meta, the counts are on cpu"):
        crit(torch.zeros(2, 40, device='meta'), torch.tensor([r0, r0]))
    with pytest.raises(ValueError, match="activation"):
        ga.SparseMSELoss(counts, activation='relu')
    with pytest.raises(ValueError, match="reduction"):
        ga.SparseMSELoss(counts, reduction='none')
    with pytest.raises(ValueError, match=r"gene_scale must be \(40,\)"):
        ga.SparseMSELoss(counts, gene_scale=torch.ones(39))
    with pytest.raises(TypeError, match="SpotCounts"):
        ga.SparseMSELoss(object())
    resident = counts._view(counts._genes, counts._arrays)                          # counts that say they live on a device
    resident._s = copy.copy(counts._s)
    resident._s.device = torch.device('cuda:0')
    with pytest.raises(RuntimeError, match="the counts are on cuda:0; the criterion has no device form"):
        ga.SparseMSELoss(resident)
    free = ga.SparseMSELoss(view, check_rows=False)                                 # unchecked: a row of arr0 gets its target
    assert torch.isfinite(free(z, torch.tensor([r0 - 1, r0])))
    assert not list(crit.parameters()) and not crit.state_dict()                    # nothing to optimise, nothing to save


def test_expression_net_on_the_host():
    import gridnext_amd as ga
    torch.manual_seed(0)
    back = nn.Sequential(nn.Flatten(), nn.Linear(12, 5))
    net = ga.ExpressionNet(back, 7, in_features=5)
    x = torch.randn(3, 3, 2, 2)
    assert torch.equal(net(x), net.head(back(x))) and net(x).shape == (3, 7)
    with pytest.raises(ValueError, match="in_features"):
        ga.ExpressionNet(back, 7)
    with pytest.raises(ValueError, match="the head takes"):
        ga.ExpressionNet(back, 7, in_features=6)(x)
    dn = ga.DenseNet(growth_rate=4, block_config=(1, 1), num_init_features=8, bn_size=2, small_inputs=True, classify=False)
    net = ga.ExpressionNet(dn, 9)
    assert net.head.in_features == dn.num_features and net.head.out_features == 9


# ------------------------------------------------------------------------------------------------ SlideCountDataset
def _slide_setup(tmp_path):
    import gridnext_amd as ga
    trees = _trees(tmp_path)
    dirs = [t[0] for t in trees]
    slide = np.random.default_rng(8).integers(0, 256, size=(520, 470, 3), dtype=np.uint8)
    return ga, trees, dirs, slide


def test_slide_count_dataset_on_the_host(tmp_path):
    ga, trees, dirs, slide = _slide_setup(tmp_path)
    annots = _write_annots(tmp_path, trees)
    counts = ga.create_visium_counts(dirs, annots)                                  # the annotated in-tissue spots only
    every = ga.create_visium_counts(dirs)
    ds = ga.SlideCountDataset([slide, slide], dirs, counts, patch_size=8, window_size=12)
    assert len(ds) == counts.n_spots and ds.dropped == every.n_spots - counts.n_spots > 0
    obs = counts.obs
    # rows against obs: arrays in the order of counts.arrays, spots in the position file's order
    want_rows, want_px = [], []
    for k, name in enumerate(counts.arrays):
        at = {(x, y): r for r, (x, y, a) in enumerate(zip(obs['x'], obs['y'], obs['array'])) if a == name}
        for b, inside, r, c, pr, pc in trees[k][3]:
            if inside and (c, r) in at:
                want_rows.append(at[(c, r)])
                want_px.append((k, pc, pr))
    assert ds.rows.tolist() == want_rows and ds.items == want_px and ds.rows.dtype == np.int64
    classes, ids = ga.visium_datasets._labels_of(counts, None)
    assert list(ds.classes) == list(classes) and ds.annotations.tolist() == ids[ds.rows].tolist()
    plain = ga.SlidePatchDataset([slide, slide], dirs, patch_size=8, window_size=12)
    where = {item: j for j, item in enumerate(plain.items)}
    picks = [len(ds) - 1, 0, 3, len(ds) - 1]
    batch = ds.__getitems__(picks)
    for (patch, row, label), k in zip(batch, picks):
        assert torch.equal(patch, plain[where[ds.items[k]]][0]) and patch.dtype == torch.uint8 and patch.shape == (3, 8, 8)
        assert row.dtype == torch.int64 and row.dim() == 0 and int(row) == ds.rows[k] and int(label) == ds.annotations[k]
    one = ds[2]
    assert torch.equal(one[0], ds.__getitems__([2])[0][0]) and int(one[1]) == ds.rows[2]
    from torch.utils.data import DataLoader
    xb, rb, yb = next(iter(DataLoader(ds, batch_size=5)))
    assert xb.shape == (5, 3, 8, 8) and rb.tolist() == ds.rows[:5].tolist() and yb.tolist() == ds.annotations[:5].tolist()
    # the other order of arrays, a view on one array, no annotations: labels -1
    rev = ga.SlideCountDataset([slide, slide], dirs[::-1], counts, patch_size=8, window_size=12)
    assert rev.rows.tolist() == want_rows and [(1 - k, x, y) for k, x, y in rev.items] == want_px
    only = ga.SlideCountDataset([slide], dirs[1:], counts.subset_arrays(['sampleB']), patch_size=8, window_size=12)
    assert only.rows.tolist() == [r for r, (k, _, _) in zip(want_rows, want_px) if k == 1]
    bare = ga.SlideCountDataset([slide, slide], dirs, every, patch_size=8, window_size=12, raw_uint8=False)
    assert bare.dropped == 0 and set(bare.annotations.tolist()) == {-1} and bare[0][0].dtype == torch.float32
    assert sorted(bare.rows.tolist()) == list(range(every.n_spots))


def test_slide_count_dataset_refusals(tmp_path):
    ga, trees, dirs, slide = _slide_setup(tmp_path)
    counts = ga.create_visium_counts(dirs)
    with pytest.raises(ValueError, match="no slide for array sampleB"):
        ga.SlideCountDataset([slide], dirs[:1], counts, patch_size=8)
    with pytest.raises(ValueError, match=r"device=cuda:0, but the counts are on the host"):
        ga.SlideCountDataset([slide, slide], dirs, counts, patch_size=8, device='cuda:0')
    # two spots of the counts that the position file does not list in tissue
    obs = counts.obs.copy()
    k0, k1 = 2, int(counts._s.row_start[1]) - 1
    for k, xy in ((k0, (41, 1)), (k1, (43, 1))):
        obs.iloc[k, obs.columns.get_loc('x')], obs.iloc[k, obs.columns.get_loc('y')] = xy
    ptr, idx, val = (t.numpy() for t in counts._s.csr)
    X = sp.csr_matrix((val, idx, ptr), shape=(len(obs), counts.n_genes))
    moved = ga.SpotCounts(X, obs, list(counts.gene_ids))
    with pytest.raises(ValueError, match=r"2 spots of array sampleA are not in-tissue spots of .*tissue_positions.csv \(first: x 41, y 1\)"):
        ga.SlideCountDataset([slide, slide], dirs, moved, patch_size=8)
    with pytest.raises(ValueError, match="must match"):
        ga.SlideCountDataset([slide], dirs, counts, patch_size=8)


# ------------------------------------------------------------------------------------------------ the loop
def test_train_expression_equals_a_hand_written_loop(tmp_path, monkeypatch, capsys):
    ga, trees, dirs, slide = _slide_setup(tmp_path)
    from torch.utils.data import DataLoader
    monkeypatch.setattr(ga.training.gdist, 'default_device', lambda: CPU)           # the host path, also beside a GPU
    counts = ga.create_visium_counts(dirs)
    counts.normalize_total(1e4).log1p()
    scale = ga.SparseMSELoss.unit_scale(counts)
    P, G = 6, counts.n_genes
    sets = {'train': ga.SlideCountDataset([slide], dirs[:1], counts.subset_arrays(['sampleA']), patch_size=P, raw_uint8=False),
            'val': ga.SlideCountDataset([slide], dirs[1:], counts.subset_arrays(['sampleB']), patch_size=P, raw_uint8=False)}

    def loaders():
        gen = torch.Generator().manual_seed(5)
        return {'train': DataLoader(sets['train'], batch_size=4, shuffle=True, generator=gen),
                'val': DataLoader(sets['val'], batch_size=4)}

    torch.manual_seed(1)
    first = nn.Sequential(nn.Flatten(), nn.Linear(3 * P * P, G))
    epochs, lr = 6, 4.0                                                             # a step large enough that validation is not monotone

    # the hand-written loop: nn.MSELoss on dense targets
    dense = torch.from_numpy(_dense(counts)) * scale
    ref = copy.deepcopy(first)
    opt = torch.optim.SGD(ref.parameters(), lr=lr)
    mse, hist, best, best_wts = nn.MSELoss(), {'train': [], 'val': []}, float('inf'), None
    dl = loaders()
    for epoch in range(epochs):
        for phase in ('train', 'val'):
            ref.train(phase == 'train')
            running = 0.0
            for x, rows, _ in dl[phase]:
                opt.zero_grad()
                with torch.set_grad_enabled(phase == 'train'):
                    loss = mse(torch.sigmoid(ref(x)), dense[rows])
                    if phase == 'train':
                        loss.backward()
                        opt.step()
                running += loss.item()
            hist[phase].append(running / len(dl[phase]))
            if phase == 'val' and hist['val'][-1] < best:
                best, best_wts = hist['val'][-1], copy.deepcopy(ref.state_dict())

    model = copy.deepcopy(first)
    out = str(tmp_path / 'expr.pt')
    crit = ga.SparseMSELoss(counts, gene_scale=scale)
    model, vh, th = ga.train_expression(model, loaders(), crit, torch.optim.SGD(model.parameters(), lr=lr), num_epochs=epochs,
                                        outfile=out)
    text = capsys.readouterr().out
    assert vh == hist['val'] and th == hist['train'] and len(vh) == epochs
    assert int(np.argmin(vh)) != epochs - 1, vh                                     # the best epoch is not the last one
    for k, v in model.state_dict().items():
        assert torch.equal(v, best_wts[k]), k
    assert any(not torch.equal(v, ref.state_dict()[k]) for k, v in best_wts.items())            # ... nor the last weights
    saved = torch.load(out)
    assert all(torch.equal(saved[k], best_wts[k]) for k in best_wts)
    assert 'train Loss: %.4f' % th[0] in text and 'val Loss: %.4f' % vh[-1] in text and 'Best val loss' in text
    assert os.path.exists(out)


def test_new_names_are_declared_bound_and_exported():
    from gridnext_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = _lib.lib()
    assert _lib.PARAMS['gnx_sparse_line_max_f32'] == ['lineptr', 'idx', 'val', 'lines', 'n_lines', 'idx_mask', 'out', 'stream']
    assert len(_lib.SIGNATURES['gnx_sparse_line_max_f32'][1]) == 8 and hasattr(handle, 'gnx_sparse_line_max_f32')
    assert 'counts_from_img.ipynb' in open(_lib.HEADER_PATH).read()
    import gridnext_amd as ga
    assert ga.SparseMSELoss is ga.expression.SparseMSELoss and ga.ExpressionNet is ga.expression.ExpressionNet
    assert ga.SlideCountDataset is ga.multimodal_datasets.SlideCountDataset and ga.train_expression is ga.training.train_expression
