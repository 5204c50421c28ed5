"""Sparse counts on the host: the numpy restatement (tests/sparse_counts_ref.py) against scipy and numpy, the Spaceranger
readers against the reference's recorded output (tests/golden/visium_count_readers.npz, tools/gen_golden_counts.py),
`create_visium_counts` / `SpotCounts` / the two datasets on their host path against the restatement and against the dense
`CountDataset` / `CountGridDataset`, the refusals, and `to_loupe_annots`.  No GPU."""
import os
import types

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import sparse_counts_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'visium_count_readers.npz')


def _csr(rng, n, m, density=0.3):
    dense = rng.integers(1, 50, size=(n, m)) * (rng.random((n, m)) < density)
    mat = sp.csr_matrix(dense.astype(np.float32))
    mat.sort_indices()
    return dense.astype(np.float32), mat


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_expand_is_scipys_toarray():
    rng = np.random.default_rng(0)
    dense, mat = _csr(rng, 9, 70)
    ptr, idx, val = mat.indptr.astype(np.int64), mat.indices.astype(np.int32), mat.data
    assert np.array_equal(R.expand(ptr, idx, val, None, 9, None, 70), mat.toarray())
    lines = np.array([8, 8, 0, 3], dtype=np.int32)
    perm = rng.permutation(70).astype(np.int32)
    want = np.zeros((4, 70), dtype=np.float32)
    want[:, perm] = dense[lines]
    assert np.array_equal(R.expand(ptr, idx, val, lines, 4, perm, 70), want)
    kept = np.arange(70) % 3 != 0
    drop = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int32)                # injective where >= 0: 46 positions
    got = R.expand(ptr, idx, val, None, 9, drop, 50, ld_out=53)
    assert np.isnan(got[:, 50:]).all() and not np.isnan(got[:, :50]).any()
    keep = drop >= 0
    assert np.array_equal(got[:, drop[keep]], dense[:, keep]) and got[:, :50].sum() == dense[:, keep].sum()
    csc = mat.tocsc()
    csc.sort_indices()
    assert np.array_equal(R.expand(csc.indptr, csc.indices, csc.data, None, 70, None, 9), mat.toarray().T)


def test_restated_moments_and_divisions_are_numpys():
    rng = np.random.default_rng(1)
    dense, mat = _csr(rng, 40, 30)
    x = np.log1p(dense / 7).astype(np.float32)
    m = sp.csc_matrix(x)
    m.sort_indices()
    rows = R.moments_fsum(m.indptr, m.indices, m.data, None, 30)
    s1, s2 = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    x64 = x.astype(np.float64)
    assert np.allclose(s1 / 40, np.mean(x64, 0), rtol=1e-14, atol=0) and \
        np.allclose(np.sqrt(s2 / 40 - (s1 / 40) ** 2), np.std(x64, 0), rtol=1e-12, atol=0)
    mask = (np.arange(40) % 2).astype(np.uint8)
    rows = R.moments_fsum(m.indptr, m.indices, m.data, None, 30, mask)
    assert np.allclose([r[0] for r in rows], x64[1::2].sum(0), rtol=1e-14)
    d = rng.integers(1, 9, 40).astype(np.float32)
    assert np.array_equal(sp.csr_matrix((R.div_by_line(mat.indptr, mat.data, d), mat.indices, mat.indptr), (40, 30)).toarray(),
                          dense / d[:, None])
    c = mat.tocsc()
    assert np.array_equal(sp.csc_matrix((R.div_by_idx(c.indices, c.data, d), c.indices, c.indptr), (40, 30)).toarray(),
                          dense / d[:, None])
    bar, own = R.log1p_bar(x[x > 0])
    assert 0 < own <= 2.0 and bar == 4 * own                 # numpy's float32 log1p is good to about 1.5 ulp


def test_restated_tutorial_selection():
    X, obs, genes = R.synthetic_arrays()
    y, x = R.normalise_log1p_dense(X.toarray())
    assert np.allclose(x.sum(1), R.TARGET, rtol=1e-5) and y.dtype == np.float32
    mean, std, score = R.tutorial_scores(y)
    top = R.top_genes(score, 64)
    assert len(set(top)) == 64 and score[top].min() >= np.delete(score, top).max()


# ------------------------------------------------------------------------------------------------ readers, create_visium_counts
def _trees(tmp_path):
    return [R.write_spaceranger_tree(tmp_path, **spec) for spec in R.TREES]


def test_readers_return_what_the_reference_recorded(tmp_path):
    from gridnext_amd import visium_datasets as V
    gold = np.load(GOLDEN)
    for k, (srd, dense, barcodes, _) in enumerate(_trees(tmp_path)):
        found = V.find_feature_matrix_files(srd)
        assert [os.path.relpath(found[key], srd) for key in ('matrix', 'features', 'barcodes')] == list(gold['found_%d' % k])
        frame = V.read_feature_matrix(srd)
        assert all(isinstance(t, pd.SparseDtype) for t in frame.dtypes)
        assert list(frame.index) == list(gold['genes_%d' % k]) and list(frame.columns) == list(gold['barcodes_%d' % k])
        assert np.array_equal(frame.sparse.to_dense().values, gold['matrix_%d' % k])
        assert np.array_equal(gold['matrix_%d' % k], dense) and list(frame.columns) == barcodes      # and what was written
        names = V.read_feature_names(srd)
        assert list(names.index) == list(gold['names_index_%d' % k])
        assert list(names['gene_symbol']) == list(gold['names_symbol_%d' % k])
        assert V.read_feature_matrix(None, individual_files=found).equals(frame)
    with pytest.raises(NotImplementedError):
        V.find_feature_matrix_files(srd, hd_binning='square_008um')
    with pytest.raises(NotImplementedError):
        V.read_feature_matrix(srd, hd_binning='square_008um')
    with pytest.raises(ValueError, match="matrix files"):
        V.find_feature_matrix_files(str(tmp_path / 'nothing_here'))


def _write_annots(tmp_path, trees, every=5):
    """Loupe CSVs: every in-tissue barcode but each `every`-th gets a label; one extra row for a barcode outside the tissue."""
    files = []
    for k, (srd, _, _, positions) in enumerate(trees):
        inside = [p[0] for p in positions if p[1]]
        outside = [p[0] for p in positions if not p[1]]
        rows = [(b, ('WM', 'Layer1', 'Layer2')[j % 3]) for j, b in enumerate(inside) if j % every != every - 1]
        path = str(tmp_path / ('annot%d.csv' % k))
        pd.DataFrame(rows + [(outside[0], 'WM')], columns=['Barcode', 'AARs']).to_csv(path, index=False)
        files.append(path)
    return files


def _expected(trees, annotated=None):
    """Dense (spots, union genes), obs rows and names as create_visium_counts should build them, from what was written."""
    genes = sorted(set().union(*[spec['genes'] for spec in R.TREES]))
    blocks, rows = [], []
    for k, (srd, dense, barcodes, positions) in enumerate(trees):
        col = {b: j for j, b in enumerate(barcodes)}
        for b, inside, r, c, pr, pc in positions:
            if inside and (annotated is None or b in annotated[k]):
                vec = np.zeros(len(genes))
                vec[[genes.index(g) for g in R.TREES[k]['genes']]] = dense[:, col[b]]
                blocks.append(vec)
                rows.append((c, r, pc, pr, R.TREES[k]['name'], None if annotated is None else annotated[k][b]))
    return np.array(blocks), rows, genes


def test_create_visium_counts_on_a_spaceranger_tree(tmp_path):
    import gridnext_amd as ga
    trees = _trees(tmp_path)
    dirs = [t[0] for t in trees]
    counts = ga.create_visium_counts(dirs)
    want, rows, genes = _expected(trees)
    assert counts.device is None and counts.arrays == ['sampleA', 'sampleB']
    assert list(counts.gene_ids) == genes and list(counts.gene_symbols) == ['SYM_' + g for g in genes]
    assert list(counts.obs.columns) == ['x', 'y', 'x_px', 'y_px', 'array', 'annotation']
    assert [tuple(r)[:5] for r in counts.obs.itertuples(index=False)] == [r[:5] for r in rows]
    assert list(counts.obs.index) == ['%s_%d_%d' % (r[4], r[0], r[1]) for r in rows]
    s = counts._s
    assert (s.csr[0].dtype, s.csr[1].dtype, s.csr[2].dtype) == (torch.int64, torch.int32, torch.float32)
    assert all((p.dtype, i.dtype, v.dtype) == (torch.int64, torch.int32, torch.float32) for p, i, v in s.csc)
    got = sp.csr_matrix((s.csr[2].numpy(), s.csr[1].numpy(), s.csr[0].numpy()), shape=want.shape).toarray()
    assert np.array_equal(got, want)
    for a in range(2):
        r0, r1 = s.row_start[a], s.row_start[a + 1]
        p, i, v = (t.numpy() for t in s.csc[a])
        assert np.array_equal(sp.csc_matrix((v, i, p), shape=(r1 - r0, len(genes))).toarray(), want[r0:r1])
    # with annotations: the in-tissue spots that have one, and their labels
    files = _write_annots(tmp_path, trees)
    annotated = [dict(pd.read_csv(f).values.tolist()) for f in files]
    counts = ga.create_visium_counts(dirs, files)
    want, rows, _ = _expected(trees, annotated)
    assert counts.n_spots == len(rows) < ga.create_visium_counts(dirs).n_spots
    assert list(counts.obs['annotation']) == [r[5] for r in rows]
    vecs = torch.stack([v for v, _ in ga.SparseCountDataset(counts)])
    assert np.array_equal(vecs.numpy(), want)


def test_from_anndata_on_a_duck_object():
    import gridnext_amd as ga
    X, obs, genes = R.synthetic_arrays(n_arrays=2, n_genes=40, n_spots=30)
    order = np.random.default_rng(3).permutation(X.shape[0])                    # arrays interleaved: sorted at construction
    duck = types.SimpleNamespace(X=X[order], obs=obs.iloc[order].rename(columns={'array': 'slide', 'annotation': 'aar'}),
                                 var=pd.DataFrame({'gene_symbol': ['S%d' % g for g in range(40)]}, index=genes))
    counts = ga.SpotCounts.from_anndata(duck, obs_arr='slide', obs_label='aar')
    assert counts.arrays == list(pd.unique(duck.obs['slide'])) and list(counts.gene_symbols) == ['S%d' % g for g in range(40)]
    back = {name: k for k, name in enumerate(obs.index)}
    rows = [back[n] for n in counts.obs.index]
    assert list(counts.obs['array']) == sorted(counts.obs['array'], key=counts.arrays.index)
    ds = ga.SparseCountDataset(counts)
    assert np.array_equal(torch.stack([v for v, _ in ds]).numpy(), X.toarray()[rows])
    assert [ds.classes[int(l)] for _, l in ds] == list(obs['annotation'].values[rows])
    dense = ga.SpotCounts.from_anndata(types.SimpleNamespace(X=X.toarray(), obs=obs, var=pd.DataFrame(index=genes)))
    assert torch.equal(dense._s.csr[2], ga.SpotCounts(X, obs, genes)._s.csr[2]) and list(dense.gene_symbols) == genes


def test_refusals():
    import gridnext_amd as ga
    X, obs, genes = R.synthetic_arrays(n_arrays=1, n_genes=20, n_spots=12)
    for bad, what in ((0.5, "integers"), (-1.0, "integers"), (2.0 ** 24, "2\\^24"), (np.nan, "integers")):
        Y = X.copy().tolil()
        Y[3, 4] = bad
        with pytest.raises(ValueError, match=what):
            ga.SpotCounts(Y.tocsr(), obs, genes)
    ga.SpotCounts(sp.csr_matrix(np.full((len(obs), 20), 2.0 ** 24 - 1)), obs, genes)
    with pytest.raises(ValueError, match="spots"):
        ga.SpotCounts(X[:5], obs, genes)
    fake = types.SimpleNamespace(nnz=2 ** 31, indptr=np.zeros(1), indices=np.zeros(0), data=np.zeros(0))
    from gridnext_amd import visium_datasets as V
    with pytest.raises(ValueError, match="2\\^31"):
        V._trio(fake)
    counts = ga.SpotCounts(X, obs, genes)
    with pytest.raises(ValueError, match="twice"):
        counts.subset_genes([genes[1], genes[1]])
    with pytest.raises(ValueError, match="not among"):
        counts.subset_genes(['nope'])
    with pytest.raises(ValueError, match="no array"):
        counts.subset_arrays(['nope'])
    with pytest.raises(ValueError, match="one position"):
        V._check_injective(np.array([0, 3, -1, -1, 3]), "map")
    # a spot outside the grid, two spots on one cell: before anything is expanded
    far = obs.copy()
    far.iloc[0, far.columns.get_loc('y')] = 78
    with pytest.raises(ValueError, match="outside"):
        ga.SparseCountGridDataset(ga.SpotCounts(X, far, genes))[0]
    twice = obs.copy()
    twice.iloc[1, :2] = twice.iloc[0, :2].values
    with pytest.raises(ValueError, match="one position"):
        ga.SparseCountGridDataset(ga.SpotCounts(X, twice, genes))[0]


# ------------------------------------------------------------------------------------------------ transforms and moments
def test_host_transforms_moments_and_views_against_the_restatement():
    import gridnext_amd as ga
    X, obs, genes = R.synthetic_arrays()
    dense = X.toarray()
    counts = ga.SpotCounts(X, obs, genes)
    assert np.array_equal(counts.detection_rate().numpy(), (dense > 0).mean(0))
    assert np.array_equal(counts.spot_totals().numpy(), dense.sum(1))
    mean, std = counts.gene_moments()
    assert mean.dtype == torch.float64 and np.allclose(mean.numpy(), dense.mean(0), rtol=1e-13) and \
        np.allclose(std.numpy(), dense.std(0), rtol=1e-11)
    assert counts.normalize_total(1e4) is counts and counts.log1p() is counts
    want, _ = R.normalise_log1p_dense(dense)
    ds = ga.SparseCountDataset(counts)
    assert torch.equal(torch.stack([v for v, _ in ds]), torch.from_numpy(want))                      # the CSR
    grids = ga.SparseCountGridDataset(counts)
    for k in range(3):                                                                               # every CSC: the same bits
        x, y = grids[k]
        rows = np.flatnonzero(obs['array'].values == 'arr%d' % k)
        assert x.shape == (300, 78, 64) and y.shape == (78, 64) and x.dtype == torch.float32 and y.dtype == torch.int64
        for r in rows[::17]:
            col, row = (obs['x'].values[r] - obs['y'].values[r] % 2) // 2, obs['y'].values[r]
            assert torch.equal(x[:, row, col], torch.from_numpy(want[r]))
            assert y[row, col] == 1 + list(grids.classes).index(obs['annotation'].values[r])
        assert int((y > 0).sum()) == len(rows) and float(x.sum(dtype=torch.float64)) == float(want[rows].sum(dtype=np.float64))
    mean, std = counts.gene_moments()
    rmean, rstd, score = R.tutorial_scores(want)
    assert np.allclose(mean.numpy(), rmean, rtol=1e-12) and np.allclose(std.numpy(), rstd, rtol=1e-10)
    top = R.top_genes(score, 64)
    with np.errstate(divide='ignore', invalid='ignore'):
        mine = np.abs(mean.numpy() / std.numpy())
    assert np.array_equal(R.top_genes(np.where(np.isfinite(mine), mine, -np.inf), 64), top)
    # views: maps over the same storage
    view = counts.subset_genes([genes[g] for g in top])
    assert view.n_genes == 64 and list(view.gene_ids) == [genes[g] for g in top] and view._s is counts._s
    assert torch.equal(torch.stack([v for v, _ in ga.SparseCountDataset(view)]), torch.from_numpy(want[:, top]))
    assert torch.equal(view.subset_genes(np.arange(64) % 2 == 0).gene_moments()[0], mean[top[::2]])
    val = view.subset_arrays(['arr2'])
    assert val.arrays == ['arr2'] and val.n_spots == int((obs['array'] == 'arr2').sum())
    x, y = ga.SparseCountGridDataset(val, classes=grids.classes)[0]
    assert torch.equal(x, grids[2][0][torch.from_numpy(top)]) and torch.equal(y, grids[2][1])
    m2, s2 = view.gene_moments(arrays=['arr0', 'arr1'])
    sub = want[obs['array'].values != 'arr2'][:, top].astype(np.float64)
    assert np.allclose(m2.numpy(), sub.mean(0), rtol=1e-12) and np.allclose(s2.numpy(), sub.std(0), rtol=1e-10)
    # the total over the selected genes only
    part = ga.SpotCounts(X, obs, genes).subset_genes(genes[:50])
    part.normalize_total(100.0)
    got = torch.stack([v for v, _ in ga.SparseCountDataset(part)]).numpy()
    S = dense[:, :50].sum(1)
    d = np.where(S == 0, np.float32(1), S.astype(np.float32) / np.float32(100.0)).astype(np.float32)
    assert np.array_equal(got, dense[:, :50].astype(np.float32) / d[:, None])


# ------------------------------------------------------------------------------------------------ against the dense datasets
def test_host_datasets_equal_the_dense_count_datasets(tmp_path):
    """Raw counts: SparseCountGridDataset / SparseCountDataset over create_visium_counts == CountGridDataset / CountDataset over
    the equivalent unified TSVs (genes x in-tissue spots, "col_row" headers), the same Loupe and position files."""
    import gridnext_amd as ga
    from gridnext_amd.imgprocess import visium_find_position_file
    trees = _trees(tmp_path)
    dirs = [t[0] for t in trees]
    annots = _write_annots(tmp_path, trees)
    full, rows, genes = _expected(trees)
    tsvs, at = [], 0
    for k, (srd, _, _, positions) in enumerate(trees):
        mine = [r for r in rows if r[4] == R.TREES[k]['name']]
        block = full[at:at + len(mine)]
        at += len(mine)
        frame = pd.DataFrame(block.T.astype(int), index=genes, columns=['%d_%d' % (r[0], r[1]) for r in mine])
        tsvs.append(str(tmp_path / ('unified%d.tsv' % k)))
        frame.to_csv(tsvs[-1], sep='\t')
    pfiles = [visium_find_position_file(d) for d in dirs]
    counts = ga.create_visium_counts(dirs, annots)
    dense_grid = ga.CountGridDataset(tsvs, annots, pfiles, h_st=6, w_st=5)
    grid = ga.SparseCountGridDataset(counts, h_st=6, w_st=5)
    assert len(grid) == len(dense_grid) == 2 and list(grid.classes) == list(dense_grid.classes) == ['Layer1', 'Layer2', 'WM']
    for k in range(2):
        (x0, y0), (x1, y1) = dense_grid[k], grid[k]
        assert torch.equal(x0, x1) and torch.equal(y0, y1) and x1.dtype == torch.float32 and y1.dtype == torch.int64
    dense_spots = ga.CountDataset(tsvs, annots, pfiles)
    spots = ga.SparseCountDataset(counts)
    assert len(spots) == len(dense_spots) > 20 and list(spots.classes) == list(dense_spots.classes)
    for k in range(len(spots)):
        (x0, y0), (x1, y1) = dense_spots[k], spots[k]
        assert torch.equal(x0, x1) and torch.equal(y0, y1) and y1.dtype == torch.int64
    batch = spots.__getitems__([5, 0, 5, len(spots) - 1])
    assert all(torch.equal(batch[j][0], spots[k][0]) for j, k in enumerate([5, 0, 5, len(spots) - 1]))
    from torch.utils.data import DataLoader
    xb, yb = next(iter(DataLoader(spots, batch_size=7)))
    assert xb.shape == (7, len(genes)) and torch.equal(xb[3], spots[3][0]) and yb.tolist() == [int(spots[k][1]) for k in range(7)]


def test_to_loupe_annots_round_trip(tmp_path):
    from gridnext_amd.count_datasets import read_annotfile
    from gridnext_amd.imgprocess import visium_find_position_file
    from gridnext_amd.utils import pseudo_hex_to_oddr, to_loupe_annots
    for srd, _, _, positions in _trees(tmp_path):
        pfile = visium_find_position_file(srd)
        grid = torch.from_numpy(np.random.default_rng(5).integers(0, 4, size=(1, 6, 5)))
        names = ['Layer1', 'Layer2', 'WM']
        out = str(tmp_path / 'loupe.csv')
        to_loupe_annots(grid, pfile, out, annot_names=names)
        table = pd.read_csv(out, keep_default_na=False)
        inside = [p for p in positions if p[1]]
        assert list(table.columns) == ['Barcode', 'AARs'] and list(table['Barcode']) == [p[0] for p in inside]
        coords, labels = read_annotfile(out, position_file=pfile)
        want = {}
        for b, _, r, c, _, _ in inside:
            x, y = pseudo_hex_to_oddr(c, r)
            if grid[0, y, x] > 0:
                want['%d_%d' % (c, r)] = names[int(grid[0, y, x]) - 1]
        assert dict(zip(coords, labels)) == want and len(want) > 5
        to_loupe_annots(grid[0], pfile, out, zero_bg=False)                       # integers, no background
        assert list(pd.read_csv(out)['AARs']) == [int(grid[0][pseudo_hex_to_oddr(p[3], p[2])[::-1]]) for p in inside]


def test_new_symbols_are_declared_bound_and_exported():
    from gridnext_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = _lib.lib()
    for name, nargs in (('gnx_sparse_expand_f32', 10), ('gnx_sparse_line_moments_f64', 8), ('gnx_sparse_div_by_line_f32', 5),
                        ('gnx_sparse_div_by_idx_f32', 5), ('gnx_log1p_f32', 3), ('gnx_sparse_expand_chunk', 0)):
        assert name in _lib.PARAMS, "%s is not declared in the header" % name
        assert len(_lib.PARAMS[name]) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(handle, name)
    assert _lib.PARAMS['gnx_sparse_expand_f32'] == ['lineptr', 'idx', 'val', 'lines', 'n_lines', 'pos_of_idx', 'out', 'ld_out',
                                                    'L', 'stream']
    assert _lib.query('gnx_sparse_expand_chunk') == 8192
    assert 'count_datasets.py:347-376' in text and 'utils.py:197-217' in text and 'visium_datasets.py:221-272' in text
    import gridnext_amd as ga
    assert ga.SpotCounts is ga.visium_datasets.SpotCounts and callable(ga.create_visium_counts)
    assert ga.SparseCountDataset is ga.visium_datasets.SparseCountDataset
    assert ga.SparseCountGridDataset is ga.visium_datasets.SparseCountGridDataset
