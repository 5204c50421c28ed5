"""numpy restatement of csrc/sparse_counts.hip and of the count tutorial's preprocessing, and the fixtures the sparse-count tests
share.  A matrix is (lineptr int64, idx int32, val float32): the rows of a CSR or the columns of a CSC matrix.  Nothing here
imports gridnext_amd: the tests compare the package (host path and device path) against this file."""
import gzip
import math
import os

import numpy as np

TARGET = 1e4


# ------------------------------------------------------------------------------------------------ the kernels
def expand(lineptr, idx, val, lines, n_lines, pos_of_idx, L, ld_out=None, fill=np.nan):
    """out[n_lines][ld_out]: positions [0, L) of row i hold line i's values (0 where no entry maps), the padding keeps `fill`."""
    ld_out = L if ld_out is None else ld_out
    out = np.full((n_lines, ld_out), fill, dtype=np.float32)
    for i in range(n_lines):
        out[i, :L] = 0.0
        line = i if lines is None else int(lines[i])
        for e in range(int(lineptr[line]), int(lineptr[line + 1])):
            p = int(idx[e]) if pos_of_idx is None else int(pos_of_idx[idx[e]])
            if 0 <= p < L:
                out[i, p] = val[e]
    return out


def line_entries(lineptr, idx, val, line, idx_mask=None):
    v = val[int(lineptr[line]):int(lineptr[line + 1])]
    if idx_mask is not None:
        v = v[idx_mask[idx[int(lineptr[line]):int(lineptr[line + 1])]] != 0]
    return v


def moments_fsum(lineptr, idx, val, lines, n_lines, idx_mask=None):
    """Per line: (fsum v, fsum v^2, entries, fsum |v|, fsum v^2 again as the scale of the squares' bound); v^2 exact in double."""
    rows = []
    for i in range(n_lines):
        v = line_entries(lineptr, idx, val, i if lines is None else int(lines[i]), idx_mask).astype(np.float64)
        rows.append((math.fsum(v), math.fsum(v * v), len(v), math.fsum(np.abs(v))))
    return rows


def moments_bound(n, scale):
    """Any summation order of n doubles: |error| <= (n - 1) u sum|v| + O(u^2), u = 2^-53; stated as n u sum|v|."""
    return n * 2.0 ** -53 * scale


def div_by_line(lineptr, val, divisor):
    return (val / np.repeat(divisor.astype(np.float32), np.diff(lineptr))).astype(np.float32)


def div_by_idx(idx, val, divisor):
    return (val / divisor.astype(np.float32)[idx]).astype(np.float32)


def ulps_of(got32, want64):
    """|got - want| in units of the float32 spacing at want (want: float64 of the exact function)."""
    want32 = np.abs(want64).astype(np.float32)
    return np.abs(got32.astype(np.float64) - want64) / np.spacing(np.maximum(want32, np.float32(2.0 ** -126))).astype(np.float64)


def log1p_bar(x32):
    """(bar, numpy's own error): 4 x the largest error, in ulps, of numpy's float32 log1p on these inputs."""
    own = float(ulps_of(np.log1p(x32), np.log1p(x32.astype(np.float64))).max())
    return 4.0 * own, own


# ------------------------------------------------------------------------------------------------ the tutorial
def normalise_log1p_dense(counts, target_sum=TARGET):
    """float32 (spots, genes): normalize_total then log1p as gridnext_amd/visium_datasets.py fixes the arithmetic."""
    S = counts.astype(np.float64).sum(1)
    d = np.where(S == 0, np.float32(1), S.astype(np.float32) / np.float32(target_sum)).astype(np.float32)
    x = counts.astype(np.float32) / d[:, None]
    return np.log1p(x).astype(np.float32), x


def tutorial_scores(x):
    """float64 (mean, std, |mean / std|) per gene of a dense float32 matrix: the tutorial's X.mean(0), X.std(0)."""
    x = x.astype(np.float64)
    mean, std = x.mean(0), x.std(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        score = np.abs(mean / std)
    return mean, std, np.where(np.isfinite(score), score, -np.inf)


def top_genes(score, k):
    """Indices of the k largest scores, largest first (ties by index)."""
    return np.argsort(-score, kind='stable')[:k]


# ------------------------------------------------------------------------------------------------ fixtures
def random_lines(rng, lengths, n_idx, integer=True):
    """A matrix whose line l has lengths[l] entries with sorted distinct indices below n_idx."""
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(n_idx, size=n, replace=False)) for n in lengths] + [np.zeros(0, np.int64)])
    n = int(ptr[-1])
    val = rng.integers(1, 200, size=n).astype(np.float32) if integer else rng.random(n).astype(np.float32) * 9 + 0.01
    return ptr, idx.astype(np.int32), val


def synthetic_arrays(seed=0, n_arrays=3, n_genes=300, h=78, w=64, n_spots=200, n_classes=4, density=0.25):
    """(X scipy csr spots x genes of integer counts, obs DataFrame, gene ids): `n_arrays` arrays of about n_spots spots on
    distinct cells of an h x w Visium grid, annotations 'c0' .. ; genes differ in level and in how often they are seen."""
    import pandas as pd
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    level = rng.gamma(2.0, 3.0, size=n_genes) + 0.5
    seen = np.clip(rng.beta(2, 4, size=n_genes) * 4 * density, 0.02, 0.95)
    blocks, frames = [], []
    for a in range(n_arrays):
        cells = rng.choice(h * w, size=n_spots + a, replace=False)
        rows, cols = cells // w, cells % w
        on = rng.random((len(cells), n_genes)) < seen
        counts = (rng.poisson(level, size=on.shape) + 1) * on
        blocks.append(sp.csr_matrix(counts.astype(np.float64)))
        frames.append(pd.DataFrame({'x': 2 * cols + rows % 2, 'y': rows, 'array': 'arr%d' % a,
                                    'annotation': ['c%d' % k for k in rng.integers(0, n_classes, len(cells))]},
                                   index=['arr%d_%d_%d' % (a, x, y) for x, y in zip(2 * cols + rows % 2, rows)]))
    return sp.vstack(blocks, format='csr'), pd.concat(frames), ['ENSG%05d' % g for g in range(n_genes)]


def write_spaceranger_tree(root, name, seed, genes, n_rows=6, n_cols=5, header=True, nested=True):
    """A Spaceranger-like output directory root/name: [outs/]filtered_feature_bc_matrix/{matrix.mtx.gz, features.tsv.gz,
    barcodes.tsv.gz} and [outs/]spatial/tissue_positions.csv (header=True, Spaceranger >= 2) or tissue_positions_list.csv
    (headerless).  Every cell of the n_rows x n_cols odd-right grid is a barcode, about 70 % in tissue; the matrix lists the
    in-tissue barcodes in shuffled order.  Returns (dir, dense genes x barcodes int matrix, barcodes of the matrix, positions
    rows [(barcode, in_tissue, row, col, pxl_row, pxl_col)])."""
    import scipy.io
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    base = os.path.join(str(root), name)
    top = os.path.join(base, 'outs') if nested else base
    os.makedirs(os.path.join(top, 'filtered_feature_bc_matrix'))
    os.makedirs(os.path.join(top, 'spatial'))
    positions = []
    for r in range(n_rows):
        for c in range(n_cols):
            col = 2 * c + r % 2
            positions.append(('BC%s%02d%02d-1' % (name[-1], r, col), int(rng.random() < 0.7), r, col, 100 * r + 7, 50 * col + 3))
    inside = [p[0] for p in positions if p[1]]
    barcodes = [inside[k] for k in rng.permutation(len(inside))]
    dense = rng.poisson(1.2, size=(len(genes), len(barcodes))) * (rng.random((len(genes), len(barcodes))) < 0.5)
    mtx = os.path.join(top, 'filtered_feature_bc_matrix', 'matrix.mtx')
    scipy.io.mmwrite(mtx, sp.coo_matrix(dense.astype(np.int64)), field='integer')
    with open(mtx, 'rb') as src, gzip.open(mtx + '.gz', 'wb') as dst:
        dst.write(src.read())
    os.remove(mtx)
    with gzip.open(os.path.join(top, 'filtered_feature_bc_matrix', 'features.tsv.gz'), 'wt') as fh:
        for g in genes:
            fh.write('%s\tSYM_%s\tGene Expression\n' % (g, g))
    with gzip.open(os.path.join(top, 'filtered_feature_bc_matrix', 'barcodes.tsv.gz'), 'wt') as fh:
        fh.write(''.join(b + '\n' for b in barcodes))
    pfile = os.path.join(top, 'spatial', 'tissue_positions.csv' if header else 'tissue_positions_list.csv')
    with open(pfile, 'w') as fh:
        if header:
            fh.write('barcode,in_tissue,array_row,array_col,pxl_row_in_fullres,pxl_col_in_fullres\n')
        for p in positions:
            fh.write('%s,%d,%d,%d,%d,%d\n' % p)
    return base, dense, barcodes, positions


TREES = (dict(name='sampleA', seed=11, genes=['ENSG%03d' % g for g in (1, 2, 3, 5, 8, 13)], header=True, nested=True),
         dict(name='sampleB', seed=12, genes=['ENSG%03d' % g for g in (2, 3, 4, 8, 21)], header=False, nested=False))
