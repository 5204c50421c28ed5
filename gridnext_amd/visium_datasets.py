"""Sparse Spaceranger counts, resident on the device (API surface of the reference's gridnext/visium_datasets.py, "small
dataset" path of notebooks/Tutorial_visium_count.ipynb).

The reference reads Spaceranger's matrix.mtx.gz into an AnnData (`create_visium_anndata`, :221-272), runs scanpy's
`normalize_total` and `log1p` on it, keeps the genes with the largest |mean / std| and densifies everything on the host
(`anndata_to_tensordataset`, count_datasets.py:347-376; `anndata_to_grids`, utils.py:197-217).  Here the counts stay sparse:
`SpotCounts` holds one CSR over all spots (sorted by array) and one CSC per array - fp32 values, int32 indices, int64 line
pointers - and after `.to(device)` the transforms, the moments and the densifying of every item are launches of
csrc/sparse_counts.hip.  On the host (device None) every method runs a numpy restatement of the same arithmetic.

Arithmetic, fixed here (scanpy is not a dependency and is not pinned by any test):
    S = the spot's total over the currently selected genes, exact in double (raw counts are integers below 2^24);
    d = float32(S) / float32(target_sum), d = 1 where S == 0;      x = float32(c) / d;      then log1pf(x).
scanpy sums in float32, which is the same number while S < 2^24.  Per-gene moments are per-array partial sums (double),
added on the host in array order: mean = S1 / N, var = S2 / N - mean^2 clamped at 0 (zeros included, population std: the
tutorial's X.mean(0) and X.std(0)).

anndata is never imported: `SpotCounts.from_anndata` reads `.X`, `.obs` and `.var` of whatever it is handed.
"""
import csv
import glob
import gzip
from pathlib import Path

import numpy as np
import pandas as pd
import torch
import torch.nn as nn
from torch.utils.data import Dataset

from . import _lib as L
from .imgprocess import visium_get_positions
from .utils import pseudo_hex_to_oddr

_I32, _I64, _F32 = torch.int32, torch.int64, torch.float32


# ---------------------------------------------------------------------------------------------- readers (host)
def find_feature_matrix_files(spaceranger_dir, hd_binning=None):
    """{'matrix', 'features', 'barcodes'} -> the first path under `spaceranger_dir` (any depth) that contains matrix.mtx.gz,
    features.tsv.gz, barcodes.tsv.gz (reference utils.py:290-313)."""
    if hd_binning is not None:
        raise NotImplementedError("Visium HD binned outputs are not implemented")
    existing = glob.glob(str(spaceranger_dir) + '/**', recursive=True)
    found = {}
    for key, name in (("matrix", "matrix.mtx.gz"), ("features", "features.tsv.gz"), ("barcodes", "barcodes.tsv.gz")):
        for path in existing:
            if name in path:
                found[key] = path
                break
    if len(found) == 3:
        return found
    raise ValueError("Cannot locate matrix files for %s" % spaceranger_dir)


def _first_column(path):
    with gzip.open(path, "rt") as fh:
        return [row[0] for row in csv.reader(fh, delimiter="\t")]


def _read_matrix(srd, individual_files=None, hd_binning=None):
    import scipy.io
    files = find_feature_matrix_files(srd, hd_binning) if individual_files is None else individual_files
    mat = scipy.io.mmread(files["matrix"])
    return mat, _first_column(files["features"]), _first_column(files["barcodes"])


def read_feature_matrix(srd, individual_files=None, hd_binning=None):
    """The result of a Spaceranger run as a (genes, spots) sparse DataFrame (reference visium_datasets.py:178-205)."""
    mat, feature_ids, barcodes = _read_matrix(srd, individual_files, hd_binning)
    return pd.DataFrame.sparse.from_spmatrix(mat, index=feature_ids, columns=barcodes)


def read_feature_names(srd, individual_files=None, hd_binning=None):
    """DataFrame ENSEMBL -> gene_symbol of every gene Spaceranger lists (reference visium_datasets.py:209-217)."""
    files = find_feature_matrix_files(srd, hd_binning) if individual_files is None else individual_files
    return pd.read_csv(files["features"], header=None, index_col=0, sep='\t', names=['ENSEMBL', 'gene_symbol'],
                       usecols=[0, 1])


def create_visium_counts(spaceranger_dirs, annot_files=None):
    """What `create_visium_anndata` (reference visium_datasets.py:221-272) builds, as a `SpotCounts` on the host: per array the
    in-tissue spots (intersected with the annotated ones when Loupe files are given, in the position file's order), obs
    columns x, y, x_px, y_px, array, annotation, the outer join of the arrays' gene lists (the common order when they are
    equal, else the sorted union, as pandas' Index.union gives it; a gene an array does not list counts zero there), gene ids
    and symbols.  The array's name is the directory's stem."""
    import scipy.sparse as sp
    per_array, obs_frames, symbols = [], [], {}
    for i, srd in enumerate(spaceranger_dirs):
        mat, gene_ids, barcodes = _read_matrix(srd)
        pos = visium_get_positions(srd)
        names = read_feature_names(srd)
        keep = pos[pos['in_tissue'] == 1].index
        annot = None
        if annot_files is not None:
            annot = pd.read_csv(annot_files[i], header=0, index_col=0, sep=',')
            annot = annot.loc[annot.iloc[:, 0] != '']
            annot = annot.loc[~annot.iloc[:, 0].isna()]
            keep = keep.intersection(annot.index)
        column = {b: k for k, b in enumerate(barcodes)}
        missing = [b for b in keep if b not in column]
        if missing:
            raise ValueError("%s: %d in-tissue barcodes are not in barcodes.tsv.gz (first: %s)" % (srd, len(missing), missing[0]))
        arr = Path(str(srd)).stem
        obs = pd.DataFrame({'x': pos.loc[keep, 'array_col'].values, 'y': pos.loc[keep, 'array_row'].values,
                            'x_px': pos.loc[keep, 'pxl_col_in_fullres'].values,
                            'y_px': pos.loc[keep, 'pxl_row_in_fullres'].values, 'array': arr})
        obs['annotation'] = annot.loc[keep].iloc[:, 0].values if annot is not None else None
        obs.index = ['%s_%d_%d' % (arr, x, y) for x, y in zip(obs['x'].values, obs['y'].values)]
        spots_by_genes = sp.csc_matrix(mat)[:, [column[b] for b in keep]].T.tocsr()
        per_array.append((spots_by_genes, list(gene_ids)))
        obs_frames.append(obs)
        for g in gene_ids:
            symbols.setdefault(g, names.loc[g, 'gene_symbol'] if g in names.index else g)
    all_ids = per_array[0][1]
    if any(ids != all_ids for _, ids in per_array[1:]):
        all_ids = sorted(set().union(*[ids for _, ids in per_array]))
    where = {g: k for k, g in enumerate(all_ids)}
    blocks = []
    for m, ids in per_array:
        coo = m.tocoo()
        cols = np.array([where[g] for g in ids], dtype=np.int64)[coo.col]
        blocks.append(sp.csr_matrix((coo.data, (coo.row, cols)), shape=(m.shape[0], len(all_ids))))
    return SpotCounts(sp.vstack(blocks, format='csr'), pd.concat(obs_frames, axis=0), all_ids, [symbols[g] for g in all_ids])


# ---------------------------------------------------------------------------------------------- storage
class _Store:
    """The shared, resident part of a SpotCounts and its views: csr = (ptr, idx, val) over all spots, csc[a] the same per
    array (idx = the spot's row within the array), torch tensors on `device` (None: CPU tensors over numpy memory).  `raw`: the
    stored values are still the counts; an in-place transform clears it and leaves its name in `transformed_by`."""

    def __init__(self, csr, csc, row_start, array_names, obs, gene_ids, gene_symbols, device=None, raw=True, transformed_by=None):
        self.csr, self.csc, self.row_start, self.array_names = csr, csc, row_start, array_names
        self.obs, self.gene_ids, self.gene_symbols, self.device = obs, gene_ids, gene_symbols, device
        self.csr_ptr_host = None             # the CSR's line pointers as a numpy array, copied back on first use
        self.raw, self.transformed_by = raw, transformed_by

    def rewritten_by(self, transform):
        self.raw, self.transformed_by = False, transform

    def nbytes(self):
        return sum(t.numel() * t.element_size() for trio in [self.csr] + self.csc for t in trio)


def _trio(m):
    """(int64 line pointers, int32 indices, fp32 values) of a scipy CSR / CSC matrix with sorted indices."""
    if m.nnz >= 2 ** 31:
        raise ValueError("a matrix of %d entries cannot be indexed: an array must have fewer than 2^31 entries" % m.nnz)
    return (torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int32)),
            torch.from_numpy(m.data.astype(np.float32)))


def _check_injective(pos, what):
    """A position map is injective on its non-negative values: two entries of a line on one position would race."""
    used = pos[pos >= 0]
    if len(np.unique(used)) != len(used):
        raise ValueError("%s: two indices map to one position" % what)


def same_device(a, b):
    """Whether two places - None (the host) or whatever torch.device takes - are one device; no index is index 0."""
    a, b = (torch.device('cpu' if d is None else d) for d in (a, b))
    return a.type == b.type and (a.index or 0) == (b.index or 0)


def trio_ptrs(trio):
    """The three leading pointers of every sparse launch: lineptr (int64), idx (int32), val (fp32)."""
    return L.ptr(trio[0], _I64), L.ptr(trio[1], _I32), L.ptr(trio[2])


def expand(trio, lines, n_lines, pos_of_idx, out, L_pos):
    """`gnx_sparse_expand_f32` on the current stream (out on a HIP device: the trio, the lists and maps live there too), or its
    numpy restatement into a CPU tensor.  out: 2-D float32 with unit stride along positions; lines / pos_of_idx: int32
    tensors or None."""
    if out.is_cuda:
        L.call('gnx_sparse_expand_f32', *trio_ptrs(trio), L.ptr(lines, _I32), n_lines, L.ptr(pos_of_idx, _I32), L.ptr(out),
               out.stride(0), L_pos, L.stream())
        return out
    o = out.numpy()
    o[:, :L_pos] = 0.0
    ptr, idx, val = (t.numpy() for t in trio)
    for i in range(n_lines):
        line = i if lines is None else int(lines[i])
        b, e = ptr[line], ptr[line + 1]
        p = idx[b:e].astype(np.int64) if pos_of_idx is None else pos_of_idx.numpy()[idx[b:e]].astype(np.int64)
        ok = (p >= 0) & (p < L_pos)
        o[i, p[ok]] = val[b:e][ok]
    return out


def line_moments(trio, lines, n_lines, idx_mask, device):
    """(n_lines, 2) float64 CPU tensor: the sum and the sum of squares of every line's entries with idx_mask[idx] != 0
    (`gnx_sparse_line_moments_f64`, or numpy's float64 sums on the host)."""
    if device is not None:
        out = torch.empty((n_lines, 2), dtype=torch.float64, device=device)
        L.call('gnx_sparse_line_moments_f64', *trio_ptrs(trio), L.ptr(lines, _I32), n_lines, L.ptr(idx_mask, torch.uint8),
               L.ptr(out, torch.float64), L.stream())
        return out.cpu()
    ptr, idx, val = (t.numpy() for t in trio)
    val = val.astype(np.float64)
    if idx_mask is not None:
        val = val * (idx_mask.numpy()[idx] != 0)
    line_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))            # float64 sums in entry order, per line
    out = np.stack([np.bincount(line_of, weights=val, minlength=len(ptr) - 1),
                    np.bincount(line_of, weights=val * val, minlength=len(ptr) - 1)], axis=1)
    return torch.from_numpy(out[:n_lines] if lines is None else out[lines.numpy().astype(np.int64)])


def line_clip_moments(trio, lines, n_lines, idx_mask, clip, device):
    """`line_moments` of the entries cut at their row's bound: per row i the sum and the sum of squares of min(v, clip[i])
    over the kept entries.  clip: float64 tensor (n_lines,) where the trio lives (`gnx_sparse_line_clip_moments_f64`, or numpy's
    float64 sums on the host)."""
    if device is not None:
        out = torch.empty((n_lines, 2), dtype=torch.float64, device=device)
        L.call('gnx_sparse_line_clip_moments_f64', *trio_ptrs(trio), L.ptr(lines, _I32), n_lines, L.ptr(idx_mask, torch.uint8),
               L.ptr(clip, torch.float64), L.ptr(out, torch.float64), L.stream())
        return out.cpu()
    ptr, idx, val = (t.numpy() for t in trio)
    line = np.arange(n_lines, dtype=np.int64) if lines is None else lines.numpy().astype(np.int64)
    at_line = np.maximum(line, 0)                                         # a negative entry: an empty line
    first = ptr[at_line]
    length = np.where(line >= 0, ptr[at_line + 1] - first, 0)
    row_of = np.repeat(np.arange(n_lines), length)                        # the row of every entry walked, rows in order
    at = np.repeat(first - (np.cumsum(length) - length), length) + np.arange(int(length.sum()))
    t = np.fmin(val[at].astype(np.float64), clip.numpy()[row_of])         # fmin, as the kernel: a NaN bound does not clip
    if idx_mask is not None:
        t = t * (idx_mask.numpy()[idx[at]] != 0)
    return torch.from_numpy(np.stack([np.bincount(row_of, weights=t, minlength=n_lines),
                                      np.bincount(row_of, weights=t * t, minlength=n_lines)], axis=1))


def line_max(trio, lines, n_lines, idx_mask, device):
    """(n_lines,) float32 CPU tensor: the largest of 0 and every line's entries with idx_mask[idx] != 0
    (`gnx_sparse_line_max_f32`, or numpy on the host); a line without a kept entry gives 0, the implicit value."""
    if device is not None:
        out = torch.empty(n_lines, dtype=_F32, device=device)
        L.call('gnx_sparse_line_max_f32', *trio_ptrs(trio), L.ptr(lines, _I32), n_lines, L.ptr(idx_mask, torch.uint8), L.ptr(out),
               L.stream())
        return out.cpu()
    ptr, idx, val = (t.numpy() for t in trio)
    if idx_mask is not None:
        val = np.where(idx_mask.numpy()[idx] != 0, val, np.float32(0))
    out = np.zeros(len(ptr) - 1, dtype=np.float32)
    np.maximum.at(out, np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), val)
    return torch.from_numpy(out[:n_lines] if lines is None else out[lines.numpy().astype(np.int64)])


class RowMap(nn.Module):
    """The storage rows of a SpotCounts view: `bound`, the bool mask of the rows of the view's arrays, and `pos`, the int32
    storage row -> position in the batch (-1: not in it), of which `pos[r0:]` is an array's `pos_of_idx`.  Both are
    non-persistent buffers - the map follows its owner's .to() and adds no state_dict key - and `bound_host` stays on the CPU.
    It only produces `ok`: a caller reads it back when it chooses and raises in its own words.  positions=False: no `pos`."""

    def __init__(self, counts, positions=True):
        super().__init__()
        self.bound_host = torch.zeros(int(counts._s.row_start[-1]), dtype=torch.bool)
        self.bound_host[counts.view_rows()] = True
        self.register_buffer('bound', self.bound_host, persistent=False)
        self.register_buffer('pos', torch.full((len(self.bound_host),), -1, dtype=_I32) if positions else None, persistent=False)

    def fill(self, rows):
        """`pos`, filled for the batch `rows` (storage rows inside the storage, where the map lives)."""
        pos = self.pos
        pos.fill_(-1)
        pos[rows.long()] = torch.arange(rows.numel(), dtype=_I32, device=pos.device)
        return pos

    def in_view(self, rows):
        """(ok, safe) where `rows` live, the map's device or the CPU: ok, a 0-dim bool tensor, is True when every row lies inside
        the storage and in a bound array; safe is the rows clamped into the storage, int64.  Nothing is read back here."""
        bound = self.bound_host if rows.device.type == 'cpu' else self.bound
        n = bound.numel()
        inside = (rows >= 0) & (rows < n)
        safe = rows.clamp(0, max(n - 1, 0)).long()
        return inside.all() & bound[safe].all(), safe

    def distinct(self, safe, pos):
        """0-dim bool tensor: no row of `safe` is repeated, `pos` being fill(safe)."""
        return (pos[safe] == torch.arange(safe.numel(), dtype=_I32, device=pos.device)).all()


class SpotCounts:
    """Sparse counts of a set of Visium arrays: spots x genes, raw integer counts at construction.

    X: scipy sparse or dense (n_spots, n_genes); obs: DataFrame with columns x, y, array (and annotation, x_px, y_px), one row
    per spot; gene_ids / gene_symbols: per gene.  Spots are stably sorted by array (arrays in order of first appearance).
    Refused with ValueError: a non-integer or negative raw count, a count of 2^24 or more (fp32 holds smaller ones exactly),
    an array with 2^31 or more entries.

    `to(device)` uploads the storage once and returns the resident SpotCounts.  `normalize_total` and `log1p` rewrite the
    stored values in place - the CSR and every CSC get the same bits, the function being elementwise - as scanpy rewrites
    adata.X.  `subset_genes` / `subset_arrays` return lazy views: maps and lists over the same storage, so a transform through a
    view is seen by every view.  Results of `gene_moments` / `detection_rate` are float64 CPU tensors over the selected genes."""

    def __init__(self, X, obs, gene_ids, gene_symbols=None):
        import scipy.sparse as sp
        X = sp.csr_matrix(X)
        if X.shape != (len(obs), len(gene_ids)):
            raise ValueError("X is %s for %d spots and %d genes" % (X.shape, len(obs), len(gene_ids)))
        X.sum_duplicates()
        X.eliminate_zeros()
        data = np.asarray(X.data, dtype=np.float64)
        if not np.all(np.isfinite(data)) or np.any(data != np.rint(data)) or np.any(data < 0):
            raise ValueError("raw counts must be non-negative integers")
        if np.any(data >= 2.0 ** 24):
            raise ValueError("a count of 2^24 or more is not exact in fp32")
        names = list(pd.unique(obs['array']))
        code = pd.Categorical(obs['array'], categories=names).codes
        order = np.argsort(code, kind='stable')
        X, obs = X[order], obs.iloc[order]
        X.sort_indices()
        row_start = np.concatenate([[0], np.cumsum(np.bincount(code, minlength=len(names)))]).astype(np.int64)
        csc = []
        for a in range(len(names)):
            m = X[row_start[a]:row_start[a + 1]].tocsc()
            m.sort_indices()
            csc.append(_trio(m))
        csr = (torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int32)),
               torch.from_numpy(X.data.astype(np.float32)))
        symbols = list(gene_ids) if gene_symbols is None else list(gene_symbols)
        self._s = _Store(csr, csc, row_start, names, obs, np.asarray(list(gene_ids), dtype=object),
                         np.asarray(symbols, dtype=object))
        self._genes = None                   # int64 indices into the stored genes, in channel order; None: all
        self._arrays = list(range(len(names)))
        self._maps = {}

    @classmethod
    def from_anndata(cls, adata, obs_arr='array', obs_label='annotation', obs_x='x', obs_y='y'):
        """From anything with `.X` (scipy sparse or dense, spots x genes), `.obs` (DataFrame) and `.var.index` - an AnnData of
        raw counts, or a stand-in; `.var['gene_symbol']` is used when it is there."""
        src = adata.obs
        obs = pd.DataFrame({'x': src[obs_x].values, 'y': src[obs_y].values, 'array': src[obs_arr].values}, index=src.index)
        for col in ('x_px', 'y_px'):
            if col in src.columns:
                obs[col] = src[col].values
        obs['annotation'] = src[obs_label].values if obs_label is not None and obs_label in src.columns else None
        var = adata.var
        symbols = list(var['gene_symbol']) if 'gene_symbol' in getattr(var, 'columns', []) else None
        return cls(adata.X, obs, list(var.index), symbols)

    # ---- views
    def _view(self, genes, arrays):
        v = object.__new__(SpotCounts)
        v._s, v._genes, v._arrays, v._maps = self._s, genes, arrays, {}
        return v

    def to(self, device):
        """The same counts and selection with the storage on `device` (uploaded once, here); None or 'cpu': on the host."""
        s = self._s
        if same_device(device, s.device):
            return self
        dev = None if device is None or torch.device(device).type == 'cpu' else torch.device(device)
        where = 'cpu' if dev is None else dev
        move = lambda trio: tuple(t.to(where) for t in trio)                     # noqa: E731
        store = _Store(move(s.csr), [move(t) for t in s.csc], s.row_start, s.array_names, s.obs, s.gene_ids, s.gene_symbols, dev,
                       s.raw, s.transformed_by)
        v = self._view(self._genes, self._arrays)
        v._s = store
        return v

    device = property(lambda self: self._s.device)
    arrays = property(lambda self: [self._s.array_names[a] for a in self._arrays])
    n_genes = property(lambda self: len(self._s.gene_ids) if self._genes is None else len(self._genes))
    nnz = property(lambda self: int(self._s.csr[2].numel()))          # stored entries of the whole storage
    n_spots = property(lambda self: sum(r1 - r0 for r0, r1 in map(self.array_span, self._arrays)))
    gene_ids = property(lambda self: self._s.gene_ids if self._genes is None else self._s.gene_ids[self._genes])
    gene_symbols = property(lambda self: self._s.gene_symbols if self._genes is None else self._s.gene_symbols[self._genes])

    @property
    def obs(self):
        return pd.concat([self._s.obs.iloc[slice(*self.array_span(a))] for a in self._arrays], axis=0)

    def resident_bytes(self):
        return self._s.nbytes()

    def subset_genes(self, names_or_mask):
        """A view on some genes, in the order given (names: gene ids) or in the current order (a boolean mask over the
        currently selected genes)."""
        sel = np.asarray(names_or_mask.cpu() if torch.is_tensor(names_or_mask) else names_or_mask)
        current = np.arange(len(self._s.gene_ids)) if self._genes is None else self._genes
        if sel.dtype == bool:
            if sel.shape != current.shape:
                raise ValueError("a gene mask must have one entry per selected gene (%d)" % len(current))
            picked = current[sel]
        else:
            where = {g: k for k, g in zip(current, self._s.gene_ids[current])}
            missing = [g for g in sel if g not in where]
            if missing:
                raise ValueError("%d genes are not among the selected ones (first: %s)" % (len(missing), missing[0]))
            picked = np.array([where[g] for g in sel], dtype=np.int64)
            if len(np.unique(picked)) != len(picked):
                raise ValueError("a gene is listed twice")
        return self._view(picked.astype(np.int64), self._arrays)

    def subset_arrays(self, names):
        names = [names] if isinstance(names, str) else list(names)
        mine = self.arrays
        missing = [n for n in names if n not in mine]
        if missing:
            raise ValueError("no array named %s among %s" % (missing[0], mine))
        return self._view(self._genes, [self._s.array_names.index(n) for n in names])

    # ---- the view vocabulary: what every walk over the view's arrays is written in
    def array_span(self, a):
        """(first storage row, one past the last) of the array with id `a`: Python ints from the host row_start."""
        return int(self._s.row_start[a]), int(self._s.row_start[a + 1])

    def view_rows(self):
        """int64 numpy array: the storage rows of the view's arrays, in view order."""
        return np.concatenate([np.arange(*self.array_span(a), dtype=np.int64) for a in self._arrays] or [np.zeros(0, np.int64)])

    def _array_ids(self, names=None):
        """The array ids of `names`, in the order given; None: the view's arrays."""
        return self._arrays if names is None else [self._s.array_names.index(n) for n in names]

    def bound_csc(self, arrays=None):
        """Yields (k, a, trio, r0) per array of `arrays` (names; None: the view's), in that order: k counts from 0 (a launch
        accumulates when k > 0), a is the array id, trio its CSC, r0 its first storage row (map[r0:] is its `pos_of_idx`)."""
        for k, a in enumerate(self._array_ids(arrays)):
            yield k, a, self._s.csc[a], self.array_span(a)[0]

    def host_csr(self, rows=None, dtype=np.float32):
        """scipy CSR (len(rows), G) of the storage rows `rows` (numpy int64, all >= 0; None: every row) over the selected
        genes, in `dtype`: the stored values as they are now, counts on the host."""
        import scipy.sparse as sp
        ptr, idx, val = (t.numpy() for t in self._s.csr)
        X = sp.csr_matrix((val, idx, ptr), shape=(len(ptr) - 1, len(self._s.gene_ids)), copy=False)
        if rows is not None:
            X = X[rows]
        if self._genes is not None:
            X = X[:, self._genes]
        return X.astype(dtype)

    # ---- maps (built once per view, kept where the kernels read them)
    def _put(self, array):
        t = torch.from_numpy(np.ascontiguousarray(array))
        return t if self._s.device is None else t.to(self._s.device)

    def gene_lines(self):
        """int32 list of the selected genes in channel order (the `lines` of a CSC launch), or None: all, in order."""
        if self._genes is None:
            return None
        if 'lines' not in self._maps:
            self._maps['lines'] = self._put(self._genes.astype(np.int32))
        return self._maps['lines']

    def gene_channel(self):
        """int32 map gene -> channel (-1: not selected; the `pos_of_idx` of a CSR launch), or None: the identity."""
        if self._genes is None:
            return None
        if 'channel' not in self._maps:
            pos = np.full(len(self._s.gene_ids), -1, dtype=np.int32)
            pos[self._genes] = np.arange(len(self._genes), dtype=np.int32)
            _check_injective(pos, "gene -> channel")
            self._maps['channel'] = self._put(pos)
        return self._maps['channel']

    def gene_mask(self):
        if self._genes is None:
            return None
        if 'mask' not in self._maps:
            mask = np.zeros(len(self._s.gene_ids), dtype=np.uint8)
            mask[self._genes] = 1
            self._maps['mask'] = self._put(mask)
        return self._maps['mask']

    def _host_neighbors(self, n_rings=1):
        """The numpy neighbour tables of the view's arrays, in view order; built once per n_rings."""
        from .spatial import neighbor_table
        key = ('neighbors', n_rings)
        if key not in self._maps:
            obs, tables = self._s.obs, []
            for a in self._arrays:
                r = slice(*self.array_span(a))
                try:
                    tables.append(neighbor_table(obs['x'].values[r], obs['y'].values[r], n_rings, names=obs.index[r]))
                except ValueError as err:
                    raise ValueError("array %s: %s" % (self._s.array_names[a], err)) from None
            self._maps[key] = tables
        return self._maps[key]

    def spot_neighbors(self, n_rings=1):
        """The hexagonal spot graph of every array of the view, in view order: a list of (n_a, K) int32 tensors where the
        storage is, [r][k] = the row WITHIN the array of spot r's k-th neighbour (`spatial.hex_offsets(n_rings)`: K = 6 for
        n_rings=1, 18 for 2), -1 where it is absent - from the integer obs x, y through a dictionary, O(n), built once per
        n_rings.  ValueError naming the array and the spot: two spots on one coordinate, a spot with x + y odd."""
        key = ('neighbors_put', n_rings)
        if key not in self._maps:
            self._maps[key] = [self._put(t) for t in self._host_neighbors(n_rings)]
        return self._maps[key]

    def edge_index(self, n_rings=1):
        """(2, E) int64 CPU tensor: the directed edges (source, target) of the view's spot graph over STORAGE rows, sorted by
        source then target per array - what the reference's `read_visium_graph` (graph_datasets.py:145-157) returns as A,
        without its N x N pdist matrix and with the diagonal neighbours its `<= 1` rule loses to rounding."""
        from .spatial import edge_index
        return torch.from_numpy(edge_index(self._host_neighbors(n_rings), [self.array_span(a)[0] for a in self._arrays]))

    # ---- transforms (in place)
    def _csr_entries(self, a):
        """(first entry, entries) of array a inside the CSR's idx / val."""
        s = self._s
        if s.csr_ptr_host is None:
            s.csr_ptr_host = s.csr[0].cpu().numpy()
        r0, r1 = self.array_span(a)
        e0, e1 = s.csr_ptr_host[r0], s.csr_ptr_host[r1]
        return int(e0), int(e1 - e0)

    def spot_totals(self):
        """float64 CPU tensor (n_spots of the whole storage,): every spot's total over the selected genes."""
        s = self._s
        return line_moments(s.csr, None, len(s.csr[0]) - 1, self.gene_mask(), s.device)[:, 0]

    def normalize_total(self, target_sum=1e4):
        """x = float32(c) / (float32(S) / float32(target_sum)) for the spots of the selected arrays, S the spot's total over the
        selected genes (spots with S == 0 are left as they are).  Every stored value of those spots is rewritten."""
        s = self._s
        S = self.spot_totals().numpy()
        s.rewritten_by('normalize_total')
        d = np.ones(len(S), dtype=np.float32)
        for a in self._arrays:
            r = slice(*self.array_span(a))
            d[r] = np.where(S[r] == 0, np.float32(1), S[r].astype(np.float32) / np.float32(target_sum))
        if s.device is None:
            ptr, _, val = (t.numpy() for t in s.csr)
            val /= np.repeat(d, np.diff(ptr))
            for _, _, trio, r0 in self.bound_csc():
                _, idx, v = (t.numpy() for t in trio)
                v /= d[r0:][idx]
            return self
        dd = torch.from_numpy(d).to(s.device)
        L.call('gnx_sparse_div_by_line_f32', L.ptr(s.csr[0], _I64), L.ptr(s.csr[2]), len(d), L.ptr(dd), L.stream())
        for _, _, (_, idx, v), r0 in self.bound_csc():
            L.call('gnx_sparse_div_by_idx_f32', L.ptr(idx, _I32), L.ptr(v), v.numel(), L.ptr(dd[r0:]), L.stream())
        return self

    def log1p(self):
        """x = log1pf(x) on every stored value of the selected arrays."""
        s = self._s
        s.rewritten_by('log1p')
        for a in self._arrays:
            e0, n = self._csr_entries(a)
            for v in (s.csr[2][e0:e0 + n], s.csc[a][2]):
                if s.device is None:
                    np.log1p(v.numpy(), out=v.numpy())
                else:
                    L.call('gnx_log1p_f32', L.ptr(v), v.numel(), L.stream())
        return self

    # ---- moments
    def gene_moments(self, arrays=None):
        """(mean, std) of every selected gene over the spots of `arrays` (names; None: the selected arrays), zeros included,
        population std."""
        G = self.n_genes
        s1, s2, N = np.zeros(G), np.zeros(G), 0
        for _, a, trio, r0 in self.bound_csc(arrays):
            m = line_moments(trio, self.gene_lines(), G, None, self.device).numpy()
            s1, s2 = s1 + m[:, 0], s2 + m[:, 1]
            N += self.array_span(a)[1] - r0
        mean = s1 / N
        var = np.maximum(s2 / N - mean * mean, 0.0)
        return torch.from_numpy(mean), torch.from_numpy(np.sqrt(var))

    def gene_max(self, arrays=None):
        """float32 CPU tensor over the selected genes: the largest stored value of every gene over the spots of `arrays` (names;
        None: the selected arrays), 0 for a gene without an entry there - the divisor of a [0, 1] expression target
        (notebooks/counts_from_img.ipynb).  One `gnx_sparse_line_max_f32` launch per array over its CSC, the arrays' maxima
        combined on the host in array order; a maximum has no rounding, so host and device agree bit for bit."""
        out = np.zeros(self.n_genes, dtype=np.float32)
        for _, _, trio, _ in self.bound_csc(arrays):
            out = np.maximum(out, line_max(trio, self.gene_lines(), self.n_genes, None, self.device).numpy())
        return torch.from_numpy(out)

    def detection_rate(self):
        """Fraction of the selected arrays' spots in which every selected gene has a stored (non-zero) value.  The stored
        pattern is the raw counts' (explicit zeros are dropped at construction, the transforms map non-zeros to non-zeros)."""
        s = self._s
        hits = np.zeros(len(s.gene_ids))
        for _, _, (ptr, _, _), _ in self.bound_csc():
            hits += np.diff(ptr.cpu().numpy())
        return torch.from_numpy((hits if self._genes is None else hits[self._genes]) / self.n_spots)

    # ---- gene selection
    def highly_variable_genes(self, n_top_genes=2150, span=0.3, batch=None):
        """Seurat-v3 highly variable genes of this view - its genes, the spots of its arrays - from the RAW counts: what
        `sc.pp.highly_variable_genes(adata, flavor='seurat_v3', n_top_genes=...)` computes in the reference's
        notebooks/register_hvgs.ipynb, as a `hvg.HighlyVariableGenes` (`.highly_variable`, a bool mask over the view's genes
        for `subset_genes`; `.means`, `.variances`, `.variances_norm`, `.highly_variable_rank`, `.highly_variable_nbatches`;
        `.to_frame()`), float64 / int64 / bool CPU arrays.  batch=None: the whole view is one batch; 'array': every array is
        one, as scanpy's batch_key.  Call it before `normalize_total`.

        The arithmetic is fixed in gridnext_amd/hvg.py and is not pinned to scanpy: the loess fit of log10(variance) on
        log10(mean) is evaluated DIRECTLY at every gene (scikit-misc interpolates on a k-d tree by default, so scores near
        the cut can differ), ties in the ranking go to the lower gene index (scanpy leaves them to quicksort), and a run of
        equal means never makes the fit fail (scanpy is known to fail there).  On a device, per batch: ONE
        `gnx_loess_fit_f64` launch and one `gnx_sparse_line_clip_moments_f64` launch per array of the batch, after one
        `gnx_sparse_line_moments_f64` launch per array of the view; nothing of size spots x genes is allocated.

        ValueError, before the loess fit or the clipped pass are launched: stored values that `normalize_total` or `log1p` have
        rewritten (the message names the transform), n_top_genes outside [1, G], span outside (0, 1], a batch other than
        None / 'array', a batch with fewer than 2 spots, fewer than 3 genes with a positive variance in a batch."""
        from .hvg import highly_variable_genes
        return highly_variable_genes(self, n_top_genes, span, batch)

    def spatial_autocorr(self, n_rings=1, n_perms=None, seed=0):
        """Moran's I and Geary's C of every gene of this view over its hexagonal spot graph (`spot_neighbors(n_rings)`), from
        the stored values AS THEY ARE NOW, raw or normalised - what squidpy's `spatial_neighbors` + `spatial_autocorr` is used
        for - as a `spatial.SpatialAutocorr`: I, C, expected_I, var_norm_*, pval_norm_*, pval_norm_fdr_bh_*; with n_perms also
        pval_sim_*, mean_sim_*, var_sim_*, pval_z_sim_*, sim_I, sim_C; `.to_frame()`; `.top(n, by='I')`, a bool mask for
        `subset_genes`.  The graph is binary and block diagonal (no edge between arrays); permutations (numpy's
        default_rng(seed), one per array and round) stay within an array; p-values are one-sided towards positive
        autocorrelation.  The arithmetic is fixed in gridnext_amd/spatial.py and is not pinned to squidpy.

        On a device, per array of the view: one `gnx_sparse_line_moments_f64` launch and one `gnx_sparse_line_spatial_f64`
        launch per chunk of at most 64 MB of neighbour tables (the table itself, then one relabelled table per permutation,
        built on the host); nothing of size spots x genes is allocated.  On the host: scipy's float64 `A @ X`.

        ValueError, before any launch: n_rings other than 1 or 2, n_perms below 1, a view of fewer than 3 spots or without a
        single edge, two spots on one coordinate or a spot with x + y odd, on a device an array of more spots than
        `gnx_sparse_spatial_max_idx()` = 32 768 (the host path, device=None, has no cap)."""
        from .spatial import spatial_autocorr
        return spatial_autocorr(self, n_rings, n_perms, seed)

    # ---- PCA
    def fit_pca(self, n_components=None, scale=True, max_genes=8192):
        """A `count_pca.CountPCA` of the stored values as they are now (after normalize_total and log1p, for the reference's
        recipe, scripts/fit_pca_unified_cortex.py:33-100) over this view's genes and the spots of its arrays: the eigenvectors
        of the covariance of (X - mean) / scale, from the Gram matrix X^T X in double - `gnx_sparse_gram_f64`, one launch per
        array in view order, on a device; scipy's float64 product on the host - and float64 host work after it.  scale=True:
        scale is the population std, 1 where it is 0 (sklearn's StandardScaler); False: all ones.  n_components: None keeps
        min(G, N - 1); an int must lie in [1, min(G, N - 1)].  More than `max_genes` genes raise ValueError with the bytes a
        (G, G) double matrix would need.  The scaled values are not clipped (the script's np.minimum(X, 10) is not linear in
        the counts)."""
        from .count_pca import fit_pca
        return fit_pca(self, n_components, scale, max_genes)


def _labels_of(counts, classes):
    """(classes, int64 array over counts.obs: class id, or -1 where a spot has no annotation)."""
    annot = counts.obs['annotation'].values if 'annotation' in counts.obs.columns else np.full(counts.n_spots, None)
    has = np.array([a is not None and not (isinstance(a, float) and np.isnan(a)) and a != '' for a in annot], dtype=bool)
    if classes is None:
        classes = np.unique(np.asarray([str(a) for a in annot[has]]))
    classes = np.asarray(classes)
    ids = np.full(len(annot), -1, dtype=np.int64)
    if has.any():
        strs = np.asarray([str(a) for a in annot[has]])
        at = np.searchsorted(classes, strs)
        if np.any(at >= len(classes)) or np.any(classes[np.minimum(at, len(classes) - 1)] != strs):
            raise ValueError("an annotation is not among the classes given")
        ids[has] = at
    return classes, ids


def _pc_layer(counts, use_pcs, pca, others):
    """The frozen layer behind `use_pcs=`: `pca.to_layer(counts, use_pcs)`, or None when use_pcs is None.  others: the
    keywords use_pcs excludes, name -> whether it was given."""
    if use_pcs is None:
        return None
    if pca is None:
        raise ValueError("use_pcs needs pca=: a CountPCA fitted on these counts (SpotCounts.fit_pca)")
    for name, given in others.items():
        if given:
            raise ValueError("use_pcs cannot be combined with %s" % name)
    if isinstance(use_pcs, bool) or int(use_pcs) != use_pcs or not 1 <= use_pcs <= len(pca.components_):
        raise ValueError("use_pcs must be an integer in [1, %d], the components of the PCA, got %r" % (len(pca.components_), use_pcs))
    return pca.to_layer(counts, int(use_pcs))


def _refuse_worker(counts):
    if counts.device is not None and torch.utils.data.get_worker_info() is not None:
        raise RuntimeError("counts on a HIP device are expanded on that device in the calling process: use "
                           "DataLoader(num_workers=0)")


class SparseCountDataset(Dataset):
    """One item per annotated spot of `counts` (its selected arrays, in order): (vector (G,) float32 over the selected genes,
    label int64) - `anndata_to_tensordataset` (reference count_datasets.py:347-376) without the dense matrix.  `classes`: the
    sorted unique annotations (or the ones given, to share them between a training and a validation view).  `__getitems__`
    (what a DataLoader's fetcher calls with a batch of indices) makes ONE expand launch into one (B, G) buffer and returns its
    rows.  Counts on the CPU: the host path.  `as_rows=True`: an item is (the spot's storage row index, an int64 scalar tensor,
    label) and nothing is launched - what `sparse_linear.SparseCountLinear` consumes through a stock DataLoader.
    `use_pcs=k, pca=` (a `CountPCA` of this storage and gene selection; the reference's use_pcs, count_datasets.py:309-376):
    an item is ((k,) float32: the spot's first k PCs, label), a batch ONE forward launch of `pca.to_layer(counts, k)`."""

    def __init__(self, counts, classes=None, as_rows=False, use_pcs=None, pca=None):
        super().__init__()
        self.counts, self.as_rows = counts, bool(as_rows)
        self.pc_layer = _pc_layer(counts, use_pcs, pca, {'as_rows=True': as_rows})
        self.classes, ids = _labels_of(counts, classes)
        self.rows, self.annotations = counts.view_rows()[ids >= 0].astype(np.int32), ids[ids >= 0]

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, idx):
        return self.__getitems__([idx])[0]

    def __getitems__(self, indices):
        indices = [range(len(self))[int(k)] for k in indices]
        if self.as_rows:
            return [(torch.tensor(int(self.rows[k]), dtype=_I64), torch.tensor(self.annotations[k]).long()) for k in indices]
        c = self.counts
        _refuse_worker(c)
        lines = torch.from_numpy(self.rows[indices])
        if self.pc_layer is not None:
            with torch.no_grad():
                buf = self.pc_layer(lines)
            return [(buf[b], torch.tensor(self.annotations[k]).long()) for b, k in enumerate(indices)]
        buf = torch.empty((len(indices), c.n_genes), dtype=_F32, device='cpu' if c.device is None else c.device)
        if c.device is not None:
            lines = lines.to(c.device)
        expand(c._s.csr, lines, len(indices), c.gene_channel(), buf, c.n_genes)
        return [(buf[b], torch.tensor(self.annotations[k]).long()) for b, k in enumerate(indices)]


class SparseCountGridDataset(Dataset):
    """One item per selected array of `counts`: (counts (G, h_st, w_st) float32, labels (h_st, w_st) int64: class id + 1 at the
    spot's cell, 0 elsewhere) - `anndata_to_grids` (reference utils.py:197-217) per array, as AnnGridDataset yields it, written
    channels-first by ONE expand launch on the current stream.  vis_coords: obs x, y are Visium pseudo-hex coordinates and go
    through `pseudo_hex_to_oddr`; else they are the cell.  Labels and cell maps are built once per array and kept; a spot
    outside the grid, or two spots on one cell, raise before anything is launched.  The item's tensors live where the counts do.

    `first_layer`: a frozen `sparse_linear.SparseCountLinear` over the same storage and gene selection.  An item is then
    (features (F, h_st, w_st) float32, labels): the layer's output per cell - its bias at an empty cell, what nn.Linear gives on
    the zero vector - from ONE forward launch, the transposed view of `first_layer.array_rows(...)`, in place of the
    (G, h_st, w_st) counts; the rest of f runs on it as a (F,)-feature spot classifier.  Raises if a parameter of the layer
    requires grad (stage 2 freezes f), or if the layer's storage or genes are not this dataset's.

    `use_pcs=k, pca=` (a `CountPCA` of this storage and gene selection; the reference's use_pcs, count_datasets.py:382-475,
    utils.py:197-205): an item is ((k, h_st, w_st) float32, labels): the spot's first k PCs at its cell and 0 at an empty cell,
    as `anndata_to_grids` leaves it - not the layer's bias, which `first_layer=` gives - from ONE forward launch of
    `pca.to_layer(counts, k)` and a fill: the rows without a spot are set to 0 by torch after the launch."""

    def __init__(self, counts, h_st=78, w_st=64, vis_coords=True, classes=None, first_layer=None, use_pcs=None, pca=None):
        super().__init__()
        self.counts, self.h_st, self.w_st, self.vis_coords = counts, h_st, w_st, vis_coords
        self.pc_layer = _pc_layer(counts, use_pcs, pca, {'first_layer=': first_layer is not None})
        if first_layer is not None:
            theirs = first_layer.counts
            if any(p.requires_grad for p in first_layer.parameters()):
                raise ValueError("first_layer has a parameter that requires grad: the grid stage runs on a frozen f "
                                 "(requires_grad = False on every parameter)")
            if theirs._s is not counts._s:
                raise ValueError("first_layer is bound to another storage than this dataset's counts")
            if (theirs._genes is None) != (counts._genes is None) or \
                    (counts._genes is not None and not np.array_equal(theirs._genes, counts._genes)):
                raise ValueError("first_layer's gene selection is not this dataset's")
        self.first_layer = first_layer
        self.classes, ids = _labels_of(counts, classes)
        self._ids, self._kept = ids, {}

    def __len__(self):
        return len(self.counts._arrays)

    def _array(self, k):
        if k not in self._kept:
            c = self.counts
            obs = c._s.obs
            a = c._arrays[k]
            r0, r1 = c.array_span(a)
            first = sum(b1 - b0 for b0, b1 in map(c.array_span, c._arrays[:k]))
            cells = np.empty(r1 - r0, dtype=np.int32)
            for j, (x, y) in enumerate(zip(obs['x'].values[r0:r1], obs['y'].values[r0:r1])):
                x, y = pseudo_hex_to_oddr(int(x), int(y)) if self.vis_coords else (int(x), int(y))
                if not (0 <= x < self.w_st and 0 <= y < self.h_st):
                    raise ValueError("array %s: spot %s lies outside the %d x %d grid" %
                                     (c._s.array_names[a], obs.index[r0 + j], self.h_st, self.w_st))
                cells[j] = y * self.w_st + x
            _check_injective(cells, "array %s: spot -> cell" % c._s.array_names[a])
            labels = np.zeros(self.h_st * self.w_st, dtype=np.int64)
            labels[cells] = self._ids[first:first + r1 - r0] + 1
            self._kept[k] = (c._put(cells), c._put(labels.reshape(self.h_st, self.w_st)))
        return self._kept[k]

    def __getitem__(self, idx):
        idx = range(len(self))[idx]
        c = self.counts
        cells, labels = self._array(idx)
        _refuse_worker(c)
        HW = self.h_st * self.w_st
        if self.pc_layer is not None:
            rows = self.pc_layer.array_rows(c.arrays[idx], cells, HW, zero_empty=True)
            return rows.t().view(rows.shape[1], self.h_st, self.w_st), labels.clone()
        if self.first_layer is not None:
            rows = self.first_layer.array_rows(c.arrays[idx], cells, HW)
            return rows.t().view(rows.shape[1], self.h_st, self.w_st), labels.clone()
        out = torch.empty((c.n_genes, HW), dtype=_F32, device='cpu' if c.device is None else c.device)
        expand(c._s.csc[c._arrays[idx]], c.gene_lines(), c.n_genes, cells, out, HW)
        return out.view(c.n_genes, self.h_st, self.w_st), labels.clone()
