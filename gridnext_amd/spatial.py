"""Spatially variable genes on sparse counts, host or resident: Moran's I and Geary's C of every gene over the hexagonal spot
graph, with normality and permutation p-values - what squidpy's `spatial_neighbors` + `spatial_autocorr` is used for, without
the dense or AnnData detour.  Neither squidpy nor libpysal is imported.

The graph.  The reference builds it as an N x N `pdist` matrix with the rule `0 < d <= 1` on coordinates scaled by sqrt(3) / 2
(gridnext/graph_datasets.py:145-157; its TODO asks for the O(N) enumeration).  Here a spot's neighbours are the spots at fixed
INTEGER offsets of its Visium pseudo-hex coordinates (`hex_offsets`), found through a dictionary: a table (n, K) int32 of rows
within the array, -1 where a neighbour is absent.  The graph is binary, symmetric and block diagonal: spots of different arrays
are never neighbours.

Arithmetic, fixed here (squidpy is not a dependency and is not pinned by any test).  A view has arrays a of n_a spots with
tables T_a; deg_r is the number of present neighbours of spot r, N = sum n_a, W = sum_a sum_r deg_r.  Per gene, over the stored
entries (r, v) of its line in the array's CSC, x the line as a dense vector:
    S1 = sum v   S2 = sum v^2   P = sum_r v_r (sum_k x[T[r][k]])   D = sum_r deg_r v_r   Q = sum_r deg_r v_r^2
in double, per array, added in view order (S1, S2: `gnx_sparse_line_moments_f64`; P, D, Q: `gnx_sparse_line_spatial_f64`; on the
host scipy's float64 `A @ X` with A built from the table).  m = S1 / N, den = S2 - N m^2,
    I = (N / W) (P - 2 m D + m^2 W) / den          C = ((N - 1) / (2 W)) (2 Q - 2 P) / den
- z^T W z / z^T z and sum w_ij (x_i - x_j)^2 / (2 W) over the sample variance, with z = x - m and the zeros implicit.  A gene whose
den is not above its own rounding bar (N + 4) 2^-53 (S2 + N m^2) has no variance: NaN in both.
Permutations.  For a permutation perm of an array's spots, y = x[perm]: the sums of y over T are the sums of x over the
relabelled table T'[r][k] = perm[T[inv[r]][k]] (inv = argsort(perm), -1 stays -1) - `permuted_table` - so a permutation is one
more table of the same launch; S1, S2, m, den, N and W do not change.  Draws: numpy.random.default_rng(seed); for t = 1 ..
n_perms, for every array in view order, one rng.permutation(n_a).
Normality (the same for every gene, float64 on the host), S1w = 2 W, S2w = 4 sum deg^2:
    E[I] = -1 / (N - 1)     Var I = (N^2 S1w - N S2w + 3 W^2) / ((N^2 - 1) W^2) - E[I]^2
    E[C] = 1                Var C = ((2 S1w + S2w) (N - 1) - 4 W^2) / (2 (N + 1) W^2)
p-values are one-sided towards POSITIVE autocorrelation: pval_norm = 0.5 erfc(z_I / sqrt 2) for I, 0.5 erfc(-z_C / sqrt 2) for
C; Benjamini-Hochberg over the finite ones; pval_sim = (1 + #{t: I_t >= I}) / (n_perms + 1), for C the count of C_t <= C;
mean_sim, var_sim (population) and pval_z_sim, the same tail on the simulated mean and std.

Differences from the reference and squidpy: the graph is defined by integer offsets - on the full 78 x 64 array the reference's
bare `<= 1` rule finds 19 734 of the 29 386 directed neighbour pairs and loses the 9 652 diagonal ones to rounding (d =
1.0000000000000002); the graph is block diagonal and permutations stay within an array, where squidpy permutes over all cells;
the tails of the p-values are as above."""
import math

import numpy as np
import pandas as pd
import torch

from . import _lib as L

_I32, _F64 = torch.int32, torch.float64
TABLE_CHUNK_BYTES = 64 << 20                     # of neighbour tables per launch
_RING1 = [(-2, 0), (2, 0), (-1, -1), (1, -1), (-1, 1), (1, 1)]
_RING2 = [(-4, 0), (4, 0), (-3, -1), (3, -1), (-3, 1), (3, 1), (-2, -2), (2, -2), (-2, 2), (2, 2), (0, -2), (0, 2)]
STATS = ('I', 'C')
COLUMNS = ['I', 'C', 'expected_I', 'var_norm_I', 'var_norm_C', 'pval_norm_I', 'pval_norm_C', 'pval_norm_fdr_bh_I',
           'pval_norm_fdr_bh_C']
SIM_COLUMNS = ['pval_sim_I', 'pval_sim_C', 'mean_sim_I', 'mean_sim_C', 'var_sim_I', 'var_sim_C', 'pval_z_sim_I', 'pval_z_sim_C']


# ---------------------------------------------------------------------------------------------- the graph (host)
def hex_offsets(n_rings=1):
    """The pseudo-hex offsets (dx, dy) of a spot's neighbours in the tables' fixed column order: the 6 of ring 1 (true distance
    1), then the 12 of ring 2 (true distances sqrt 3 and 2)."""
    if isinstance(n_rings, bool) or n_rings not in (1, 2):
        raise ValueError("n_rings must be 1 (6 neighbours) or 2 (18), got %r" % (n_rings,))
    return list(_RING1) if n_rings == 1 else _RING1 + _RING2


def neighbor_table(x, y, n_rings=1, names=None):
    """(n, K) int32: row [r][k] is the spot at (x[r], y[r]) + hex_offsets(n_rings)[k], or -1.  x, y: the integer Visium pseudo-hex
    coordinates (array_col, array_row) of one array's spots; O(n) through a dictionary.  ValueError naming the spot (its entry
    of `names`, else its position): two spots on one coordinate, a spot with x + y odd (not Visium pseudo-hex)."""
    offsets = hex_offsets(n_rings)
    xf, yf = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if xf.shape != yf.shape or xf.ndim != 1:
        raise ValueError("x and y must be two vectors of one length")
    if np.any(xf != np.rint(xf)) or np.any(yf != np.rint(yf)):
        raise ValueError("spot coordinates must be integers (Visium array_col, array_row)")
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    name = (lambda r: "spot %d" % r) if names is None else (lambda r: "spot %s" % (names[r],))
    where = {}
    for r, key in enumerate(zip(xi.tolist(), yi.tolist())):
        if (key[0] + key[1]) % 2:
            raise ValueError("%s at (%d, %d) has x + y odd: not Visium pseudo-hex coordinates" % (name(r), key[0], key[1]))
        if key in where:
            raise ValueError("%s and %s lie on one coordinate (%d, %d)" % (name(where[key]), name(r), key[0], key[1]))
        where[key] = r
    table = np.full((len(xi), len(offsets)), -1, dtype=np.int32)
    for (cx, cy), r in where.items():
        for k, (dx, dy) in enumerate(offsets):
            table[r, k] = where.get((cx + dx, cy + dy), -1)
    return table


def edge_index(tables, row_starts):
    """(2, E) int64 numpy array of directed edges (source, target) over storage rows: per array its table's present entries
    shifted by the array's first row, sorted by source then target - what the reference's `read_visium_graph` returns as A
    (np.where of the adjacency matrix), without the pdist."""
    parts = []
    for table, r0 in zip(tables, row_starts):
        table = np.asarray(table)
        src, k = np.nonzero(table >= 0)
        dst = table[src, k].astype(np.int64)
        order = np.lexsort((dst, src))
        parts.append(np.stack([src[order].astype(np.int64), dst[order]]) + int(r0))
    return np.concatenate(parts, axis=1) if parts else np.zeros((2, 0), dtype=np.int64)


def permuted_table(table, perm):
    """T'[r][k] = perm[T[inv[r]][k]], inv = argsort(perm), -1 staying -1: the sums of y = x[perm] over T are the sums of x
    over T'."""
    table, perm = np.asarray(table), np.asarray(perm, dtype=np.int64)
    if perm.shape != (len(table),) or not np.array_equal(np.sort(perm), np.arange(len(table))):
        raise ValueError("perm must be a permutation of the table's %d rows" % len(table))
    moved = table[np.argsort(perm, kind='stable')]
    return np.where(moved >= 0, perm[np.maximum(moved, 0)], -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------- the result
class SpatialAutocorr:
    """What `SpotCounts.spatial_autocorr` returns, float64 / int64 CPU numpy arrays over the view's genes: I, C, expected_I,
    var_norm_I, var_norm_C (the same number for every gene), pval_norm_I / _C, pval_norm_fdr_bh_I / _C; n_spots, total_weight,
    gene_ids; with permutations pval_sim_I / _C, mean_sim_I / _C, var_sim_I / _C, pval_z_sim_I / _C and sim_I, sim_C of shape
    (n_perms, G).  A gene without variance is NaN throughout."""

    def __init__(self, gene_ids, n_spots, total_weight, columns, sims=None):
        self.gene_ids, self.n_spots, self.total_weight = gene_ids, n_spots, total_weight
        self.columns = list(columns)
        for name, values in columns.items():
            setattr(self, name, values)
        self.n_perms = None if sims is None else len(sims[0])
        if sims is not None:
            self.sim_I, self.sim_C = sims

    def to_frame(self):
        """DataFrame indexed by gene id, one column per per-gene result."""
        return pd.DataFrame({c: getattr(self, c) for c in self.columns}, index=pd.Index(self.gene_ids), columns=self.columns)

    def top(self, n, by='I'):
        """bool mask over the view's genes for `subset_genes`: the n genes with the largest I (by='I') or the smallest C
        (by='C'); ties go to the lower index, NaN goes last."""
        if by not in STATS:
            raise ValueError("by must be 'I' or 'C', got %r" % (by,))
        G = len(self.I)
        if isinstance(n, bool) or int(n) != n or not 1 <= n <= G:
            raise ValueError("n must be an integer in [1, %d], the genes of the view, got %r" % (G, n))
        stat = -self.I if by == 'I' else self.C
        order = np.lexsort((np.arange(G), np.where(np.isnan(stat), np.inf, stat), np.isnan(stat)))
        mask = np.zeros(G, dtype=bool)
        mask[order[:int(n)]] = True
        return mask


# ---------------------------------------------------------------------------------------------- statistics (host, float64)
def statistics(S1, S2, P, D, Q, N, W):
    """(I, C) from the sums; P, D, Q may carry leading axes (one row per table).  NaN where the gene has no variance."""
    m = S1 / N
    den = S2 - N * m * m
    flat = ~(den > (N + 4) * 2.0 ** -53 * (S2 + N * m * m))
    with np.errstate(divide='ignore', invalid='ignore'):
        I = (N / W) * (P - 2.0 * m * D + m * m * W) / den                        # noqa: E741
        C = ((N - 1) / (2.0 * W)) * (2.0 * Q - 2.0 * P) / den
    return np.where(flat, np.nan, I), np.where(flat, np.nan, C)


def normality_variances(N, W, sum_deg2):
    """(E[I], Var I, Var C) under normality for a binary symmetric graph: S0 = W, S1w = 2 W, S2w = 4 sum deg^2."""
    N, W = float(N), float(W)
    s1w, s2w = 2.0 * W, 4.0 * float(sum_deg2)
    e_i = -1.0 / (N - 1.0)
    var_i = (N * N * s1w - N * s2w + 3.0 * W * W) / ((N * N - 1.0) * W * W) - e_i * e_i
    var_c = ((2.0 * s1w + s2w) * (N - 1.0) - 4.0 * W * W) / (2.0 * (N + 1.0) * W * W)
    return e_i, var_i, var_c


def upper_tail(z):
    """0.5 erfc(z / sqrt 2): the standard normal's P(Z >= z); NaN stays NaN."""
    from scipy.special import erfc
    return 0.5 * erfc(np.asarray(z, dtype=np.float64) / math.sqrt(2.0))


def benjamini_hochberg(p):
    """Benjamini-Hochberg adjusted p-values over the finite entries of p; the others stay NaN."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    at = np.flatnonzero(np.isfinite(p))
    if len(at):
        order = at[np.argsort(p[at], kind='stable')]
        scaled = p[order] * len(at) / np.arange(1, len(at) + 1)
        out[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return out


# ---------------------------------------------------------------------------------------------- the sums
def _host_sums(trio, lines, G, tables):
    """(n_tables, G, 3) float64: P, D, Q of every table over one array's CSC through scipy: A @ X with A built from the table."""
    import scipy.sparse as sp
    ptr, idx, val = (t.numpy() for t in trio)
    n = tables.shape[1]
    X = sp.csc_matrix((val.astype(np.float64), idx, ptr), shape=(n, len(ptr) - 1))
    if lines is not None:
        X = X[:, lines.numpy().astype(np.int64)]
    X2 = X.multiply(X)
    out = np.empty((len(tables), G, 3), dtype=np.float64)
    for t, table in enumerate(tables):
        r, k = np.nonzero(table >= 0)
        A = sp.csr_matrix((np.ones(len(r)), (r, table[r, k])), shape=(n, n))
        deg = np.asarray((table >= 0).sum(1), dtype=np.float64)
        out[t, :, 0] = np.asarray(X.multiply(A @ X).sum(0)).ravel()
        out[t, :, 1] = X.T @ deg
        out[t, :, 2] = X2.T @ deg
    return out


def line_spatial(trio, lines, n_lines, n_idx, tables, device):
    """(n_tables, n_lines, 3) float64 numpy array: P, D, Q of every line of `trio` over every table of `tables` ((n_tables,
    n_idx, K) int32: a numpy array on the host, a tensor where the trio lives on a device): ONE `gnx_sparse_line_spatial_f64`
    launch on the current stream, or scipy on the host."""
    if device is None:
        return _host_sums(trio, lines, n_lines, np.asarray(tables))
    from .visium_datasets import trio_ptrs
    n_tables, _, K = tables.shape
    out = torch.empty((n_tables, n_lines, 3), dtype=_F64, device=device)
    L.call('gnx_sparse_line_spatial_f64', *trio_ptrs(trio), L.ptr(lines, _I32), n_lines, n_idx, L.ptr(tables, _I32), K, n_tables,
           L.ptr(out, _F64), L.stream())
    return out.cpu().numpy()


def spatial_autocorr(counts, n_rings=1, n_perms=None, seed=0):
    """`SpotCounts.spatial_autocorr`: see there and the module text."""
    from .visium_datasets import line_moments
    hex_offsets(n_rings)
    if n_perms is not None and (isinstance(n_perms, bool) or int(n_perms) != n_perms or n_perms < 1):
        raise ValueError("n_perms must be None or an integer of at least 1, got %r" % (n_perms,))
    n_perms = 0 if n_perms is None else int(n_perms)
    arrays = list(counts.bound_csc())
    sizes = [counts.array_span(a)[1] - r0 for _, a, _, r0 in arrays]
    N, dev = sum(sizes), counts.device
    if N < 3:
        raise ValueError("a view of %d spots has no spatial autocorrelation: at least 3 are needed" % N)
    if dev is not None:
        cap = L.query('gnx_sparse_spatial_max_idx')
        for (_, a, _, _), n in zip(arrays, sizes):
            if n > cap:
                raise ValueError("array %s has %d spots, more than the %d the kernel holds in the LDS; the host path has no cap: "
                                 "counts.to(None), device=None" % (counts._s.array_names[a], n, cap))
    host_tables = counts._host_neighbors(n_rings)
    degs = [(t >= 0).sum(1).astype(np.int64) for t in host_tables]
    W, sum_deg2 = int(sum(d.sum() for d in degs)), int(sum((d * d).sum() for d in degs))
    if W == 0:
        raise ValueError("no spot of the view has a neighbour (W == 0): the statistics are undefined")
    resident = counts.spot_neighbors(n_rings)
    G, lines = counts.n_genes, counts.gene_lines()
    rng = np.random.default_rng(seed)
    # t = 1 .. n_perms, arrays in view order.  All draws are made here, before the chunk loop, because a chunk belongs to ONE
    # array while the draw order runs across the arrays; kept as int32, 4 n_perms N bytes of host memory (56 MB for 1 000
    # permutations of 14 000 spots) - the tables themselves exist one chunk at a time
    perms = [[rng.permutation(n).astype(np.int32) for n in sizes] for _ in range(n_perms)]
    S1, S2, PDQ = np.zeros(G), np.zeros(G), np.zeros((n_perms + 1, G, 3))
    for (k, _, trio, _), n, table, here in zip(arrays, sizes, host_tables, resident):
        mom = line_moments(trio, lines, G, None, dev).numpy()
        S1, S2 = S1 + mom[:, 0], S2 + mom[:, 1]
        step = max(1, min(65535, TABLE_CHUNK_BYTES // max(1, table.nbytes)))
        mine = np.empty((n_perms + 1, G, 3))
        for t0 in range(0, n_perms + 1, step):
            t1 = min(n_perms + 1, t0 + step)
            if t0 == 0 and t1 == 1:
                chunk = here[None] if dev is not None else table[None]
            else:
                chunk = np.stack([table if t == 0 else permuted_table(table, perms[t - 1][k]) for t in range(t0, t1)])
                if dev is not None:
                    chunk = torch.from_numpy(chunk).to(dev)
            mine[t0:t1] = line_spatial(trio, lines, G, n, chunk, dev)
        PDQ = PDQ + mine                                                         # in view order
    I_all, C_all = statistics(S1, S2, PDQ[..., 0], PDQ[..., 1], PDQ[..., 2], N, W)
    I, C = I_all[0], C_all[0]                                                    # noqa: E741
    e_i, var_i, var_c = normality_variances(N, W, sum_deg2)
    full = lambda v: np.full(G, v, dtype=np.float64)                             # noqa: E731
    cols = {'I': I, 'C': C, 'expected_I': full(e_i), 'var_norm_I': full(var_i), 'var_norm_C': full(var_c),
            'pval_norm_I': upper_tail((I - e_i) / math.sqrt(var_i)), 'pval_norm_C': upper_tail(-(C - 1.0) / math.sqrt(var_c))}
    cols['pval_norm_fdr_bh_I'] = benjamini_hochberg(cols['pval_norm_I'])
    cols['pval_norm_fdr_bh_C'] = benjamini_hochberg(cols['pval_norm_C'])
    sims = None
    if n_perms:
        sims = (I_all[1:], C_all[1:])
        nan = np.isnan(I)
        for name, stat, sim, sign in (('I', I, sims[0], 1.0), ('C', C, sims[1], -1.0)):
            beyond = (sim >= stat) if name == 'I' else (sim <= stat)
            mean, var = sim.mean(0), sim.var(0)
            with np.errstate(divide='ignore', invalid='ignore'):
                z = (stat - mean) / np.sqrt(var)
            cols['pval_sim_' + name] = np.where(nan, np.nan, (1.0 + beyond.sum(0)) / (n_perms + 1.0))
            cols['mean_sim_' + name], cols['var_sim_' + name] = mean, var
            cols['pval_z_sim_' + name] = upper_tail(sign * z)
        cols = {c: cols[c] for c in COLUMNS + SIM_COLUMNS}
    return SpatialAutocorr(np.asarray(counts.gene_ids), N, W, cols, sims)
