"""The five per-gene sums of csrc/expr_moments.hip and gridnext_amd.expression.ExpressionMetrics, restated with math.fsum over
float64 terms: sum p, sum p^2 over all rows, sum t, sum t^2, sum p t over the STORED entries, p = act(float64(z)) through
sparse_mse_ref.sigmoid64 and t the float32 targets of sparse_mse_ref.targets.  Beside every sum: the sum of the terms'
magnitudes and the number of terms, which is what the bound is stated in.  Nothing here imports gridnext_amd."""
import math

import numpy as np

import sparse_mse_ref as R

U = 2.0 ** -53
EXTRA = 16        # roundings inside one term, with more than twofold margin: exp (1 ulp), add, divide, product


def stored_targets(ptr, idx, val, rows, B, n_lines, pos_of_idx, gene_scale, G):
    """(t float32 (B, G), stored bool (B, G)): sparse_mse_ref.targets, and where an entry was stored (a stored entry is a term
    of the sparse sums even when its value is 0)."""
    t = R.targets(ptr, idx, val, rows, B, n_lines, pos_of_idx, gene_scale, G)
    stored = R.targets(ptr, idx, np.ones_like(val), rows, B, n_lines, pos_of_idx, None, G) != 0
    return t, stored


def csc_targets(ptr, idx, val, gene_lines, n_channels, pos_of_idx, gene_scale, B):
    """The same for ONE array's CSC (a line is a gene, idx a row of the array): (t, stored) as (B, n_channels), t[pos, c] =
    fl32(val * gene_scale[c]) for the entries of line gene_lines[c] (None: line c; negative: none) whose row maps to
    pos = pos_of_idx[idx] >= 0 (None: the identity)."""
    n_lines = len(ptr) - 1
    raw = R.targets(ptr, idx, val, gene_lines, n_channels, n_lines, pos_of_idx, None, B)          # (n_channels, B)
    stored = R.targets(ptr, idx, np.ones_like(val), gene_lines, n_channels, n_lines, pos_of_idx, None, B) != 0
    if gene_scale is not None:
        raw = (raw * np.asarray(gene_scale, dtype=np.float32)[:, None]).astype(np.float32)        # the fp32 product
    return np.ascontiguousarray(raw.T), np.ascontiguousarray(stored.T)


def predictions(z, activation):
    """float64 p of float32 (or any) z: the sigmoid in its two-branch form, or z."""
    return R.sigmoid64(z) if activation else np.asarray(z, dtype=np.float64)


def sums(z, t, stored, activation):
    """(S, A, N), each (G, 5): per gene the fsum of the terms, the fsum of their magnitudes, and their number.  Columns: p, p^2
    over the B rows; t, t^2, p t over the stored entries."""
    p = predictions(z, activation)
    t = np.asarray(t, dtype=np.float64)
    B, G = p.shape
    S, A, N = np.zeros((G, 5)), np.zeros((G, 5)), np.zeros((G, 5), dtype=np.int64)
    for g in range(G):
        k = stored[:, g]
        terms = (p[:, g], p[:, g] * p[:, g], t[k, g], t[k, g] * t[k, g], p[k, g] * t[k, g])
        for j, x in enumerate(terms):
            if np.isnan(x).any():
                S[g, j] = A[g, j] = np.nan
            else:
                S[g, j], A[g, j] = math.fsum(x), math.fsum(np.abs(x))
            N[g, j] = len(x)
    return S, A, N


def bound(N, A, calls=1):
    """|sum - fsum| <= (n + 16) 2^-53 sum |term|, n the terms added so far plus the calls that added them."""
    return (np.asarray(N, dtype=np.float64) + calls + EXTRA) * U * A


def statistics(S, n):
    """mean_pred, mean_target, mse, var_p, var_t, cov from (G, 5) sums, plainly."""
    mp, mt = S[:, 0] / n, S[:, 2] / n
    return mp, mt, (S[:, 1] - 2 * S[:, 4] + S[:, 3]) / n, S[:, 1] / n - mp * mp, S[:, 3] / n - mt * mt, S[:, 4] / n - mp * mt
