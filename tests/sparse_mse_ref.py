"""numpy restatement of the expression criterion - the sparse targets and mse(activation(z), target) with its gradient in
float64 - and of the per-line maximum of csrc/sparse_counts.hip.  A matrix is (lineptr int64, idx int32, val float32) as in
tests/sparse_counts_ref.py.  Nothing here imports gridnext_amd."""
import math

import numpy as np

F32 = np.float32


def targets(ptr, idx, val, rows, B, n_lines, pos_of_idx, gene_scale, G):
    """float32 (B, G): t = fl32(val * gene_scale[c]) where line rows[b] stores an entry that maps to channel c, else +0.0; a row
    outside [0, n_lines) is a line without entries."""
    t = np.zeros((B, G), dtype=F32)
    for b in range(B):
        line = b if rows is None else int(rows[b])
        if not 0 <= line < n_lines:
            continue
        for e in range(int(ptr[line]), int(ptr[line + 1])):
            c = int(idx[e]) if pos_of_idx is None else int(pos_of_idx[idx[e]])
            if 0 <= c < G:
                t[b, c] = val[e] if gene_scale is None else F32(val[e]) * F32(gene_scale[c])
    return t


def den(B, G, reduction):
    return float(B) * float(G) if reduction == 'mean' else 1.0


def sigmoid64(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(z >= 0, 1.0 / (1.0 + np.exp(-z)), np.exp(z) / (1.0 + np.exp(z)))


def loss_and_grad_f64(z, t, activation, reduction, dloss=1.0):
    """(loss, dz) in float64 of mse(activation(z), t): z, t float32 arrays."""
    z64, t64 = z.astype(np.float64), t.astype(np.float64)
    p = sigmoid64(z64) if activation else z64
    d = p - t64
    n = den(z.shape[0], z.shape[1], reduction)
    loss = math.fsum((d * d).ravel()) / n if z.size or reduction == 'sum' else float('nan')
    dz = 2.0 * d * (p * (1.0 - p) if activation else 1.0) * (dloss / n if z.size else 0.0)
    return loss, dz


def line_max(ptr, idx, val, lines, n_lines, idx_mask=None):
    """float32 (n_lines,): the largest of 0 and the kept entries of every line."""
    out = np.zeros(n_lines, dtype=F32)
    for i in range(n_lines):
        line = i if lines is None else int(lines[i])
        v = val[int(ptr[line]):int(ptr[line + 1])]
        if idx_mask is not None:
            v = v[idx_mask[idx[int(ptr[line]):int(ptr[line + 1])]] != 0]
        if len(v):
            out[i] = max(F32(0), v.max())
    return out
