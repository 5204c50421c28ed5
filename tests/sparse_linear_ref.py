"""numpy restatement of csrc/sparse_linear.hip: the forward and the weight gradient of a Linear layer over sparse lines, in
float64 (with the scale T and the entry count n of the derived bound) and in the kernels' documented fp32 order (one fmaf chain
per output element, in entry order, then init + chain).  A matrix is (lineptr int64, idx int32, val float32) as in
tests/sparse_counts_ref.py; the weight is gene-major, W[G][F].  Nothing here imports gridnext_amd."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    """n + 1 roundings (n multiply-adds and the final addition of init): |error| <= gamma(n) * T."""
    n = np.asarray(n, dtype=np.float64)
    return (n + 1) * U / (1 - (n + 1) * U)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the exact product (48 bits, exact in float64), one float64 addition whose rounding
    error is recovered (TwoSum), and ONE rounding to float32 - a float64 sum that sits exactly between two float32 values is
    resolved by the sign of the recovered error, which is where rounding twice would differ from the fused instruction."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    away = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (s != r64) & (s == (r64 + away.astype(np.float64)) / 2) & (err != 0)
    # on a tie float32(s) went to even; the true sum lies on err's side of s
    toward_away = tie & ((err > 0) == (away.astype(np.float64) > r64))
    return np.where(toward_away, away, r).astype(np.float32)


def _kept(lineptr, idx, val, line, row_of_idx):
    """(matrix rows, values) of the kept entries of `line`, in entry order; a negative line has none."""
    if line < 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    b, e = int(lineptr[line]), int(lineptr[line + 1])
    r = idx[b:e].astype(np.int64) if row_of_idx is None else np.asarray(row_of_idx)[idx[b:e]].astype(np.int64)
    return r[r >= 0], val[b:e][r >= 0]


def gather_sum64(lineptr, idx, val, lines, n_rows, row_of_idx, M, init):
    """float64 (out, T, n): out[i] = init[i] + sum val[e] M[row(e)], T[i] = |init[i]| + sum |val[e] M[row(e)]| per element,
    n[i] the kept entries.  init: (n_rows, F) float64 or None."""
    F = M.shape[1]
    out, T, n = np.zeros((n_rows, F)), np.zeros((n_rows, F)), np.zeros(n_rows, dtype=np.int64)
    M = M.astype(np.float64)
    for i in range(n_rows):
        r, v = _kept(lineptr, idx, val, i if lines is None else int(lines[i]), row_of_idx)
        prod = v.astype(np.float64)[:, None] * M[r]
        out[i], T[i], n[i] = prod.sum(0), np.abs(prod).sum(0), len(r)
    if init is not None:
        out, T = out + init, T + np.abs(init)
    return out, T, n


def gather_sum32(lineptr, idx, val, lines, n_rows, row_of_idx, M, init):
    """The kernel's order in float32: per element acc = 0, acc = fmaf(val[e], M[row(e)][f], acc) in entry order, then
    init + acc (0.0f where init is None)."""
    F = M.shape[1]
    out = np.zeros((n_rows, F), dtype=np.float32)
    for i in range(n_rows):
        r, v = _kept(lineptr, idx, val, i if lines is None else int(lines[i]), row_of_idx)
        acc = np.zeros(F, dtype=np.float32)
        for rr, vv in zip(r, v):
            acc = fma32(np.full(F, vv, dtype=np.float32), M[rr], acc)
        out[i] = (np.float32(0) if init is None else init[i]) + acc
    return out


def fwd64(lineptr, idx, val, lines, n_lines, chan_of_idx, W, bias):
    init = None if bias is None else np.broadcast_to(bias.astype(np.float64), (n_lines, W.shape[1]))
    return gather_sum64(lineptr, idx, val, lines, n_lines, chan_of_idx, W, init)


def fwd32(lineptr, idx, val, lines, n_lines, chan_of_idx, W, bias):
    init = None if bias is None else np.broadcast_to(bias.astype(np.float32), (n_lines, W.shape[1]))
    return gather_sum32(lineptr, idx, val, lines, n_lines, chan_of_idx, W, init)


def wgrad64(lineptr, idx, val, gene_lines, n_channels, pos_of_idx, dY, dW=None):
    """One array's contribution on top of dW (float64 (out, T, n); dW None: written)."""
    return gather_sum64(lineptr, idx, val, gene_lines, n_channels, pos_of_idx, dY, dW)


def wgrad32(lineptr, idx, val, gene_lines, n_channels, pos_of_idx, dY, dW=None):
    return gather_sum32(lineptr, idx, val, gene_lines, n_channels, pos_of_idx, dY, dW)


def to_scipy(lineptr, idx, val, n_idx):
    import scipy.sparse as sp
    return sp.csr_matrix((val.astype(np.float64), idx, lineptr), shape=(len(lineptr) - 1, n_idx))
