"""numpy float64 restatement of csrc/sparse_gram.hip and of `SpotCounts.fit_pca` from dense matrices, the derived bounds, and
the fixture the sparse-PCA tests share.  Nothing here imports gridnext_amd: the tests compare the package (host path and device
path) and sklearn against this file.

Bounds.  The product of two fp32 values is exact in double, so a Gram element is a sum of n exact terms: any summation order
lies within n 2^-53 sum |v u| of the exact sum (tests/sparse_counts_ref.py: moments_bound), and integer terms whose sums stay
below 2^53 are exact in every order.  The fit: the Gram route and sklearn's SVD route each round every element of a G x G
matrix about once, 2^-53 lambda_1 per element, Frobenius norm G 2^-53 lambda_1 per route: eps = G 2^-52 lambda_1 between the
two.  Eigenvalues move by at most eps (Weyl), the angle of a separated eigenvector by sin <= 2 eps / gap (Davis-Kahan)."""
import math

import numpy as np

import sparse_counts_ref as R

STRENGTHS = (3.0, 2.4, 1.9, 1.5, 1.2, 0.9)
N_ARRAY, N_ARRAYS, G, PLANTED = 300, 2, 96, 6


# ------------------------------------------------------------------------------------------------ the kernel
def _dense_operands(csc, n_spots, gene_lines, n_channels, csr, row0, chan_of_idx, dtype):
    """(A, B) for the array's n_spots spots: A[r][a] = the value of spot r in CSC line gene_lines[a] (0 without a line),
    B[r][b] = the value of CSR row row0 + r on channel b; C = A^T B is the kernel's arithmetic."""
    cptr, cidx, cval = csc
    rptr, ridx, rval = csr
    A, B = np.zeros((n_spots, n_channels), dtype=dtype), np.zeros((n_spots, n_channels), dtype=dtype)
    for a in range(n_channels):
        line = a if gene_lines is None else int(gene_lines[a])
        if line >= 0:
            b, e = int(cptr[line]), int(cptr[line + 1])
            A[cidx[b:e], a] = cval[b:e]
    for r in range(n_spots):
        b, e = int(rptr[row0 + r]), int(rptr[row0 + r + 1])
        ch = ridx[b:e].astype(np.int64) if chan_of_idx is None else np.asarray(chan_of_idx)[ridx[b:e]].astype(np.int64)
        ok = (ch >= 0) & (ch < n_channels)
        B[r, ch[ok]] = rval[b:e][ok]
    return A, B


def gram_int(csc, n_spots, gene_lines, n_channels, csr, row0, chan_of_idx):
    """The int64 product: exact for raw counts."""
    A, B = _dense_operands(csc, n_spots, gene_lines, n_channels, csr, row0, chan_of_idx, np.int64)
    return A.T @ B


def gram_fsum(csc, n_spots, gene_lines, n_channels, csr, row0, chan_of_idx):
    """(C, n, T) float64 (n_channels, n_channels): every element as math.fsum of its exact products, the number of its terms
    and sum |v u|."""
    A, B = _dense_operands(csc, n_spots, gene_lines, n_channels, csr, row0, chan_of_idx, np.float64)
    C, n, T = (np.zeros((n_channels, n_channels)) for _ in range(3))
    for a in range(n_channels):
        rows = np.flatnonzero(A[:, a])
        if len(rows):
            P = A[rows, a][:, None] * B[rows]
            cols = np.flatnonzero(P.any(0))
            C[a, cols] = [math.fsum(col) for col in P[:, cols].T.tolist()]
            n[a], T[a] = (P != 0).sum(0), np.abs(P).sum(0)
    return C, n, T


def gram_fsum_dense(X):
    """(C, n, T) of a dense (N, G) matrix: every element of X^T X as math.fsum of its exact products, the number of its
    non-zero terms and sum |v u|."""
    X = np.asarray(X, dtype=np.float64)
    C = np.zeros((X.shape[1], X.shape[1]))
    for a in range(X.shape[1]):
        rows = np.flatnonzero(X[:, a])
        C[a] = [math.fsum(col) for col in (X[rows, a][:, None] * X[rows]).T.tolist()]
    nz = (X != 0).astype(np.float64)
    return C, nz.T @ nz, np.abs(X).T @ np.abs(X)


def gram_bound(n, T):
    return R.moments_bound(n, T)


# ------------------------------------------------------------------------------------------------ the fit
def gram64(X):
    X = np.asarray(X, dtype=np.float64)
    return X.T @ X


def sign_rule(V):
    """Each row's entry of largest magnitude positive, the first such entry on ties."""
    first = np.argmax(np.abs(V), axis=1)
    return V * np.where(V[np.arange(len(V)), first] < 0, -1.0, 1.0)[:, None]


def fit64(X, scale=True):
    """dict of the fit's results from a dense (N, G) matrix, every component kept (min(G, N - 1))."""
    X = np.asarray(X, dtype=np.float64)
    N, G_ = X.shape
    mean, std = X.mean(0), X.std(0)
    sc = np.where(std == 0, 1.0, std) if scale else np.ones(G_)
    C = gram64(X)
    C = np.triu(C) + np.triu(C, 1).T
    cov = (C / N - np.outer(mean, mean)) / np.outer(sc, sc) * (N / (N - 1))
    lam, V = np.linalg.eigh(cov)
    order = np.argsort(-lam, kind='stable')
    lam, V = np.maximum(lam[order], 0.0), V[:, order].T
    k = min(G_, N - 1)
    return dict(mean=mean, scale=sc, components=sign_rule(V[:k]), variance=lam[:k], ratio=lam[:k] / lam.sum(), all=lam)


def eps_of(lam1, n_genes):
    return n_genes * 2.0 ** -52 * lam1


def gaps(lam):
    """gap_i of every eigenvalue but the last: the distance to its nearest neighbour."""
    d = -np.diff(lam)
    return np.minimum(np.concatenate([[np.inf], d]), np.concatenate([d, [np.inf]]))[:-1]


def sin_angle(u, v):
    """sin of the angle between two unit-length directions, sign ignored; sqrt(1 - cos^2) loses everything below 1e-8, so
    the norm of the part of u orthogonal to v."""
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    return float(np.linalg.norm(u - (u @ v) * v))


def projector(V):
    return V.T @ V


# ------------------------------------------------------------------------------------------------ against sklearn
def sklearn_fit(X, scale):
    from sklearn.decomposition import PCA
    mean, std = X.mean(0), X.std(0)
    sc = np.where(std == 0, 1.0, std) if scale else np.ones(X.shape[1])
    return PCA(svd_solver='full').fit((X - mean) / sc), mean, sc


def check_fit(pca, X, scale, tag):
    """The bars of the module's docstring on a fitted CountPCA against sklearn on the dense X; returns the sklearn model."""
    sk, mean, sc = sklearn_fit(X, scale)
    N, G = X.shape
    k = min(G, N - 1)
    lam, ratio, V = (t.numpy() for t in (pca.explained_variance_, pca.explained_variance_ratio_, pca.components_))
    assert V.shape == (k, G) and lam.shape == ratio.shape == (k,) and pca.n_samples_ == N
    assert all(str(t.dtype) == 'torch.float64' and not t.is_cuda for t in (pca.components_, pca.mean_, pca.scale_,
                                                                          pca.explained_variance_, pca.explained_variance_ratio_))
    assert np.allclose(pca.mean_.numpy(), mean, rtol=0, atol=1e-14) and np.allclose(pca.scale_.numpy(), sc, rtol=0, atol=1e-13)
    eps = eps_of(sk.explained_variance_[0], G)
    gap = gaps(sk.explained_variance_)
    assert (gap[:PLANTED] >= 0.02 * sk.explained_variance_[0]).all(), gap[:PLANTED] / sk.explained_variance_[0]
    d_lam = np.abs(lam - sk.explained_variance_[:k]).max()
    d_ratio = np.abs(ratio - sk.explained_variance_ratio_[:k]).max()
    sins = [sin_angle(V[i], sk.components_[i]) for i in range(PLANTED)]
    bars = [2 * eps / gap[i] for i in range(PLANTED)]
    gap8 = sk.explained_variance_[7] - sk.explained_variance_[8]
    d_proj = np.linalg.norm(projector(V[:8]) - projector(sk.components_[:8]), 2)
    print("%s: |d lambda| %.3g (bar eps = %.3g), |d ratio| %.3g (bar %.3g), sin of the six %s (bars %s), projector of 8 %.3g "
          "(bar %.3g), smallest of the six gaps %.4f lambda_1"
          % (tag, d_lam, eps, d_ratio, eps / sk.explained_variance_.sum(), ' '.join('%.2g' % s for s in sins),
             ' '.join('%.2g' % b for b in bars), d_proj, 2 * eps / gap8, gap[:PLANTED].min() / sk.explained_variance_[0]))
    assert d_lam <= eps and d_ratio <= eps / sk.explained_variance_.sum()
    assert all(s <= b for s, b in zip(sins, bars))
    assert d_proj <= 2 * eps / gap8
    assert np.allclose(V @ V.T, np.eye(k), rtol=0, atol=1e-12)                            # rows orthonormal
    assert abs(ratio.sum() - 1) <= 1e-12 if k == G else ratio.sum() <= 1 + 1e-12
    return sk


# ------------------------------------------------------------------------------------------------ the fixture
def planted_counts():
    """(600, 96) integer counts with six planted factors, deterministic."""
    rng = np.random.default_rng(0)
    Z = rng.normal(size=(N_ARRAY * N_ARRAYS, PLANTED)) * np.array(STRENGTHS)
    loadings = rng.normal(size=(PLANTED, G)) * 0.35
    return rng.poisson(np.exp(-1.2 + Z @ loadings))


def fixture(n_classes=4):
    """(X scipy csr of the planted counts, obs DataFrame, gene ids): two arrays 'arr0', 'arr1' of 300 spots on distinct cells
    of the 78 x 64 Visium grid, annotations 'c0' .. ."""
    import pandas as pd
    import scipy.sparse as sp
    counts = planted_counts()
    rng = np.random.default_rng(1)
    frames = []
    for a in range(N_ARRAYS):
        cells = rng.choice(78 * 64, size=N_ARRAY, replace=False)
        rows, cols = cells // 64, cells % 64
        frames.append(pd.DataFrame({'x': 2 * cols + rows % 2, 'y': rows, 'array': 'arr%d' % a,
                                    'annotation': ['c%d' % k for k in rng.integers(0, n_classes, N_ARRAY)]},
                                   index=['arr%d_%d_%d' % (a, x, y) for x, y in zip(2 * cols + rows % 2, rows)]))
    return sp.csr_matrix(counts.astype(np.float64)), pd.concat(frames), ['ENSG%05d' % g for g in range(G)]


def fixture_dense():
    """float32 (600, 96): the planted counts after normalize_total(1e4) and log1p, as the package fixes the arithmetic."""
    return R.normalise_log1p_dense(planted_counts())[0]
