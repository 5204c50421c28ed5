"""numpy float64 restatement of the Seurat-v3 gene selection as gridnext_amd/hvg.py fixes it, on a DENSE matrix, and the fixture
the HVG tests share.  Nothing here imports gridnext_amd: the loess is solved per point by np.linalg.lstsq on the
sqrt(w)-scaled design, the windows are found by trying every candidate, the clipped sums are math.fsum."""
import math

import numpy as np

import sparse_counts_ref as CR

U = 2.0 ** -53
N_TOP = 64


# ------------------------------------------------------------------------------------------------ loess
def window(xs, i, q):
    """(lo, cnt, h) of point i of the sorted xs: the q consecutive points with the smallest largest distance, leftmost on a
    tie; h == 0: every point that ties with xs[i]."""
    n = len(xs)
    cands = range(max(0, i - q + 1), min(i, n - q) + 1)
    far = [max(xs[i] - xs[l], xs[l + q - 1] - xs[i]) for l in cands]
    k = int(np.argmin(far))                                                      # the first of the smallest
    if far[k] == 0:
        same = np.flatnonzero(xs == xs[i])
        return int(same[0]), len(same), 0.0
    return cands[k], q, float(far[k])


def q_of(n, span):
    return max(1, min(n, int(math.floor(span * n + 1e-5))))


def point(xs, ys, lo, cnt, inv_h, degree, x0):
    """(beta_0 by lstsq, cond of the weighted moment matrix M = A^T W A, max |y| in the window) for one evaluation point."""
    x, y = xs[lo:lo + cnt], ys[lo:lo + cnt]
    u = (x - x0) * inv_h
    w = np.ones(cnt) if inv_h == 0 else np.where(np.abs(u) < 1, (1 - np.abs(u) ** 3) ** 3, 0.0)
    A = np.vander(u, degree + 1, increasing=True)
    sw = np.sqrt(w)
    beta = np.linalg.lstsq(A * sw[:, None], y * sw, rcond=None)[0]
    M = A.T @ (A * w[:, None])
    return float(beta[0]), float(np.linalg.cond(M)), float(np.abs(y).max())


def degree_of(xs, lo, cnt, inv_h, x0):
    if inv_h == 0:
        return 0
    x = xs[lo:lo + cnt]
    h = np.abs(x - x0).max()                     # a point AT the distance h has weight 0, whatever its computed u rounds to
    return min(2, len(np.unique(x[(np.abs(x - x0) < h) & (np.abs((x - x0) * inv_h) < 1)])) - 1)


def loess(xs, ys, span):
    """(fit, bar, windows) at every point of the sorted xs: bar = 8 cond(M) (cnt + 16) 2^-53 max |y in window| - normal
    equations lose cond(M), any order of cnt additions loses cnt 2^-53; windows = (lo, cnt, inv_h, degree) arrays."""
    n = len(xs)
    q = q_of(n, span)
    fit, bar, wins = np.empty(n), np.empty(n), []
    for i in range(n):
        lo, cnt, h = window(xs, i, q)
        inv_h = 0.0 if h == 0 else 1.0 / h
        d = degree_of(xs, lo, cnt, inv_h, xs[i])
        fit[i], cond, ymax = point(xs, ys, lo, cnt, inv_h, d, xs[i])
        bar[i] = 8 * cond * (cnt + 16) * U * ymax
        wins.append((lo, cnt, inv_h, d))
    lo, cnt, inv_h, d = (np.array(c) for c in zip(*wins))
    return fit, bar, (lo.astype(np.int32), cnt.astype(np.int32), inv_h.astype(np.float64), d.astype(np.int32))


# ------------------------------------------------------------------------------------------------ the recipe, dense
def batch_scores(X, span=0.3):
    """Of one batch X (spots, genes) float64 of integer counts: dict of N, mean, var, s1, s2, fit, fit_bar, reg_std, clip, c1, c2
    (fsum; counts are not negative, so these are the sums of |terms| too), c_terms (entries per gene), norm (variances_norm),
    above (entries above their bound), above_g (per gene, entries within 1e-9 of the bound included)."""
    N, G = X.shape
    s1 = np.array([math.fsum(X[:, g]) for g in range(G)])
    s2 = np.array([math.fsum(X[:, g] ** 2) for g in range(G)])
    mean = s1 / N
    var = (s2 - N * mean * mean) / (N - 1)
    pos = np.flatnonzero(var > 0)
    x, y = np.log10(mean[pos]), np.log10(var[pos])
    order = np.argsort(x, kind='stable')
    f, b, _ = loess(x[order], y[order], span)
    fit, fit_bar = np.zeros(G), np.zeros(G)
    fit[pos[order]], fit_bar[pos[order]] = f, b
    reg_std = np.sqrt(10.0 ** fit)
    clip = reg_std * np.sqrt(N) + mean
    T = np.minimum(X, clip[None, :])
    c1 = np.array([math.fsum(T[:, g]) for g in range(G)])
    c2 = np.array([math.fsum(T[:, g] ** 2) for g in range(G)])
    norm = (N * mean * mean + c2 - 2 * mean * c1) / ((N - 1) * reg_std * reg_std)
    return dict(N=N, mean=mean, var=var, s1=s1, s2=s2, fit=fit, fit_bar=fit_bar, reg_std=reg_std, clip=clip, c1=c1, c2=c2,
                c_terms=(X != 0).sum(0), norm=norm, above=int((X > clip[None, :]).sum()),
                above_g=(X > clip[None, :] * (1 - 1e-9)).sum(0))


def moment_bars(p):
    """(bar of mean, bar of var) per gene: any order of n additions is within n 2^-53 sum |term| (moments_bound of
    sparse_counts_ref), and 4 more roundings cover the division, the product, the difference and the quotient."""
    n, N = p['c_terms'] + 4, p['N']
    return n * U * np.abs(p['mean']), n * U * (p['s2'] + N * p['mean'] ** 2) / (N - 1)


def norm_bar(p):
    """Bar of a batch's variances_norm, propagated from the two kernels' bars.  With d the fit's bar (loess()), r = reg_std:
    r = 10^(fit / 2) moves by r (ln 10 / 2) d, the bound clip = r sqrt(N) + mean by dclip = r sqrt(N) ((ln 10 / 2) d + 4 u) +
    4 u mean; min(v, clip) is 1-Lipschitz in clip and moves only for the above_g entries at or over the bound, so c1 moves by
    above_g dclip and c2 by above_g 2 clip dclip; the sums themselves are within n u c1 and (n + 2) u c2 (n additions, and the
    square's one rounding inside the fma); the numerator N m^2 + c2 - 2 m c1 is formed in 8 roundings of terms of size A; the
    denominator (N - 1) r^2 moves by its (ln 10) d + 8 u."""
    N, m, r, n, d = p['N'], p['mean'], p['reg_std'], p['c_terms'], p['fit_bar']
    ln10 = math.log(10.0)
    dclip = r * math.sqrt(N) * (ln10 / 2 * d + 4 * U) + 4 * U * m
    A = N * m * m + p['c2'] + 2 * m * p['c1']
    num = (n + 2) * U * p['c2'] + 2 * m * n * U * p['c1'] + p['above_g'] * (2 * p['clip'] + 2 * m) * dclip + 8 * U * A
    return num / ((N - 1) * r * r) + np.abs(p['norm']) * (ln10 * d + 8 * U)


def select(norms, n_top):
    """(variances_norm, rank, nbatches, highly_variable) from the batches' scores: step 6, written with loops."""
    B, G = len(norms), len(norms[0])
    ranks = np.full((B, G), np.nan)
    for b in range(B):
        order = sorted(range(G), key=lambda g: (-norms[b][g], g))
        for r, g in enumerate(order[:n_top]):
            ranks[b, g] = r
    nb = (~np.isnan(ranks)).sum(0)
    med = np.array([np.median(ranks[~np.isnan(ranks[:, g]), g]) if nb[g] else np.nan for g in range(G)])
    order = sorted(range(G), key=lambda g: (math.inf if np.isnan(med[g]) else med[g], -nb[g], g))
    hv = np.zeros(G, dtype=bool)
    hv[order[:n_top]] = True
    return np.mean(norms, axis=0), med, nb.astype(np.int64), hv


def recipe(X, row_start, batch, n_top=N_TOP, span=0.3):
    """X dense (spots, genes), row_start the arrays' first rows (and the end).  (batches' score dicts, whole-view dict's mean and
    var, the selection)."""
    spans = [(int(row_start[0]), int(row_start[-1]))] if batch is None else list(zip(row_start[:-1], row_start[1:]))
    per = [batch_scores(X[a:b], span) for a, b in spans]
    N = X.shape[0]
    s1 = np.array([math.fsum(X[:, g]) for g in range(X.shape[1])])
    s2 = np.array([math.fsum(X[:, g] ** 2) for g in range(X.shape[1])])
    mean = s1 / N
    return per, mean, (s2 - N * mean * mean) / (N - 1), select([p['norm'] for p in per], n_top)


# ------------------------------------------------------------------------------------------------ the fixture
_made = {}


def fixture():
    """(X scipy csr of raw counts, obs, gene ids, dense float64): synthetic_arrays(seed=6, n_arrays=2) - 401 spots x 300 genes -
    with planted outliers (12 genes x 3 spots, + 300 .. 3000), one never-seen gene (7) and one singleton gene (11)."""
    if 'f' not in _made:
        import scipy.sparse as sp
        X, obs, genes = CR.synthetic_arrays(seed=6, n_arrays=2)
        D = np.asarray(X.todense(), dtype=np.float64)
        rng = np.random.default_rng(65)
        for g in rng.choice(np.arange(20, 300), size=12, replace=False):
            D[rng.choice(D.shape[0], size=3, replace=False), g] += rng.integers(300, 3001, size=3)
        D[:, 7] = 0
        D[:, 11] = 0
        D[5, 11] = 4
        _made['f'] = (sp.csr_matrix(D), obs, genes, D)
    return _made['f']


def min_adjacent_gap(norm, k):
    """The smallest relative gap between adjacent ones of the k largest scores."""
    top = np.sort(norm)[::-1][:k]
    return float(((top[:-1] - top[1:]) / top[:-1]).min())


def reference(batch):
    """recipe() of the fixture for batch None / 'array', computed once: the arrays hold 200 and 201 spots."""
    if batch not in _made:
        _made[batch] = recipe(fixture()[3], [0, 200, 401], batch)
    return _made[batch]


def check_against_reference(got, batch, what):
    """The package's result against the restatement's: shared with the device test."""
    per, mean, var, (vn, rank, nb, hv) = reference(batch)
    whole = reference(None)[0][0]
    mean_bar, var_bar = moment_bars(whole)
    assert got.means.dtype == np.float64 and got.highly_variable.dtype == bool and got.highly_variable_nbatches.dtype == np.int64
    assert (np.abs(got.means - mean) <= mean_bar).all() and (np.abs(got.variances - var) <= var_bar).all(), what
    bar = np.mean([norm_bar(p) for p in per], axis=0) + 2 * U * np.abs(vn)
    err = np.abs(got.variances_norm - vn)
    print("%s, batch=%r: largest |err| of variances_norm / its bar %.3g (largest bar %.2e)"
          % (what, batch, float((err[bar > 0] / bar[bar > 0]).max()), float(bar.max())))
    assert (err <= bar).all(), what
    assert np.array_equal(got.highly_variable_rank, rank, equal_nan=True), what
    assert np.array_equal(got.highly_variable_nbatches, nb) and np.array_equal(got.highly_variable, hv), what
    assert hv.sum() == N_TOP and got.variances_norm[7] == 0 and got.variances[7] == 0
