"""Seurat-v3 highly variable genes on sparse counts, host or resident (the reference's notebooks/register_hvgs.ipynb:
`sc.pp.highly_variable_genes(adata, flavor='seurat_v3', n_top_genes=2150)` on the raw counts, whose genes it trains f and g on
through `select_genes=` of gridnext/count_datasets.py).  Neither scanpy nor scikit-misc is imported.

Arithmetic, fixed here (scanpy is not a dependency and is not pinned by any test).  Per batch - the whole view, or one array
with batch='array' - with N spots:
  1. mean = S1 / N, var = (S2 - N mean^2) / (N - 1), S1 and S2 the per-array sums of `SpotCounts.gene_moments` (double), added
     in array order.
  2. Over the genes with var > 0, stably sorted by x = log10(mean): y = log10(var).
  3. Direct loess of y on x, degree 2, tricube weights, no robustness iterations, evaluated at every point.  q = min(n,
     floor(span n + 1e-5)) (at least 1).  A point's window is the q consecutive sorted points whose largest distance h to it is
     smallest, the leftmost on a tie; u = (x - x0) * (1 / h), w = (1 - |u|^3)^3 for |u| < 1, else 0; the fitted value is beta_0
     of the weighted least-squares polynomial in u.  The degree is 2, lowered to d - 1 when the window's positive-weight points
     (nearer than h, and |u| < 1 as computed) hold only d < 3 distinct abscissae.  h == 0: the window is every point that ties
     with x0, weight 1, degree 0 - their mean.  Windows, h and degrees are numpy's; the sums and the LDL^T solve are `gnx_loess_fit_f64`'s on a device (one launch per
     batch) and `_fit_host`'s - the same operations in the same association, numpy's pairwise sums in place of the kernel's
     lane order - on the host.
  4. reg_std = sqrt(10^fit), fit = 0 for a gene with var == 0 (as scanpy leaves it); clip = reg_std sqrt(N) + mean.
  5. variances_norm of the batch = (N mean^2 + sum min(v, clip)^2 - 2 mean sum min(v, clip)) / ((N - 1) reg_std^2), the two
     sums from `gnx_sparse_line_clip_moments_f64` per array (numpy on the host), added in array order.
  6. Ranks per batch from a stable argsort of -variances_norm (ties to the lower gene index); a rank >= n_top_genes is NaN;
     highly_variable_rank is the median over the batches ignoring NaN, highly_variable_nbatches the count of non-NaN ranks,
     variances_norm the mean over the batches; highly_variable marks the first n_top_genes genes by (rank ascending, nbatches
     descending, NaN last, then index).  means and variances are the whole view's.

Differences from scanpy: the loess is evaluated directly at every gene, where scikit-misc interpolates on a k-d tree by
default, so scores near the cut can differ; ties are broken by gene index, where scanpy leaves them to quicksort; a run of
equal means never makes the fit fail (scanpy is known to fail there)."""
import numpy as np
import pandas as pd
import torch

from . import _lib as L

_I32, _F64 = torch.int32, torch.float64
COLUMNS = ['means', 'variances', 'variances_norm', 'highly_variable_rank', 'highly_variable_nbatches', 'highly_variable']


class HighlyVariableGenes:
    """What `SpotCounts.highly_variable_genes` returns: scanpy's columns over the view's genes, float64 / int64 / bool CPU
    numpy arrays.  `counts.subset_genes(hvg.highly_variable)` is the selected view."""

    def __init__(self, gene_ids, means, variances, variances_norm, rank, nbatches, highly_variable):
        self.gene_ids, self.means, self.variances, self.variances_norm = gene_ids, means, variances, variances_norm
        self.highly_variable_rank, self.highly_variable_nbatches, self.highly_variable = rank, nbatches, highly_variable

    def to_frame(self):
        """DataFrame indexed by gene id with scanpy's column names."""
        return pd.DataFrame({c: getattr(self, c) for c in COLUMNS}, index=pd.Index(self.gene_ids), columns=COLUMNS)


# ---------------------------------------------------------------------------------------------- loess: windows (host)
def _first_true(lo, hi, pred):
    """Per element the first k in [lo, hi] with pred(k), hi + 1 where there is none; pred is False .. False True .. True."""
    lo, hi = lo.copy(), hi + 1
    while np.any(lo < hi):
        mid = (lo + hi) // 2
        open_ = lo < hi
        ok = np.zeros(len(lo), dtype=bool)
        ok[open_] = pred(mid[open_], open_)
        hi = np.where(open_ & ok, mid, hi)
        lo = np.where(open_ & ~ok, mid + 1, lo)
    return lo


def loess_windows(xs, span):
    """(lo int32, cnt int32, inv_h float64, degree int32) of every point of the sorted abscissae xs: step 3 of the module text."""
    xs = np.asarray(xs, dtype=np.float64)
    n = len(xs)
    if n and np.any(np.diff(xs) < 0):
        raise ValueError("the abscissae of a loess fit must be sorted")
    q = max(1, min(n, int(np.floor(span * n + 1e-5))))
    i = np.arange(n, dtype=np.int64)
    first, last = np.maximum(0, i - q + 1), np.minimum(i, n - q)                 # the candidate windows' left ends
    left = lambda l, at: xs[at] - xs[l]                                          # noqa: E731  distance to the window's ends
    right = lambda l, at: xs[l + q - 1] - xs[at]                                 # noqa: E731
    far = lambda l, at: np.maximum(left(l, at), right(l, at))                    # noqa: E731
    # left() falls and right() rises with l: the smallest far() is on either side of the first l with left <= right
    cross = _first_true(first, last, lambda l, m: left(l, i[m]) <= right(l, i[m]))
    a, b = np.maximum(cross - 1, first), np.minimum(cross, last)
    best = np.where(far(a, i) <= far(b, i), a, b)
    h = far(best, i)
    lo = _first_true(first, best, lambda l, m: far(l, i[m]) <= h[m])            # the leftmost window that far away
    cnt = np.full(n, q, dtype=np.int64)
    with np.errstate(divide='ignore'):
        inv_h = np.where(h > 0, 1.0 / h, 0.0)
    tie = h == 0
    lo[tie] = np.searchsorted(xs, xs[tie], side='left')
    cnt[tie] = np.searchsorted(xs, xs[tie], side='right') - lo[tie]
    # distinct abscissae among the positive-weight points: a run [p, beyond) around the point.  A point counts when it is
    # nearer than h AND its |u| as the sums compute it is below 1; one at the distance h itself whose u rounds below 1 gets a
    # weight of some 1e-47 in the sums and is not counted
    run = np.concatenate([[0], np.cumsum(np.diff(xs) != 0)]) if n else np.zeros(0, np.int64)
    near = lambda d, m: tie[m] | ((d < h[m]) & (d * inv_h[m] < 1.0))             # noqa: E731
    p = _first_true(lo, i, lambda k, m: near(xs[i[m]] - xs[k], m))
    beyond = _first_true(i, lo + cnt - 1, lambda k, m: ~near(xs[k] - xs[i[m]], m))
    distinct = run[beyond - 1] - run[p] + 1 if n else run
    degree = np.where(tie, 0, np.minimum(2, distinct - 1))
    return lo.astype(np.int32), cnt.astype(np.int32), inv_h, degree.astype(np.int32)


# ---------------------------------------------------------------------------------------------- loess: sums and solve
def _solve(degree, m, r):
    """beta_0 per row of the moments m (k, 5) and r (k, 3): the LDL^T of csrc/loess.hip, operation for operation."""
    with np.errstate(divide='ignore', invalid='ignore'):
        m0, m1, m2, m3, m4 = m.T
        r0, r1, r2 = r.T
        l10 = m1 / m0
        d1 = m2 - l10 * m1
        z1 = r1 - l10 * r0
        one = r0 / m0 - l10 * (z1 / d1)
        l20 = m2 / m0
        l21 = (m3 - l20 * m1) / d1
        d2 = (m4 - l20 * m2) - l21 * (l21 * d1)
        z2 = (r2 - l20 * r0) - l21 * z1
        b2 = z2 / d2
        b1 = z1 / d1 - l21 * b2
        two = (r0 / m0 - l10 * b1) - l20 * b2
    return np.where(degree == 0, r0 / m0, np.where(degree == 1, one, two))


def _fit_host(xs, ys, lo, cnt, inv_h, degree, chunk_terms=1 << 21):
    """numpy float64 restatement of `gnx_loess_fit_f64`: the same terms, numpy's pairwise sums in place of the lane order."""
    n = len(xs)
    out = np.empty(n, dtype=np.float64)
    i = 0
    while i < n:                                 # runs of equal cnt, in chunks of about chunk_terms weighted terms
        c = int(cnt[i])
        j = i + 1
        while j < n and cnt[j] == c and (j - i) * c < chunk_terms:
            j += 1
        at = lo[i:j, None].astype(np.int64) + np.arange(c)
        u = (xs[at] - xs[i:j, None]) * inv_h[i:j, None]
        a = np.abs(u)
        t = 1.0 - a * a * a
        w = np.where(inv_h[i:j, None] == 0.0, 1.0, np.where(a < 1.0, t * t * t, 0.0))
        p1 = w * u
        p2 = p1 * u
        p3 = p2 * u
        p4 = p3 * u
        y = ys[at]
        m = np.stack([w.sum(1), p1.sum(1), p2.sum(1), p3.sum(1), p4.sum(1)], axis=1)
        r = np.stack([(w * y).sum(1), (p1 * y).sum(1), (p2 * y).sum(1)], axis=1)
        out[i:j] = _solve(degree[i:j], m, r)
        i = j
    return out


def loess_fit(xs, ys, span=0.3, device=None):
    """float64 numpy array: the direct loess fit of ys on the sorted xs at every point (module text, step 3).  device None: numpy;
    a HIP device: ONE `gnx_loess_fit_f64` launch on the current stream."""
    xs, ys = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
    if xs.shape != ys.shape or xs.ndim != 1:
        raise ValueError("xs and ys must be two vectors of one length")
    if not 0 < span <= 1:
        raise ValueError("span must lie in (0, 1], got %r" % (span,))
    lo, cnt, inv_h, degree = loess_windows(xs, span)
    return fit_windows(xs, ys, lo, cnt, inv_h, degree, device)


def fit_windows(xs, ys, lo, cnt, inv_h, degree, device=None):
    """The sums and the solve for windows already chosen; a degree outside 0 .. 2 or a window outside the points raises
    ValueError before anything is uploaded."""
    n = len(xs)
    if np.any((degree < 0) | (degree > 2)):
        raise ValueError("a loess degree must be 0, 1 or 2")
    if np.any((lo < 0) | (cnt < 1) | (lo.astype(np.int64) + cnt > n)):
        raise ValueError("a loess window must lie inside the points")
    if device is None:
        return _fit_host(xs, ys, lo, cnt, inv_h, degree)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)         # noqa: E731
    dx, dy, dlo, dcnt, dih, ddeg = (put(a) for a in (xs, ys, lo, cnt, inv_h, degree))
    out = torch.empty(n, dtype=_F64, device=device)
    L.call('gnx_loess_fit_f64', L.ptr(dx, _F64), L.ptr(dy, _F64), n, L.ptr(dlo, _I32), L.ptr(dcnt, _I32), L.ptr(dih, _F64),
           L.ptr(ddeg, _I32), L.ptr(out, _F64), n, L.stream())
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the selection
def batch_moments(s1, s2, N):
    """(mean, var) per gene from the sums over N spots: scanpy's _get_mean_var with ddof=1."""
    mean = s1 / N
    return mean, (s2 - N * mean * mean) / (N - 1)


def clip_bounds(mean, var, N, span, device=None):
    """(reg_std, clip) per gene of one batch: steps 2 - 4."""
    pos = np.flatnonzero(var > 0)
    if len(pos) < 3:
        raise ValueError("a batch has %d genes with a positive variance; the loess fit needs at least 3" % len(pos))
    x, y = np.log10(mean[pos]), np.log10(var[pos])
    order = np.argsort(x, kind='stable')
    fit = np.zeros(len(mean), dtype=np.float64)
    fit[pos[order]] = loess_fit(x[order], y[order], span, device)
    reg_std = np.sqrt(10.0 ** fit)
    return reg_std, reg_std * np.sqrt(N) + mean


def normalised_variance(mean, reg_std, N, c1, c2):
    """Step 5 from the clipped sums c1 = sum min(v, clip), c2 = sum min(v, clip)^2."""
    return (N * mean * mean + c2 - 2.0 * mean * c1) / ((N - 1) * reg_std * reg_std)


def rank_and_select(norm, n_top_genes):
    """Step 6 from the batches' normalised variances norm (B, G): (variances_norm, rank, nbatches, highly_variable)."""
    B, G = norm.shape
    ranks = np.empty((B, G), dtype=np.float64)
    for b in range(B):
        ranks[b, np.argsort(-norm[b], kind='stable')] = np.arange(G)
    ranks[ranks >= n_top_genes] = np.nan
    seen = ~np.isnan(ranks)
    nbatches = seen.sum(0).astype(np.int64)
    srt = np.sort(ranks, axis=0)                                                 # NaN last: the median of the first nbatches
    k = np.maximum(nbatches, 1)
    cols = np.arange(G)
    median = 0.5 * (srt[(k - 1) // 2, cols] + srt[k // 2, cols])
    median = np.where(nbatches > 0, median, np.nan)
    order = np.lexsort((cols, -nbatches, np.where(np.isnan(median), np.inf, median)))
    hv = np.zeros(G, dtype=bool)
    hv[order[:n_top_genes]] = True
    return norm.mean(0), median, nbatches, hv


def highly_variable_genes(counts, n_top_genes=2150, span=0.3, batch=None):
    """`SpotCounts.highly_variable_genes`: see there and the module text."""
    from .visium_datasets import line_clip_moments, line_moments
    s = counts._s
    if not s.raw:
        raise ValueError("highly_variable_genes needs raw counts: the stored values were rewritten by %s; call it before "
                         "the transforms" % s.transformed_by)
    G = counts.n_genes
    if isinstance(n_top_genes, bool) or int(n_top_genes) != n_top_genes or not 1 <= n_top_genes <= G:
        raise ValueError("n_top_genes must be an integer in [1, %d], the genes of the view, got %r" % (G, n_top_genes))
    if not 0 < span <= 1:
        raise ValueError("span must lie in (0, 1], got %r" % (span,))
    if batch not in (None, 'array'):
        raise ValueError("batch must be None (the whole view is one batch) or 'array' (every array is one), got %r" % (batch,))
    arrays = list(counts.bound_csc())
    sizes = {a: counts.array_span(a)[1] - r0 for _, a, _, r0 in arrays}
    batches = [[a for _, a, _, _ in arrays]] if batch is None else [[a] for _, a, _, _ in arrays]
    for members in batches:
        if sum(sizes[a] for a in members) < 2:
            raise ValueError("a batch of %d spots has no variance: at least 2 are needed" % sum(sizes[a] for a in members))
    lines, dev = counts.gene_lines(), counts.device
    trios = {a: trio for _, a, trio, _ in arrays}
    moments = {a: line_moments(trios[a], lines, G, None, dev).numpy() for a in trios}       # one launch per array

    def sums(members, table):
        s1, s2 = np.zeros(G), np.zeros(G)
        for a in members:                                                        # in array order
            s1, s2 = s1 + table[a][:, 0], s2 + table[a][:, 1]
        return s1, s2, sum(sizes[a] for a in members)

    norm = np.empty((len(batches), G), dtype=np.float64)
    for b, members in enumerate(batches):
        s1, s2, N = sums(members, moments)
        mean, var = batch_moments(s1, s2, N)
        reg_std, clip = clip_bounds(mean, var, N, span, dev)
        bound = torch.from_numpy(clip) if dev is None else torch.from_numpy(clip).to(dev)
        clipped = {a: line_clip_moments(trios[a], lines, G, None, bound, dev).numpy() for a in members}
        c1, c2, _ = sums(members, clipped)
        norm[b] = normalised_variance(mean, reg_std, N, c1, c2)
    means, variances = batch_moments(*sums([a for _, a, _, _ in arrays], moments))
    vn, rank, nbatches, hv = rank_and_select(norm, int(n_top_genes))
    return HighlyVariableGenes(np.asarray(counts.gene_ids), means, variances, vn, rank, nbatches, hv)
