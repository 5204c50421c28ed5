"""Fit a PCA on sparse counts without densifying them (the recipe of the reference's scripts/fit_pca_unified_cortex.py:33-100:
normalise to 1e4, log1p, z-score each gene over the training arrays, `PCA().fit(X)`, keep the PCs that explain more than half
the variance; the PCs are what `use_pcs` selects in count_datasets.py:309-475 and utils.py:197-205).

The fit has one hot part, the genes x genes second-moment matrix C = X^T X of the sparse matrix: `gnx_sparse_gram_f64`
(csrc/sparse_gram.hip), one launch per array of the view, in view order, into one (G, G) double buffer that is read back once;
scipy's float64 `X.T @ X` with the counts on the host.  Everything after it is small float64 work on the host:

    C        its upper triangle mirrored, so C == C.T bit for bit
    mean_    gene_moments()[0];   scale_ = the population std, 1 where it is 0 (StandardScaler's rule), or all ones
    cov      (C / N - mean mean^T) / (scale scale^T) * N / (N - 1)          the covariance of (X - mean) / scale
    eigh     numpy.linalg.eigh, eigenvalues descending; explained_variance_ratio_ is over the sum of ALL eigenvalues
    sign     each component's entry of largest magnitude is positive (the first such entry on ties)

The fitted PCA is evaluated by a frozen `SparseCountLinear` over the sparse rows: z = x @ W + b with W = (V_k / scale_).T and
b = -(mean_ / scale_) @ V_k.T, fp32.  Clipping the scaled values (`np.minimum(X, 10)` in the script) is not linear in the
counts and is out of scope: neither the fit nor the layer clips.
"""
import numpy as np
import torch

from . import _lib as L
from .visium_datasets import trio_ptrs

_I32, _F64 = torch.int32, torch.float64


def gram(counts):
    """(G, G) float64 numpy array: X^T X over the view's genes and the spots of its arrays, symmetric bit for bit."""
    s, G = counts._s, counts.n_genes
    if s.device is not None:
        C = torch.empty((G, G), dtype=_F64, device=s.device)
        if not counts._arrays:
            C.zero_()
        for k, _, trio, r0 in counts.bound_csc():
            L.call('gnx_sparse_gram_f64', *trio_ptrs(trio), L.ptr(counts.gene_lines(), _I32), G, *trio_ptrs(s.csr), r0,
                   L.ptr(counts.gene_channel(), _I32), L.ptr(C, _F64), G, 1 if k else 0, L.stream())
        C = C.cpu().numpy()
    else:
        X = counts.host_csr(counts.view_rows(), np.float64)
        C = np.asarray((X.T @ X).todense())
    upper = np.triu(C)
    return upper + np.triu(C, 1).T


def sign_rule(V):
    """The rows of V (k, G) with signs fixed: each row's entry of largest magnitude is positive, the first such entry on ties."""
    V = np.asarray(V, dtype=np.float64)
    first = np.argmax(np.abs(V), axis=1)                                   # argmax returns the first of equal maxima
    return V * np.where(V[np.arange(len(V)), first] < 0, -1.0, 1.0)[:, None]


class CountPCA:
    """A PCA fitted by `SpotCounts.fit_pca`.  float64 CPU tensors: `components_` (k, G), rows orthonormal; `mean_`, `scale_`
    (G,); `explained_variance_`, `explained_variance_ratio_` (k,).  `n_samples_`: the spots fitted on; `gene_ids`: the G genes,
    in channel order."""

    def __init__(self, counts, components, mean, scale, variance, ratio, n_samples):
        self.components_, self.mean_, self.scale_ = components, mean, scale
        self.explained_variance_, self.explained_variance_ratio_ = variance, ratio
        self.n_samples_, self.gene_ids = n_samples, np.array(counts.gene_ids, dtype=object)
        self._store = counts._s

    def n_pcs_for(self, fraction=0.5):
        """The first k whose cumulative explained_variance_ratio_ exceeds `fraction` (the script's rule, :100); ValueError when
        the kept components never do."""
        over = np.flatnonzero(np.cumsum(self.explained_variance_ratio_.numpy()) > fraction)
        if len(over) == 0:
            raise ValueError("the %d kept components explain %.6f of the variance, not more than %s"
                             % (len(self.components_), float(self.explained_variance_ratio_.sum()), fraction))
        return int(over[0]) + 1

    def _n_pcs(self, n_pcs):
        k = len(self.components_)
        if n_pcs is None:
            return k
        if isinstance(n_pcs, bool) or int(n_pcs) != n_pcs or not 1 <= n_pcs <= k:
            raise ValueError("n_pcs must be an integer in [1, %d], got %r" % (k, n_pcs))
        return int(n_pcs)

    def _check(self, counts):
        if counts._s is not self._store:
            raise ValueError("the PCA was fitted on another storage than these counts")
        mine, theirs = list(self.gene_ids), list(counts.gene_ids)
        for j in range(max(len(mine), len(theirs))):
            fitted, given = mine[j] if j < len(mine) else None, theirs[j] if j < len(theirs) else None
            if fitted != given:
                raise ValueError("the counts' gene selection is not the PCA's: gene %d is %s, the PCA was fitted on %s"
                                 % (j, given, fitted))

    def affine(self, n_pcs=None):
        """(W (G, k), b (k,)) float64 numpy: z = x @ W + b is the first k PCs of (x - mean_) / scale_."""
        k = self._n_pcs(n_pcs)
        V, scale = self.components_.numpy()[:k], self.scale_.numpy()
        return (V / scale).T, -(self.mean_.numpy() / scale) @ V.T

    def to_layer(self, counts, n_pcs=None):
        """A frozen `SparseCountLinear` (fp32, through `from_affine`) over `counts` - a view of the fitted storage with the
        fitted gene selection, any arrays - that maps storage rows to their first n_pcs PCs.  The global RNG is left as it is."""
        from .sparse_linear import SparseCountLinear
        self._check(counts)
        W, b = self.affine(n_pcs)
        with torch.random.fork_rng(devices=[]):
            return SparseCountLinear.from_affine(counts, W, b)

    def transform(self, counts, n_pcs=None):
        """(n_spots of the view, k) float32, where the counts live: the PCs of every spot of the view's arrays, in view order,
        from ONE forward launch of `to_layer(counts, n_pcs)`."""
        layer = self.to_layer(counts, n_pcs)
        with torch.no_grad():
            return layer(torch.from_numpy(counts.view_rows()))


def fit_pca(counts, n_components=None, scale=True, max_genes=8192):
    """See `SpotCounts.fit_pca`."""
    G, N = counts.n_genes, counts.n_spots
    if G > max_genes:
        raise ValueError("%d genes: a (G, G) double matrix would need %d bytes; select genes first or raise max_genes (%d)"
                         % (G, 8 * G * G, max_genes))
    most = min(G, N - 1)
    if n_components is None:
        k = most
    elif isinstance(n_components, (bool, float)) or not isinstance(n_components, (int, np.integer)):
        raise ValueError("n_components must be None or an integer, got %r" % (n_components,))
    else:
        k = int(n_components)
    if not 1 <= k <= most:
        raise ValueError("n_components must lie in [1, min(G, N - 1)] = [1, %d] for %d genes and %d spots, got %r"
                         % (most, G, N, n_components))
    C = gram(counts)
    mean, std = (t.numpy() for t in counts.gene_moments())
    sc = np.where(std == 0, 1.0, std) if scale else np.ones(G)
    cov = (C / N - np.outer(mean, mean)) / np.outer(sc, sc) * (N / (N - 1))
    lam, V = np.linalg.eigh(cov)
    order = np.argsort(-lam, kind='stable')
    lam, V = np.maximum(lam[order], 0.0), V[:, order].T
    if not lam.sum() > 0:
        raise ValueError("the %d selected genes have no variance over the %d spots: every gene is constant" % (G, N))
    V = sign_rule(V[:k])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))          # noqa: E731
    return CountPCA(counts, t(V), t(mean), t(sc), t(lam[:k]), t(lam[:k] / lam.sum()), N)
