"""Predict a spot's expression vector from its image patch (the reference's notebooks/counts_from_img.ipynb: a DenseNet-121
whose head is nn.Linear(1024, n_genes) + nn.Sigmoid() under nn.MSELoss against the [0, 1]-normalised counts of the spot; the
notebook calls its loop train_selfsupervised).  The reference's loop is unfinished - it appends `val_loss` / `train_loss`, names
that are never assigned - so what is built here is the notebook's documented contract.

`SparseMSELoss` is the criterion over the sparse rows of a `SpotCounts` ON THE HOST: the network returns the PRE-activation z,
the criterion applies the sigmoid, and the target of batch row b is the stored row rows[b] of the CSR times a per-gene scale -
the composition scipy expand, * gene_scale, torch.sigmoid, F.mse_loss under plain autograd.  There is no device form of it
yet: with resident counts the module raises, it never computes the composition there behind the caller's back.  The per-gene
maximum that the [0, 1] target divides by, `SpotCounts.gene_max`, does run on the device (gnx_sparse_line_max_f32).

`ExpressionNet` is the model: any backbone that maps patches to (B, F) features - a `DenseNet(classify=False)` - and a Linear
head that returns z.  `multimodal_datasets.SlideCountDataset` feeds it and `training.train_expression` is the loop.

`ExpressionMetrics` is the evaluation stage, on the host AND on resident counts: per-gene Pearson correlation, R^2 and MSE of
activation(z) against the same sparse targets, from five sums per gene that csrc/expr_moments.hip takes over the resident
CSCs - no dense (B, G) target, eager, forward only, no atomics.  Its `loss` is the validation loss over the sparse rows that
a user with resident counts could not get; it is not the criterion and has no backward.  `evaluate_expression` is the pass.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import functional as GF
from .visium_datasets import RowMap, SpotCounts, same_device, trio_ptrs

_I32, _I64, _F32 = torch.int32, torch.int64, torch.float32


def _check_target(counts, activation, gene_scale):
    """Validates what SparseMSELoss and ExpressionMetrics share; returns gene_scale as a float32 CPU tensor (G,), or None."""
    if activation not in ('sigmoid', None):
        raise ValueError("activation must be 'sigmoid' or None, got %r" % (activation,))
    if gene_scale is not None:
        gene_scale = torch.as_tensor(gene_scale).detach().to(device='cpu', dtype=_F32).contiguous()
        if gene_scale.shape != (counts.n_genes,):
            raise ValueError("gene_scale must be (%d,), one per selected gene, got %s" % (counts.n_genes, tuple(gene_scale.shape)))
    return gene_scale


class SparseMSELoss(nn.Module):
    """nn.MSELoss(reduction)(activation(z), target) where the target of batch row b is the sparse row rows[b] of `counts` (a
    SpotCounts view ON THE HOST: its gene selection, its arrays) over the selected genes, times `gene_scale`.

    activation: 'sigmoid' (the notebook's nn.Sigmoid(), applied HERE: the model returns z) or None.  gene_scale: None, or a
    (G,) tensor, kept as a float32 buffer; `SparseMSELoss.unit_scale(counts)` gives 1 / gene_max, which puts every target in
    [0, 1].  reduction: 'mean' (over B * G elements) or 'sum'.

    forward(z, rows): z is (B, counts.n_genes), floating point, PRE-activation, on the CPU; rows is an int64 / int32 tensor (B,)
    of STORAGE rows, the convention of `SparseCountLinear` and `SparseCountDataset(as_rows=True).rows`; repeats are fine.
    Returns the 0-dim loss in z's dtype: scipy's rows of the CSR, densified, * gene_scale, torch.sigmoid, F.mse_loss - the
    composition itself, bit for bit, under plain autograd.

    With `check_rows=True` (the default) the rows must lie inside the storage and belong to an array of the bound view
    (`visium_datasets.RowMap.in_view`, the check SparseCountLinear makes); `check_rows=False` skips it.

    Raises ValueError, naming what differs: z elsewhere than on the CPU, a width that is not counts.n_genes, a z that is not
    floating point.  Counts on a HIP device raise RuntimeError at construction: the criterion has no device form yet, and it
    does not run the composition there in its place."""

    def __init__(self, counts, activation='sigmoid', gene_scale=None, reduction='mean', check_rows=True):
        super().__init__()
        if not isinstance(counts, SpotCounts):
            raise TypeError("counts must be a SpotCounts, got %s" % type(counts).__name__)
        if reduction not in ('mean', 'sum'):
            raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
        if counts.device is not None:
            raise RuntimeError("SparseMSELoss: the counts are on %s; the criterion has no device form yet and does not run torch's "
                               "composition there in its place - bind it to the counts on the host (SpotCounts.to(None))"
                               % counts.device)
        self.counts, self.activation, self.reduction, self.check_rows = counts, activation, reduction, bool(check_rows)
        self.register_buffer('gene_scale', _check_target(counts, activation, gene_scale), persistent=False)
        self._map = RowMap(counts, positions=False)                              # its mask only

    def extra_repr(self):
        return 'genes=%d, activation=%r, reduction=%r, gene_scale=%s' % (self.counts.n_genes, self.activation, self.reduction,
                                                                         self.gene_scale is not None)

    @classmethod
    def unit_scale(cls, counts, arrays=None):
        """(G,) float32 CPU tensor: 1 / gene_max over `arrays` (None: the view's), 1 where the maximum is 0 - from counts on the
        host or resident (`SpotCounts.gene_max`).  The largest target of an expressed gene is then fl32(max * fl32(1 / max)),
        within one rounding of 1."""
        m = counts.gene_max(arrays).numpy()
        return torch.from_numpy(np.where(m == 0, np.float32(1), np.float32(1) / np.where(m == 0, np.float32(1), m)).astype(np.float32))

    def activate(self, z):
        """The prediction a user plots: torch's sigmoid of z, or z."""
        return torch.sigmoid(z) if self.activation == 'sigmoid' else z

    def forward(self, z, rows):
        c = self.counts
        if not same_device('cpu', z.device):
            raise ValueError("SparseMSELoss: z is on %s, the counts are on cpu" % z.device)
        if z.dim() != 2 or z.shape[1] != c.n_genes:
            raise ValueError("SparseMSELoss: z must be (B, %d), one column per selected gene, got %s" % (c.n_genes, tuple(z.shape)))
        if not z.is_floating_point():
            raise ValueError("SparseMSELoss: z must be floating point, got %s" % z.dtype)
        if rows.dim() != 1 or rows.dtype not in (_I32, _I64) or rows.numel() != z.shape[0]:
            raise ValueError("SparseMSELoss: rows must be an int64 or int32 tensor (%d,), got %s %s" % (z.shape[0], rows.dtype,
                                                                                                      tuple(rows.shape)))
        rows = rows.cpu()
        if self.check_rows and rows.numel() and not bool(self._map.in_view(rows)[0]):
            raise ValueError("SparseMSELoss: the rows must be storage rows of the bound arrays %s (rows 0 .. %d of the storage, those "
                             "of the bound arrays only): a row outside the storage or of another array has no target here"
                             % (c.arrays, self._map.bound.numel() - 1))
        target = torch.from_numpy(c.host_csr(rows.numpy().astype(np.int64)).toarray()).to(z.dtype)
        if self.gene_scale is not None:
            target = target * self.gene_scale.to(device='cpu', dtype=z.dtype)
        return F.mse_loss(self.activate(z), target, reduction=self.reduction)


class ExpressionMetrics:
    """Which genes the image predicts: per-gene Pearson correlation, R^2 and MSE between activation(z) and the sparse targets
    of `counts` (a SpotCounts view ON THE HOST OR RESIDENT: its gene selection, its arrays), accumulated over the batches of an
    evaluation pass.  The definitions are SparseMSELoss's: p = activation(z) in float64 ('sigmoid' or None), t =
    fl32(value * gene_scale[c]) where the row stores gene c, else 0.  gene_scale: None or (G,), kept as float32 where the counts
    live (`SparseMSELoss.unit_scale(counts)`).

    State: the (G, 5) float64 table of sum p, sum p^2, sum t, sum t^2, sum p t per gene, where the counts live, and the host
    integer `n`, the rows seen.  `reset()` clears both.

    update(z, rows): z (B, G) PRE-activation, rows (B,) int64 / int32 STORAGE rows (SparseCountDataset.rows, the rows of a
    SlideCountDataset batch), on the CPU or where the counts live.  Resident counts: z is float32 on the counts' device, and the
    update is ONE `gnx_act_col_moments_f64` launch plus ONE `gnx_sparse_pred_moments_f64` launch per bound array, in view
    order, over the array's CSC - no dense (B, G) target exists at any point; with rows on the CPU only the arrays the batch
    touches are launched.  Host counts: z is any float dtype on the CPU and the same sums are taken in numpy float64 over
    scipy's rows.  Eager by contract: inside a stream capture update raises before it launches anything.

    With `check_rows=True` (the default) a row outside the storage, a row of an unbound array or a row REPEATED within the batch
    raises ValueError before any launch, at the cost of one 1-byte read-back: the row -> position map keeps one position per
    row, so a repeat would drop the repeated row's sparse terms while both its dense terms are counted.  `check_rows=False`
    skips the check and the read-back; the caller then guarantees the three conditions.

    compute() copies the table to the host once and returns a dict of float64 numpy arrays over the genes (and two scalars):
    n; mean_pred, mean_target; mse = (sum p^2 - 2 sum p t + sum t^2) / n; pearson = cov / sqrt(var_p var_t) from the raw
    moments; r2 = 1 - mse / var_t; loss = the mean of mse over the genes, what SparseMSELoss(reduction='mean') gives on all rows
    at once.  A variance at or below the rounding floor 8 n 2^-53 (sum x^2 / n) counts as zero, and pearson and r2 are NaN for
    that gene - a gene never seen, a constant prediction; n == 0 gives NaNs."""

    def __init__(self, counts, activation='sigmoid', gene_scale=None, check_rows=True):
        if not isinstance(counts, SpotCounts):
            raise TypeError("counts must be a SpotCounts, got %s" % type(counts).__name__)
        gene_scale = _check_target(counts, activation, gene_scale)
        self.counts, self.activation, self.check_rows = counts, activation, bool(check_rows)
        self.device = torch.device('cpu') if counts.device is None else counts.device
        self.gene_scale = None if gene_scale is None else gene_scale.to(self.device)
        self._map = RowMap(counts).to(self.device)                               # storage row -> position in the batch
        self.reset()

    def __repr__(self):
        return 'ExpressionMetrics(genes=%d, arrays=%d, activation=%r, gene_scale=%s, n=%d)' % (
            self.counts.n_genes, len(self.counts._arrays), self.activation, self.gene_scale is not None, self.n)

    def reset(self):
        self.table = torch.zeros((self.counts.n_genes, 5), dtype=torch.float64, device=self.device)
        self.n = 0
        return self

    def _refuse(self, why):
        c = self.counts
        raise ValueError("ExpressionMetrics: a batch must hold distinct storage rows of the bound arrays %s (rows 0 .. %d of the "
                         "storage): %s" % (c.arrays, self._map.pos.numel() - 1, why))

    def update(self, z, rows):
        c, m, G = self.counts, self._map, self.counts.n_genes
        if c.device is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ExpressionMetrics.update is eager by contract: it was called inside a stream capture")
        if not same_device(self.device, z.device):
            raise ValueError("ExpressionMetrics: z is on %s, the counts are on %s" % (z.device, self.device))
        if z.dim() != 2 or z.shape[1] != G:
            raise ValueError("ExpressionMetrics: z must be (B, %d), one column per selected gene, got %s" % (G, tuple(z.shape)))
        want = 'float32' if c.device is not None else 'floating point'
        if not z.is_floating_point() or (c.device is not None and z.dtype != _F32):
            raise ValueError("ExpressionMetrics: z must be %s with the counts on %s, got %s" % (want, self.device, z.dtype))
        B = z.shape[0]
        if rows.dim() != 1 or rows.dtype not in (_I32, _I64) or rows.numel() != B:
            raise ValueError("ExpressionMetrics: rows must be an int64 or int32 tensor (%d,), got %s %s" % (B, rows.dtype,
                                                                                                          tuple(rows.shape)))
        if rows.device.type != 'cpu' and not same_device(self.device, rows.device):
            raise ValueError("ExpressionMetrics: rows are on %s, the counts are on %s" % (rows.device, self.device))
        if B == 0:
            return self
        z = z.detach()
        touched = None                                                               # None: every bound array
        if rows.device.type == 'cpu':
            r = rows.numpy().astype(np.int64)
            if self.check_rows:
                if not bool(m.in_view(rows)[0]):
                    self._refuse("a row outside the storage or of another array has no target here")
                if len(np.unique(r)) != B:
                    self._refuse("a repeated row would lose its sparse terms while its prediction is counted twice")
            if c.device is None:
                return self._update_host(z, r)
            touched = set((np.searchsorted(c._s.row_start, r, side='right') - 1).tolist())   # only the arrays the batch touches
            pos = m.fill(rows.to(self.device))
        else:
            if self.check_rows:
                ok, safe = m.in_view(rows)
                pos = m.fill(safe)
                if not bool(ok & m.distinct(safe, pos)):                             # the one 1-byte read-back
                    self._refuse("a repeated row, a row outside the storage or a row of an unbound array was given")
            else:
                pos = m.fill(rows)
        z, ldz = GF._rows(z)
        act = L.CONSTANTS['GNX_ACT_SIGMOID' if self.activation == 'sigmoid' else 'GNX_ACT_NONE']
        M = self.table
        L.call('gnx_act_col_moments_f64', L.ptr(z), ldz, B, G, act, L.ptr(M, torch.float64), M.stride(0), 1, L.stream())
        for _, a, trio, r0 in c.bound_csc():
            if touched is None or a in touched:
                L.call('gnx_sparse_pred_moments_f64', *trio_ptrs(trio), L.ptr(c.gene_lines(), _I32), G, L.ptr(pos[r0:], _I32),
                       L.ptr(self.gene_scale), L.ptr(z), ldz, act, L.ptr(M, torch.float64), M.stride(0), 1, L.stream())
        self.n += B
        return self

    def _update_host(self, z, r):
        z64 = z.double().numpy()
        if self.activation == 'sigmoid':
            with np.errstate(over='ignore'):
                e = np.exp(-np.abs(z64))
            p = np.where(z64 >= 0, 1.0 / (1.0 + e), e / (1.0 + e))                   # the two-branch form of the kernel
        else:
            p = z64
        T = self.counts.host_csr(r)
        if self.gene_scale is not None:
            T = T.multiply(self.gene_scale.numpy()[None, :]).astype(np.float32)    # the fp32 product
        T = T.tocsr().astype(np.float64)
        M = self.table.numpy()
        M[:, 0] += p.sum(0)
        M[:, 1] += (p * p).sum(0)
        M[:, 2] += np.asarray(T.sum(0)).ravel()
        M[:, 3] += np.asarray(T.multiply(T).sum(0)).ravel()
        M[:, 4] += np.asarray(T.multiply(p).sum(0)).ravel()
        self.n += len(r)
        return self

    def compute(self):
        M, n, G = self.table.cpu().numpy(), self.n, self.counts.n_genes
        nan = np.full(G, np.nan)
        if n == 0:
            return dict(n=0, mean_pred=nan, mean_target=nan.copy(), mse=nan.copy(), pearson=nan.copy(), r2=nan.copy(),
                        loss=float('nan'))
        sp, spp, st, stt, spt = (M[:, k] for k in range(5))
        mp, mt = sp / n, st / n
        floor = 8.0 * n * 2.0 ** -53
        var_p, var_t = spp / n - mp * mp, stt / n - mt * mt
        var_p = np.where(var_p <= floor * (spp / n), 0.0, var_p)
        var_t = np.where(var_t <= floor * (stt / n), 0.0, var_t)
        mse = (spp - 2.0 * spt + stt) / n
        with np.errstate(divide='ignore', invalid='ignore'):
            pearson = np.where((var_p > 0) & (var_t > 0), (spt / n - mp * mt) / np.sqrt(var_p * var_t), np.nan)
            r2 = np.where(var_t > 0, 1.0 - mse / var_t, np.nan)
        return dict(n=n, mean_pred=mp, mean_target=mt, mse=mse, pearson=pearson, r2=r2, loss=float(mse.mean()) if G else float('nan'))

    def top_genes(self, k, by='pearson'):
        """int64 numpy array: the k best channels by 'pearson' or 'r2' (largest first) or 'mse' (smallest first), NaNs last,
        ties broken by index."""
        if by not in ('pearson', 'r2', 'mse'):
            raise ValueError("by must be 'pearson', 'r2' or 'mse', got %r" % (by,))
        v = self.compute()[by]
        nan = np.isnan(v)
        key = np.where(nan, 0.0, v if by == 'mse' else -v)
        return np.lexsort((np.arange(len(v)), key, nan))[:int(k)].astype(np.int64)


def evaluate_expression(model, dataloader, metrics):
    """One evaluation pass: `metrics` (an ExpressionMetrics) is reset, then updated with model(patches) and rows for every
    batch (patches, rows, labels) of `dataloader` - the batches of `training.train_expression`, labels ignored - in eval() mode
    under no_grad, on the device the metrics live on.  The model's mode is restored afterwards.  Returns metrics.compute()."""
    was_training = model.training
    model.eval()
    metrics.reset()
    try:
        with torch.no_grad():
            for patches, rows, _ in dataloader:
                metrics.update(model(patches.to(metrics.device)), rows)
    finally:
        model.train(was_training)
    return metrics.compute()


class ExpressionNet(nn.Module):
    """backbone, then nn.Linear(F, n_genes): patches -> z (B, n_genes), the PRE-activation the criterion takes.  `backbone`
    maps a batch of patches to (B, F) features - a `DenseNet(classify=False)` (F = 1024 for DenseNet-121), or any module; F is
    read from `backbone.num_features` / `.out_features` or given as `in_features`.  The head is evaluated through
    `functional.linear` on a HIP device.  `set_input_transform` is forwarded to a DenseNet backbone."""

    def __init__(self, backbone, n_genes, in_features=None):
        super().__init__()
        if in_features is None:
            for name in ('num_features', 'out_features'):
                if isinstance(getattr(backbone, name, None), int):
                    in_features = getattr(backbone, name)
                    break
        if in_features is None and hasattr(backbone, 'classifier') and isinstance(backbone.classifier, nn.Linear):
            in_features = backbone.classifier.in_features
        if in_features is None:
            raise ValueError("ExpressionNet: give in_features=, the width of the backbone's output")
        self.backbone = backbone
        self.head = nn.Linear(int(in_features), int(n_genes))

    def set_input_transform(self, compose):
        self.backbone.set_input_transform(compose)
        return self

    def forward(self, patches):
        h = self.backbone(patches)
        if h.dim() != 2 or h.shape[1] != self.head.in_features:
            raise ValueError("ExpressionNet: the backbone returned %s, the head takes (B, %d)" % (tuple(h.shape), self.head.in_features))
        if h.is_cuda:
            return GF.linear(h, self.head.weight, self.head.bias)
        return self.head(h)
