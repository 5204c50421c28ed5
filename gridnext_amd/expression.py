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
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as GF
from .sparse_linear import _host_rows, _same_device, bound_rows, rows_in_view
from .visium_datasets import SpotCounts

_I32, _I64, _F32 = torch.int32, torch.int64, torch.float32


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
    (`sparse_linear.rows_in_view`, the check SparseCountLinear makes); `check_rows=False` skips it.

    Raises ValueError, naming what differs: z elsewhere than on the CPU, a width that is not counts.n_genes, a z that is not
    floating point.  Counts on a HIP device raise RuntimeError at construction: the criterion has no device form yet, and it
    does not run the composition there in its place."""

    def __init__(self, counts, activation='sigmoid', gene_scale=None, reduction='mean', check_rows=True):
        super().__init__()
        if not isinstance(counts, SpotCounts):
            raise TypeError("counts must be a SpotCounts, got %s" % type(counts).__name__)
        if activation not in ('sigmoid', None):
            raise ValueError("activation must be 'sigmoid' or None, got %r" % (activation,))
        if reduction not in ('mean', 'sum'):
            raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
        if counts.device is not None:
            raise RuntimeError("SparseMSELoss: the counts are on %s; the criterion has no device form yet and does not run torch's "
                               "composition there in its place - bind it to the counts on the host (SpotCounts.to(None))"
                               % counts.device)
        self.counts, self.activation, self.reduction, self.check_rows = counts, activation, reduction, bool(check_rows)
        if gene_scale is not None:
            gene_scale = torch.as_tensor(gene_scale).detach().to(device='cpu', dtype=_F32).contiguous()
            if gene_scale.shape != (counts.n_genes,):
                raise ValueError("gene_scale must be (%d,), one per selected gene, got %s" % (counts.n_genes, tuple(gene_scale.shape)))
        self.register_buffer('gene_scale', gene_scale, persistent=False)
        self.register_buffer('_bound', torch.from_numpy(bound_rows(counts)), persistent=False)

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
        if not _same_device('cpu', z.device):
            raise ValueError("SparseMSELoss: z is on %s, the counts are on cpu" % z.device)
        if z.dim() != 2 or z.shape[1] != c.n_genes:
            raise ValueError("SparseMSELoss: z must be (B, %d), one column per selected gene, got %s" % (c.n_genes, tuple(z.shape)))
        if not z.is_floating_point():
            raise ValueError("SparseMSELoss: z must be floating point, got %s" % z.dtype)
        if rows.dim() != 1 or rows.dtype not in (_I32, _I64) or rows.numel() != z.shape[0]:
            raise ValueError("SparseMSELoss: rows must be an int64 or int32 tensor (%d,), got %s %s" % (z.shape[0], rows.dtype,
                                                                                                      tuple(rows.shape)))
        rows = rows.cpu()
        if self.check_rows and rows.numel() and not bool(rows_in_view(rows, self._bound.cpu())[0]):
            raise ValueError("SparseMSELoss: the rows must be storage rows of the bound arrays %s (rows 0 .. %d of the storage, those "
                             "of the bound arrays only): a row outside the storage or of another array has no target here"
                             % (c.arrays, self._bound.numel() - 1))
        target = torch.from_numpy(_host_rows(c, rows.numpy().astype(np.int64), np.float32).toarray()).to(z.dtype)
        if self.gene_scale is not None:
            target = target * self.gene_scale.to(device='cpu', dtype=z.dtype)
        return F.mse_loss(self.activate(z), target, reduction=self.reduction)


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
