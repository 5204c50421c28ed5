"""The first Linear layer of a count classifier over sparse rows (csrc/sparse_linear.hip): the layer that ends the sparse-count
path of visium_datasets.py.  The tutorial's count MLP (Tutorial_visium_count.ipynb cell 12) starts with nn.Linear(G, 500) on a
densified spot; here the layer is handed storage ROW INDICES of a `SpotCounts` and multiplies the stored entries alone:

    forward      out[b] = bias + sum over the stored entries (g, x) of row rows[b] of x * weight[channel(g)]     (CSR)
    weight.grad  dW[c]  = sum over the arrays of the bound view, in view order, over the stored entries (r, x) of gene c in
                          storage row order, of x * dY[position of r in the batch]                               (CSCs)
    bias.grad    the column sums of dY (gnx_colsum)

Nothing of B x G floats is written, saved on the tape or read back; the weight is gene-major, (G, out_features): the transpose
of nn.Linear.weight.  With the counts on the host (device None) the module runs a scipy restatement on the CPU, autograd
included.  There is no input gradient: the input is an index list.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib as L
from . import functional as GF
from .visium_datasets import RowMap, SpotCounts, _refuse_worker, same_device, trio_ptrs

_I32, _I64, _F32 = torch.int32, torch.int64, torch.float32


def _forward_lines(layer, lines, weight, bias):
    """(len(lines), F): bias + the sparse rows `lines` (int32 tensor on the weight's device; -1: no row) times `weight`."""
    c = layer.counts
    n, F = lines.numel(), weight.shape[1]
    if weight.is_cuda:
        w = weight.contiguous()
        out = torch.empty((n, F), dtype=_F32, device=w.device)
        L.call('gnx_sparse_linear_fwd_f32', *trio_ptrs(c._s.csr), L.ptr(lines, _I32), n, L.ptr(c.gene_channel(), _I32), L.ptr(w),
               w.stride(0), L.ptr(bias), L.ptr(out), F, F, L.stream())
        return out
    ln = lines.numpy().astype(np.int64)
    has = ln >= 0
    out = np.zeros((n, F), dtype=weight.numpy().dtype)
    out[has] = c.host_csr(ln[has], out.dtype) @ weight.numpy()
    if bias is not None:
        out += bias.numpy()
    return torch.from_numpy(out)


class _SparseLinear(Function):
    """rows (B,) int32 storage rows -> (B, F).  Saves the rows alone."""

    @staticmethod
    def forward(ctx, rows, weight, bias, layer):
        ctx.layer, ctx.has_bias = layer, bias is not None
        ctx.save_for_backward(rows)
        return _forward_lines(layer, rows, weight.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, dy):
        rows, = ctx.saved_tensors
        layer = ctx.layer
        c = layer.counts
        G = c.n_genes
        dw = db = None
        if not dy.is_cuda:
            d = dy.numpy()
            if ctx.needs_input_grad[1]:
                dw = torch.from_numpy(np.ascontiguousarray(c.host_csr(rows.numpy().astype(np.int64), d.dtype).T @ d))
            if ctx.has_bias and ctx.needs_input_grad[2]:
                db = torch.from_numpy(d.sum(0))
            return None, dw, db, None
        dy, lddy = GF._rows(dy)
        B, F = dy.shape
        if ctx.needs_input_grad[1]:
            pos = layer._map.fill(rows)
            dw = torch.empty((G, F), dtype=_F32, device=dy.device)
            if not c._arrays:
                dw.zero_()
            for k, _, trio, r0 in c.bound_csc():
                L.call('gnx_sparse_linear_wgrad_f32', *trio_ptrs(trio), L.ptr(c.gene_lines(), _I32), G, L.ptr(pos[r0:], _I32),
                       L.ptr(dy), lddy, L.ptr(dw), F, F, 1 if k else 0, L.stream())
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = torch.empty(F, dtype=_F32, device=dy.device)
            ws = torch.empty(L.query('gnx_bn_workspace', B, F), dtype=_F32, device=dy.device)
            L.call('gnx_colsum', L.ptr(dy), lddy, B, F, L.ptr(db), 0, L.ptr(ws), L.stream())
        return None, dw, db, None


class SparseCountLinear(nn.Module):
    """nn.Linear(G, out_features) over the sparse rows of `counts` (a SpotCounts view: its gene selection, its arrays; on the
    host or resident), G = counts.n_genes.  Parameters: `weight` (G, out_features) - gene-major, the transpose of
    nn.Linear.weight - and `bias` (out_features,), initialised to what nn.Linear(G, out_features) draws from the same RNG state.

    forward(rows): rows is an int64 / int32 tensor (B,) of STORAGE row indices (`SparseCountDataset.rows`, the items of
    `SparseCountDataset(as_rows=True)`): views of one storage - a training and a validation set - share one layer.  Returns
    (B, out_features) float32 on the weight's device.  Backward gives the dense weight.grad (one launch per array of the bound
    view, in view order) and bias.grad; only `rows` is saved.

    A row repeated within a batch that takes gradients would lose a contribution to weight.grad (the row -> position map
    keeps one position per row), and a row of an array outside the bound view would lose all of its own.  With
    `check_rows=True` (the default) every forward that takes gradients verifies on the device that the rows lie inside the
    storage, belong to bound arrays and are distinct, and raises ValueError - at the cost of ONE 1-byte read-back per training
    forward, which also makes the forward illegal inside a hipGraph capture.  `check_rows=False` skips the check and the
    read-back and is capture-safe; the caller then guarantees the three conditions.  Forwards under no_grad are never checked.

    Weight and counts live on one device (or both on the host); anything else raises and names both.  On a HIP device the
    layer raises inside a DataLoader worker, as the sparse datasets do."""

    def __init__(self, counts, out_features, bias=True, check_rows=True):
        super().__init__()
        if not isinstance(counts, SpotCounts):
            raise TypeError("counts must be a SpotCounts, got %s" % type(counts).__name__)
        self.counts, self.out_features, self.check_rows = counts, int(out_features), bool(check_rows)
        self.in_features = counts.n_genes
        lin = nn.Linear(self.in_features, self.out_features, bias=bias)         # the draws of the dense layer
        self.weight = nn.Parameter(lin.weight.detach().t().contiguous())
        self.bias = nn.Parameter(lin.bias.detach().clone()) if bias else None
        self._map = RowMap(counts)                                               # storage row -> position in the batch

    def extra_repr(self):
        return 'in_features=%d, out_features=%d, bias=%s, arrays=%d' % (self.in_features, self.out_features,
                                                                        self.bias is not None, len(self.counts._arrays))

    # ---- conversions
    @classmethod
    def from_linear(cls, linear, counts, check_rows=True):
        """The layer that computes what `linear` (an nn.Linear(counts.n_genes, F)) computes on the expanded rows."""
        if linear.in_features != counts.n_genes:
            raise ValueError("the Linear takes %d features, the counts have %d genes" % (linear.in_features, counts.n_genes))
        layer = cls(counts, linear.out_features, bias=linear.bias is not None, check_rows=check_rows).to(linear.weight.device)
        with torch.no_grad():
            layer.weight.copy_(linear.weight.t())
            if linear.bias is not None:
                layer.bias.copy_(linear.bias)
        layer.weight.requires_grad = linear.weight.requires_grad
        if linear.bias is not None:
            layer.bias.requires_grad = linear.bias.requires_grad
        return layer

    def to_linear(self):
        """nn.Linear(G, F) with this layer's values (weight transposed), on the weight's device."""
        lin = nn.Linear(self.in_features, self.out_features, bias=self.bias is not None).to(self.weight.device, self.weight.dtype)
        with torch.no_grad():
            lin.weight.copy_(self.weight.t())
            if self.bias is not None:
                lin.bias.copy_(self.bias)
        return lin

    @classmethod
    def from_affine(cls, counts, weight, bias=None):
        """A FROZEN layer x -> x @ weight + bias, weight (G, k) and bias (k,) tensors or arrays.  With weight =
        pca.components_.T and bias = -pca.mean_ @ pca.components_.T it evaluates a fitted PCA on sparse counts."""
        weight = torch.as_tensor(np.asarray(weight.detach().cpu() if torch.is_tensor(weight) else weight), dtype=_F32)
        if weight.dim() != 2 or weight.shape[0] != counts.n_genes:
            raise ValueError("weight must be (%d genes, k), got %s" % (counts.n_genes, tuple(weight.shape)))
        layer = cls(counts, weight.shape[1], bias=bias is not None)
        with torch.no_grad():
            layer.weight.copy_(weight)
            if bias is not None:
                layer.bias.copy_(torch.as_tensor(np.asarray(bias.detach().cpu() if torch.is_tensor(bias) else bias), dtype=_F32))
        for p in layer.parameters():
            p.requires_grad = False
        return layer if counts.device is None else layer.to(counts.device)

    # ---- the pass
    def _where(self):
        """Checks that weight and counts live together; True on a HIP device."""
        c, w = self.counts, self.weight
        if not same_device(c.device, w.device):
            raise RuntimeError("SparseCountLinear: the weight is on %s, the counts are on %s; move the layer with .to() or the "
                               "counts with SpotCounts.to()" % (w.device, 'cpu' if c.device is None else c.device))
        _refuse_worker(c)
        return w.is_cuda

    def _check(self, rows):
        """ValueError unless the rows lie inside the storage, in bound arrays, and are distinct (one 1-byte read-back)."""
        ok, safe = self._map.in_view(rows)
        if not bool(ok & self._map.distinct(safe, self._map.fill(safe))):
            raise ValueError("SparseCountLinear: a batch that takes gradients must hold distinct storage rows of the bound arrays "
                             "%s (rows 0 .. %d of the storage): a repeated row, a row outside the storage or a row of an unbound "
                             "array would lose its contribution to weight.grad" % (self.counts.arrays, self._map.pos.numel() - 1))

    def forward(self, rows):
        self._where()
        if rows.dim() != 1 or rows.dtype not in (_I32, _I64):
            raise TypeError("rows must be an int64 or int32 tensor (B,), got %s %s" % (rows.dtype, tuple(rows.shape)))
        rows = rows.to(self.weight.device)
        takes_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if takes_grad and self.check_rows and rows.numel():
            self._check(rows)
        return _SparseLinear.apply(rows.to(_I32), self.weight, self.bias, self)

    def array_rows(self, array_name, cells, n_cells, zero_empty=False):
        """(n_cells, out_features), under no_grad, in ONE forward launch: row cells[j] is the layer's output for spot j of the
        array (`cells`: int32 tensor, spot -> cell, injective), every other row is the bias - what nn.Linear gives on the zero
        vector a dense grid holds at an empty cell - or, with zero_empty, 0.0 written over it after the launch."""
        c = self.counts
        if array_name not in c.arrays:
            raise ValueError("no array named %s among the bound %s" % (array_name, c.arrays))
        self._where()
        r0, r1 = c.array_span(c._array_ids([array_name])[0])
        dev = self.weight.device
        with torch.no_grad():
            lines = torch.full((n_cells,), -1, dtype=_I32, device=dev)
            lines[cells.to(dev).long()] = torch.arange(r0, r1, dtype=_I32, device=dev)
            out = _forward_lines(self, lines, self.weight.detach(), None if self.bias is None else self.bias.detach())
            return out.masked_fill_((lines < 0)[:, None], 0.0) if zero_empty else out


class SparseCountMLP(nn.Module):
    """A count classifier whose first layer reads sparse rows: `first` (a SparseCountLinear) then `rest` (an nn.Sequential of
    Linear / BatchNorm1d / ReLU, the tutorial MLP without its first Linear).  forward(rows) = rest(first(rows)), `rest` through
    the HIP MLP kernels (`functional.sequential_forward`) on a HIP device.  `first` is never folded into a frozen-affine plan
    of `rest`.  `train_spotwise` steps it eagerly over `SparseCountDataset(as_rows=True)`."""

    def __init__(self, first, rest):
        super().__init__()
        if not isinstance(first, SparseCountLinear):
            raise TypeError("first must be a SparseCountLinear, got %s" % type(first).__name__)
        self.first, self.rest = first, rest

    def forward(self, rows):
        h = self.first(rows)
        return GF.sequential_forward(self.rest, h) if h.is_cuda else self.rest(h)
