"""Evaluation and coordinate helpers of the f∘g path.

Mirrors the parts of /root/reference/gridnext/utils.py that sit on (or right next to) the hot path:
  * `all_fgd_predictions` (:20-57): forward every array, keep foreground spots, return (true, argmax, softmax).
    Here the forward runs on the HIP kernels and the softmax/argmax is one fused kernel on channels-last logits;
    list inputs (GridNetHexMM) are supported - the reference's helper crashes on them (`x.to(device)` at :29);
    `all_fgd_predictions_device` is the same walk with the three results left on the device (for `gridnext_amd.metrics`);
  * the Visium coordinate maps (:64-85).
`patch_saliency` has no counterpart there: input-gradient saliency maps of a spot classifier on the HIP path.
`to_loupe_annots` (:169-193) writes a label grid back as a Loupe annotation file.
The other file readers live in count_datasets.py, imgprocess.py and visium_datasets.py.
"""
import numpy as np
import torch

from . import _lib as L
from . import distributed as gdist


def softmax_argmax_rows(rows):
    """(probs [M, C], preds [M]) of channels-last logits [M, C] on a HIP device."""
    rows = rows.contiguous()
    M, C = rows.shape
    probs = torch.empty((M, C), device=rows.device, dtype=torch.float32)
    preds = torch.empty(M, device=rows.device, dtype=torch.int64)
    L.call('gnx_softmax_rows', L.ptr(rows), C, M, C, L.ptr(probs), C, L.ptr(preds, torch.int64), L.stream())
    return probs, preds


def all_fgd_predictions(dataloader, model, f_only=False):
    """Flattened predictions for all foreground spots: (true_vals, pred_vals, pred_smax)."""
    true_vals, pred_vals, pred_smax = [], [], []
    device = gdist.default_device()
    model.to(device)
    model.eval()
    for x, y in dataloader:
        x = [t.to(device) for t in x] if isinstance(x, (list, tuple)) else x.to(device)
        y = y.to(device)
        with torch.no_grad():
            if f_only:
                outputs = model.patch_predictions(x).permute(0, 2, 3, 1)
            elif hasattr(model, 'forward_nhwc'):
                outputs = model.forward_nhwc(x)
            else:
                outputs = model(x).permute(0, 2, 3, 1)
            rows = outputs.reshape(-1, outputs.shape[-1])
            labels = y.reshape(-1)
            if rows.is_cuda:
                probs, preds = softmax_argmax_rows(rows)
            else:                                   # a CPU model handed in by the caller: spell the reference out
                probs, preds = torch.softmax(rows, dim=1), torch.argmax(rows, dim=1)
            keep = (labels > 0).cpu()
            true_vals.append((labels.cpu()[keep] - 1).numpy())
            pred_vals.append(preds.cpu()[keep].numpy())
            pred_smax.append(probs.cpu()[keep].numpy())
    return np.concatenate(true_vals), np.concatenate(pred_vals), np.concatenate(pred_smax)


def all_fgd_predictions_device(dataloader, model, f_only=False):
    """`all_fgd_predictions` with the results left where they were computed: (true_vals int64 [M], pred_vals int64 [M],
    pred_smax float32 [M, C]) as tensors on the device, the foreground selection done there too, for `gridnext_amd.metrics`.
    The same walk and the same values; a run's evaluation never leaves the device."""
    true_vals, pred_vals, pred_smax = [], [], []
    device = gdist.default_device()
    model.to(device)
    model.eval()
    for x, y in dataloader:
        x = [t.to(device) for t in x] if isinstance(x, (list, tuple)) else x.to(device)
        y = y.to(device)
        with torch.no_grad():
            if f_only:
                outputs = model.patch_predictions(x).permute(0, 2, 3, 1)
            elif hasattr(model, 'forward_nhwc'):
                outputs = model.forward_nhwc(x)
            else:
                outputs = model(x).permute(0, 2, 3, 1)
            rows = outputs.reshape(-1, outputs.shape[-1])
            labels = y.reshape(-1)
            if rows.is_cuda:
                probs, preds = softmax_argmax_rows(rows)
            else:                                   # a CPU model handed in by the caller: spell the reference out
                probs, preds = torch.softmax(rows, dim=1), torch.argmax(rows, dim=1)
            keep = (labels > 0).nonzero().reshape(-1)
            true_vals.append(labels.index_select(0, keep) - 1)
            pred_vals.append(preds.index_select(0, keep))
            pred_smax.append(probs.index_select(0, keep))
    return torch.cat(true_vals), torch.cat(pred_vals), torch.cat(pred_smax)


def patch_saliency(classifier, patches, targets=None):
    """Saliency maps of a spot classifier: (N, P, P) float32, the maximum over the colour channels of
    |d logit[target] / d patch| for every patch of `patches` (N, 3, P, P).  `targets`: (N,) int64 class indices, by default
    the classifier's own argmax.  The classifier runs in eval mode (every submodule's own previous mode is restored on exit)
    and is differentiated with respect to the patches only: afterwards every parameter's `.grad` and `requires_grad` and
    every buffer are what they were.  A `gridnext_amd.DenseNet` inside it forms no parameter gradient during the call and
    hands none to a data-parallel reducer, whatever its parameters' `requires_grad` says.  uint8 patches are first converted by the classifier's own ToTensor (+ Normalize) pass
    (`DenseNet._float_patches`); the gradient is with respect to those floats.  A DenseNet with `input_resize` / `input_crop`
    set resizes the stored uint8 patches in that same pass: the maps are then (N, Ph, Pw), the saliency of the resized patches.  Any module that is differentiable in its
    input will do - a `gridnext_amd.DenseNet` (its input gradient is `gnx_conv0_dgrad`), or one behind other layers."""
    resized = None        # the classifier whose input transform already ran in `_float_patches`: off during the call
    if patches.dtype == torch.uint8:
        to_float = getattr(classifier, '_float_patches', None)
        if to_float is None:
            raise TypeError("patch_saliency: uint8 patches need a classifier with its own conversion to float "
                            "(gridnext_amd.DenseNet); pass float patches to %s" % type(classifier).__name__)
        patches = to_float(patches)
        if getattr(classifier, '_input_transform_set', lambda: False)():
            resized = (classifier, classifier.input_resize, classifier.input_crop)
    x = patches.detach().float().requires_grad_(True)
    params = list(classifier.parameters())
    held = [p.grad for p in params]       # a checkpointed classifier accumulates into .grad from inside its backward
    modes = [(mod, mod.training) for mod in classifier.modules()]
    from .densenet import DenseNet
    nets = [mod for mod, _ in modes if isinstance(mod, DenseNet)]
    classifier.eval()
    try:
        for p in params:
            p.grad = None
        for net in nets:
            net.__dict__['_input_grad_only'] = True          # densenet_train._Grads: the input's gradient alone
        if resized is not None:
            classifier.input_resize = classifier.input_crop = None
        with torch.enable_grad():
            out = classifier(x)
            if targets is None:
                targets = out.detach().argmax(1)
            picked = out.gather(1, targets.to(out.device).reshape(-1, 1)).sum()    # eval mode: spots are independent
            grad, = torch.autograd.grad(picked, x)
    finally:
        if resized is not None:
            resized[0].input_resize, resized[0].input_crop = resized[1:]
        for net in nets:
            net.__dict__.pop('_input_grad_only', None)
        for p, g in zip(params, held):
            p.grad = g
        for mod, was_training in modes:
            mod.training = was_training
    return grad.abs().amax(1)


def to_loupe_annots(annot_tensor, position_file, output_file, annot_names=None, zero_bg=True):
    """Write a Loupe annotation CSV (Barcode,AARs) for one array from a label grid (reference utils.py:169-193): for every
    in-tissue spot of `position_file`, in its order, the label at the spot's odd-right cell minus one when zero_bg (0 is
    background: an empty annotation); `annot_names[label]` when names are given, else the integer.  annot_tensor: (h, w) after
    squeeze, any device."""
    import pandas as pd
    from .imgprocess import visium_get_positions_fromfile
    positions = visium_get_positions_fromfile(position_file)
    grid = torch.as_tensor(annot_tensor).detach().cpu().squeeze().numpy()
    barcodes, annotations = [], []
    for barcode, ent in positions.iterrows():
        if not ent['in_tissue']:
            continue
        x, y = pseudo_hex_to_oddr(int(ent['array_col']), int(ent['array_row']))
        a = int(grid[y, x]) - int(zero_bg)
        annotations.append('' if a < 0 else (annot_names[a] if annot_names is not None else a))
        barcodes.append(barcode)
    pd.DataFrame({'Barcode': barcodes, 'AARs': annotations}).to_csv(output_file, sep=',', index=False)


# ---- Visium coordinate maps (reference utils.py:64-85) ---------------------------------------------------------------
def pseudo_hex_to_oddr(col, row):
    """Visium pseudo-hex (col doubles along a row) -> odd-right (col, row)."""
    return int((col - (row % 2)) / 2), int(row)


def oddr_to_pseudo_hex(col, row):
    return int(2 * col + (row % 2)), int(row)


def pseudo_to_true_hex(col, row):
    """Cartesian centre with unit distance between neighbouring spots."""
    return col / 2, row * np.sqrt(3) / 2
