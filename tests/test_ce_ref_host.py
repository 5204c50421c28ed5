"""tests/ce_ref.py proved before test_gpu_masked_ce_forms.py uses it as the reference: against torch.nn.functional.cross_entropy
in float64 under autograd (loss and gradient, <= 1e-12) over the option grid of the GPU file, plus the statements the kernel tests
rely on (stats, first-argmax, NaN / zero of the empty reductions).  Runs on the CPU."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import ce_ref as R

torch.set_num_threads(1)


def _torch_ce(z, lab, label_base, w, e, ignore_index, reduction, accum_iters, dloss, dtype=torch.float64):
    """The generic loop's chain: gather the selected rows, shift the labels, F.cross_entropy, / accum_iters; gradient w.r.t. ALL rows."""
    zt = z.to(dtype).requires_grad_(True)
    keep = lab >= label_base
    loss = F.cross_entropy(zt[keep], lab[keep] - label_base, weight=None if w is None else w.to(dtype),
                           ignore_index=ignore_index, reduction=reduction, label_smoothing=e) / accum_iters
    (loss * dloss).backward()
    return loss.detach(), zt.grad


GRID = list(itertools.product(R.WEIGHTS, R.SMOOTHINGS, R.IGNORES, R.REDUCTIONS))


@pytest.mark.parametrize("M,C,label_base", [(1, 8, 0), (7, 1, 1), (7, 2, 0), (257, 8, 1), (300, 65, 1), (40, 5, 0)])
def test_ref_equals_float64_cross_entropy(M, C, label_base):
    for k, (wk, e, ign, red) in enumerate(GRID):
        accum, dloss = R.ACCUMS[k % 2], (1.0, 0.37)[(k // 2) % 2]
        z, lab = R.case(M, C, label_base, seed=k, ignore_index=ign)
        if M == 1:
            lab[0] = label_base + C - 1                                   # (one row: a selected one)
        w = R.weights(wk, C, seed=k)
        what = "M %d C %d base %d w %s e %g ignore %d %s accum %d" % (M, C, label_base, wk, e, ign, red, accum)
        r = R.masked_ce(z, lab, label_base, w, e, ign, red, accum, dloss)
        loss, dz = _torch_ce(z, lab, label_base, w, e, ign, red, accum, dloss)
        if math.isnan(loss.item()):                                       # 'mean' over rows of zero total weight: 0 / 0 in both
            assert red == 'mean' and r.den.item() == 0.0 and math.isnan(r.loss.item()), what
            continue
        assert abs(r.loss.item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item())), what
        assert (r.dz - dz).abs().max().item() <= 1e-12 * max(1.0, dz.abs().max().item()), what
        assert (r.dz[~r.live] == 0).all(), what
        # stats and preds are the generic loop's: flat.numel(), sum(argmax == flat) - whatever the options
        keep = lab >= label_base
        assert r.stats == (int(keep.sum()), int((torch.max(z[keep].double(), 1)[1] == lab[keep] - label_base).sum())), what
        assert torch.equal(r.preds, z.double().argmax(1)), what


def test_ref_case_grid_has_ignored_and_background_rows():
    z, lab = R.case(513, 8, 1, ignore_index=3)
    r = R.masked_ce(z, lab, 1, None, 0.0, 3)
    assert (~r.selected).any() and (r.selected & ~r.live).sum() >= 2 and not r.live[0] and not r.live[512]
    assert r.stats[0] == int(r.selected.sum()) > int(r.live.sum())


def test_ref_first_maximal_index():
    z = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]])
    r = R.masked_ce(z, torch.tensor([2, 1, 4]), 1)
    assert r.preds.tolist() == [1, 0, 2] and r.stats == (3, 2)


@pytest.mark.parametrize("reduction", R.REDUCTIONS)
def test_ref_empty_reductions(reduction):
    z, lab = R.case(20, 5, 1)
    w = R.weights('zero', 5)
    none = R.masked_ce(z, torch.zeros_like(lab), 1, w, 0.1, -100, reduction)                     # nothing selected
    ignored = R.masked_ce(z, torch.full_like(lab, 4), 1, w, 0.1, 3, reduction)                   # everything ignored
    zero_w = R.masked_ce(z, torch.full_like(lab, 5 // 2 + 1), 1, w, 0.0, -100, reduction)        # only the zero-weight class
    if reduction == 'mean':
        assert all(math.isnan(r.loss.item()) for r in (none, ignored, zero_w))
    else:
        assert none.loss.item() == 0.0 and ignored.loss.item() == 0.0 and zero_w.loss.item() == 0.0
    assert (none.dz == 0).all() and (ignored.dz == 0).all()
    assert none.stats[0] == 0 and ignored.stats[0] == 20 and zero_w.stats[0] == 20
    # torch agrees on the selected-but-ignored case (an empty gather it cannot even index)
    loss, _ = _torch_ce(z, torch.full_like(lab, 4), 1, w, 0.1, 3, reduction, 1, 1.0)
    assert math.isnan(loss.item()) if reduction == 'mean' else loss.item() == 0.0


def test_ref_class_index_past_c_is_nan():
    z, lab = R.case(20, 5, 1)
    lab[7] = 6 + 1
    for reduction in R.REDUCTIONS:
        r = R.masked_ce(z, lab, 1, R.weights('rand', 5), 0.1, -100, reduction)
        assert math.isnan(r.loss.item()) and torch.isnan(r.dz[7]).all() and (r.dz[~r.live] == 0).all()


def test_ulp32():
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(-0.75) == 2.0 ** -24 and R.ulp32(3.0) == 2.0 ** -22
