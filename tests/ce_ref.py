"""Float64 restatement of the masked cross-entropy with options (gnx_masked_ce_opt_* of csrc/masked_ce.hip), written out from
the formulas of include/gridnext_hip.h (test_ce_ref_host.py proves it against torch in float64, test_gpu_masked_ce_forms.py
uses it as the reference).  Not imported by the package; no torch.nn.functional.cross_entropy in here.

A row is selected iff label >= label_base, its class is y = label - label_base; a selected row with y == ignore_index is ignored.
With lp = log_softmax(z), class weights w (ones when None), smoothing e and S = the selected, not ignored rows:
  num  = sum_{i in S} [ (1-e) w[y_i] (-lp[i,y_i]) + (e/C) sum_c w[c] (-lp[i,c]) ]
  den  = sum_{i in S} w[y_i]  ('mean')  |  1  ('sum')
  loss = num / den / accum_iters
  dz[i,c] = (p[i,c] a_i - t[i,c]) dloss / (den accum_iters) on S, 0 elsewhere
            a_i = (1-e) w[y_i] + (e/C) sum_c w[c],   t[i,c] = (1-e) w[y_i] [c == y_i] + (e/C) w[c]
  stats = (n_selected, n_correct), preds = first maximal index: independent of w, e and ignore_index.
"""
from types import SimpleNamespace as NS

import numpy as np
import torch

NAN = float('nan')


def masked_ce(z, labels, label_base=1, weight=None, label_smoothing=0.0, ignore_index=-100, reduction='mean', accum_iters=1,
              dloss=1.0):
    """z [M][C] of any float type, labels [M] (or any shape of M entries) integers.  Everything in float64."""
    assert reduction in ('mean', 'sum')
    z = z.detach().double()
    M, C = z.shape
    lab = labels.reshape(-1).long()
    e = float(label_smoothing)
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.detach().double()
    preds = torch.from_numpy(np.argmax(z.numpy(), axis=1))                 # numpy: the FIRST maximal index
    selected = lab >= label_base
    y = lab - label_base
    live = selected & (y != ignore_index)
    bad = live & (y >= C)                                                  # a caller error: poisons the loss, reads nothing
    yc = y.clamp(0, C - 1)
    mx = z.max(1, keepdim=True).values
    lse = mx + (z - mx).exp().sum(1, keepdim=True).log()
    nlp = lse - z                                                          # -log_softmax
    p = (-nlp).exp()
    wy = w[yc]
    onehot = torch.zeros(M, C, dtype=torch.float64)
    onehot[torch.arange(M), yc] = 1.0
    row = (1 - e) * wy * nlp[torch.arange(M), yc]
    if e != 0.0:                                                           # (e = 0 never touches the other classes' -lp)
        row = row + (e / C) * (nlp * w).sum(1)
    num = row[live].sum()
    den = wy[live].sum() if reduction == 'mean' else torch.tensor(1.0, dtype=torch.float64)
    loss = num / den / accum_iters
    a = (1 - e) * wy + (e / C) * w.sum()
    t = (1 - e) * wy[:, None] * onehot + (e / C) * w[None, :]
    dz = (p * a[:, None] - t) * (dloss / (den * accum_iters))
    dz = torch.where(live[:, None], dz, torch.zeros_like(dz))
    if bad.any():
        loss = loss * NAN
        dz[bad] = NAN
        if reduction == 'mean':
            dz[live] = NAN
    n_correct = int((selected & (preds == y)).sum())
    return NS(loss=loss, dz=dz, den=den, stats=(int(selected.sum()), n_correct), preds=preds, selected=selected, live=live)


# ------------------------------------------------------------------------------------------------------------ inputs
def case(M, C, label_base, seed=0, ignore_index=-100):
    """(z float32 [M][C], labels int64 [M]) of one case: logits N(0, 2^2); labels uniform over label_base - 1 .. label_base + C - 1
    (for label_base 1 that includes the background 0; for label_base 0 the -1 is dropped: every row counts, as in the spot
    loop).  With an ignore_index inside the class range the first and the last row carry it (where M allows), so that an
    ignored row sits at both ends of the block range."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * M + C)
    z = (2.0 * torch.randn(M, C, generator=g, dtype=torch.float64)).float()
    lab = torch.randint(label_base - 1 if label_base else 0, label_base + C, (M,), generator=g)
    if 0 <= ignore_index < C and M >= 3:
        lab[0] = lab[M - 1] = ignore_index + label_base
    return z, lab


def weights(kind, C, seed=0):
    """None | 'rand': U(0.1, 1.1) float32 | 'zero': the same with class C // 2 set to 0."""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(104729 * seed + C)
    w = (0.1 + torch.rand(C, generator=g, dtype=torch.float64)).float()
    if kind == 'zero':
        w[C // 2] = 0.0
    return w


WEIGHTS = (None, 'rand', 'zero')
SMOOTHINGS = (0.0, 0.1, 1.0)
IGNORES = (-100, 3)
REDUCTIONS = ('mean', 'sum')
ACCUMS = (1, 3)


def ulp32(v):
    """One float32 unit in the last place at magnitude |v|."""
    return float(np.spacing(np.float32(abs(float(v)))))
