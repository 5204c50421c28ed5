"""CPU: how the training loops classify a criterion (training._fused_ce) - plain, fused-opt or generic - and that the loops on
CPU tensors compute a criterion with options as torch does (they take the generic path there whatever the classification)."""
import contextlib
import io

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

torch.set_num_threads(1)
CPU = torch.device('cpu')


class SameCE(nn.CrossEntropyLoss):
    pass


def test_classification():
    from gridnext_amd import functional as GF, training
    w = torch.tensor([0.5, 1.0, 2.0])
    assert training._fused_ce(nn.CrossEntropyLoss(), CPU) is GF.masked_cross_entropy
    for crit in (nn.CrossEntropyLoss(weight=w), nn.CrossEntropyLoss(label_smoothing=0.1), nn.CrossEntropyLoss(ignore_index=1),
                 nn.CrossEntropyLoss(reduction='sum'), nn.CrossEntropyLoss(weight=w, ignore_index=0, reduction='sum', label_smoothing=1.0)):
        ce = training._fused_ce(crit, CPU)
        assert ce is not None and ce is not GF.masked_cross_entropy
    for crit in (SameCE(), SameCE(weight=w), nn.CrossEntropyLoss(reduction='none'), nn.CrossEntropyLoss(weight=w.double()),
                 nn.CrossEntropyLoss(weight=w.repeat(2)[::2]), nn.CrossEntropyLoss(weight=w.view(3, 1)), nn.NLLLoss(), nn.MSELoss()):
        assert training._fused_ce(crit, CPU) is None
    assert training._fused_ce(nn.CrossEntropyLoss(weight=w), torch.device('meta')) is None        # a weight on another device


def test_options_are_read_once_and_the_weight_in_place(monkeypatch):
    from gridnext_amd import functional as GF, training
    w = torch.tensor([0.5, 1.0, 2.0])
    crit = nn.CrossEntropyLoss(weight=w, ignore_index=1, label_smoothing=0.25, reduction='sum')
    seen = []
    monkeypatch.setattr(GF, 'masked_cross_entropy_opt', lambda *a: seen.append(a) or 'out')
    ce = training._fused_ce(crit, CPU)
    crit.label_smoothing, crit.ignore_index = 0.5, 2                       # (after the train_* call read them)
    assert ce('rows', 'labels', 3, label_base=0) == 'out'
    (rows, labels, accum, base, weight, e, ign, red), = seen
    assert (rows, labels, accum, base, e, ign, red) == ('rows', 'labels', 3, 0, 0.25, 1, 'sum') and weight is w


def test_cpu_loop_with_options_is_torchs(monkeypatch):
    """train_spotwise on CPU tensors with a weighted, smoothed criterion: the epoch losses are those of the same criterion
    applied by hand (the fused kernels need a HIP device; nothing is called there)."""
    import gridnext_amd as ga
    gen = torch.Generator().manual_seed(2)
    x, y = torch.randn(24, 6, generator=gen), torch.randint(0, 3, (24,), generator=gen)
    crit = nn.CrossEntropyLoss(weight=torch.tensor([0.5, 1.0, 2.0]), label_smoothing=0.1)
    torch.manual_seed(1)
    f = nn.Sequential(nn.Linear(6, 3))
    with torch.no_grad():
        want = sum(crit(f(x[i:i + 8]), y[i:i + 8]).item() * 8 for i in (0, 8, 16)) / 24
    dl = {'train': DataLoader(TensorDataset(x, y), batch_size=8), 'val': DataLoader(TensorDataset(x, y), batch_size=8)}
    monkeypatch.setattr(ga.training.gdist, 'default_device', lambda: CPU)
    with contextlib.redirect_stdout(io.StringIO()):
        _, vh, th = ga.train_spotwise(f, dl, crit, torch.optim.SGD(f.parameters(), lr=0.0), num_epochs=1)
    np.testing.assert_allclose([th[0], vh[0]], [want, want], rtol=1e-6)
