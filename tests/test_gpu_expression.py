"""Expression from patches on the device: `SlideCountDataset` against its host path, `ExpressionNet` over a tiny DenseNet, and
`train_expression` over both with a criterion composed of torch operators on dense device targets (`SparseMSELoss` has no
device form: tests/test_gpu_sparse_line_max.py checks that it says so)."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from slide_fixture import SLIDE, SR1, SR2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_made = {}


def _slide_counts():
    """Host counts over the in-tissue spots of the two fixture position trees but every seventh: (counts, all in-tissue)."""
    if 's' not in _made:
        import gridnext_amd as ga
        from gridnext_amd import imgprocess as IP
        rng = np.random.default_rng(21)
        frames, total = [], 0
        for srd in (SR1, SR2):
            df = IP.visium_get_positions(srd)
            df = df[df['in_tissue'] == 1]
            total += len(df)
            keep = df.iloc[[k for k in range(len(df)) if k % 7 != 3]]
            name = os.path.basename(srd)
            frames.append(pd.DataFrame({'x': keep['array_col'].values, 'y': keep['array_row'].values, 'array': name,
                                        'annotation': ['c%d' % (k % 3) for k in range(len(keep))]},
                                       index=['%s_%d' % (name, k) for k in range(len(keep))]))
        obs = pd.concat(frames)
        X = sp.csr_matrix((rng.poisson(3.0, size=(len(obs), 40)) * (rng.random((len(obs), 40)) < 0.4)).astype(np.float64))
        counts = ga.SpotCounts(X, obs, ['g%02d' % g for g in range(40)])
        counts.normalize_total(1e4).log1p()
        _made['s'] = (counts, total)
    return _made['s']


def test_slide_count_dataset_on_the_device_equals_its_host_path():
    import gridnext_amd as ga
    counts, total = _slide_counts()
    kw = dict(patch_size=16, window_size=20)
    host = ga.SlideCountDataset([SLIDE, SLIDE], [SR1, SR2], counts, **kw)
    dev = ga.SlideCountDataset([SLIDE, SLIDE], [SR1, SR2], counts.to(DEV), device=DEV, **kw)
    assert len(dev) == len(host) == counts.n_spots and dev.dropped == host.dropped == total - counts.n_spots > 0
    assert np.array_equal(dev.rows, host.rows) and np.array_equal(dev.annotations, host.annotations)
    assert sorted(dev.rows.tolist()) == list(range(counts.n_spots))
    picks = [len(dev) - 1, 0, 5, 1, len(dev) - 2, 0]                                 # both slides, interleaved, a repeat
    calls, real = [], dev._src.gather

    def counting(i, *a, **k):
        calls.append(i)
        return real(i, *a, **k)
    dev._src.gather = counting
    got = dev.__getitems__(picks)
    dev._src.gather = real
    assert sorted(calls) == [0, 1]                                                   # one gather per slide of the batch
    for (p, r, l), (p0, r0, l0) in zip(got, host.__getitems__(picks)):
        assert p.is_cuda and p.dtype == torch.uint8 and torch.equal(p.cpu(), p0) and int(r) == int(r0) and int(l) == int(l0)
    xb, rb, yb = next(iter(DataLoader(dev, batch_size=6)))
    assert xb.is_cuda and xb.shape == (6, 3, 16, 16) and not rb.is_cuda and rb.tolist() == dev.rows[:6].tolist()
    assert dev.resident() == [0, 1]
    with pytest.raises(ValueError, match=r"device=None \(the host\), but the counts are on cuda:0"):
        ga.SlideCountDataset([SLIDE, SLIDE], [SR1, SR2], counts.to(DEV), **kw)


TINY = dict(growth_rate=6, block_config=(2, 3, 2), num_init_features=10, bn_size=2, small_inputs=True, classify=False, compression=0.5)


def _dense_targets():
    """float32 (storage rows, 40) on the device: the counts' rows times 1 / gene_max (the device maximum)."""
    import gridnext_amd as ga
    counts, _ = _slide_counts()
    ptr, idx, val = (t.numpy() for t in counts._s.csr)
    scale = ga.SparseMSELoss.unit_scale(counts.to(DEV))
    return (torch.from_numpy(sp.csr_matrix((val, idx, ptr), shape=(len(ptr) - 1, 40)).toarray()) * scale).to(DEV)


def _expression_run(outfile=None, epochs=3):
    import gridnext_amd as ga
    counts, _ = _slide_counts()
    dev = counts.to(DEV)
    kw = dict(patch_size=16, window_size=20, device=DEV, raw_uint8=False)
    sets = {'train': ga.SlideCountDataset([SLIDE], [SR1], dev.subset_arrays(['wsi_sr1']), **kw),
            'val': ga.SlideCountDataset([SLIDE], [SR2], dev.subset_arrays(['wsi_sr2']), **kw)}
    loaders = {'train': DataLoader(sets['train'], batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(4)),
               'val': DataLoader(sets['val'], batch_size=8)}
    torch.manual_seed(7)
    model = ga.ExpressionNet(ga.DenseNet(**TINY), counts.n_genes)
    dense = _dense_targets()

    def criterion(z, rows):                                                           # the notebook's Sigmoid + MSELoss, composed
        return F.mse_loss(torch.sigmoid(z), dense[rows.to(DEV)])
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    with contextlib.redirect_stdout(io.StringIO()) as text:
        model, vh, th = ga.train_expression(model, loaders, criterion, opt, num_epochs=epochs, outfile=outfile)
    return model, vh, th, sets, text.getvalue()


def test_train_expression_over_a_tiny_densenet(tmp_path):
    """Three epochs on 16-px patches cut from the resident fixture slide: a second run gives the same bits; the weights returned
    are the ones saved at the best validation epoch; the printed lines are the loop's."""
    out = str(tmp_path / 'expr.pt')
    model, vh, th, sets, text = _expression_run(out)
    model2, vh2, th2, _, _ = _expression_run()
    print("train_expression, 3 epochs: train", th, "val", vh)
    assert len(vh) == len(th) == 3 and np.isfinite(vh + th).all() and vh == vh2 and th == th2
    sd, sd2 = model.state_dict(), model2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)                               # a second run: the same bits
    saved = torch.load(out)
    assert list(saved) == list(sd) and all(torch.equal(saved[k].to(DEV), sd[k]) for k in sd)    # the best weights: restored, saved
    assert 'train Loss: %.4f' % th[0] in text and 'val Loss: %.4f' % vh[-1] in text and 'Best val loss: %4f' % min(vh) in text
    assert next(model.parameters()).is_cuda
    # an epoch's loss is the mean of its batch losses: the validation pass again, by hand, on the restored weights
    model.eval()
    dense = _dense_targets()
    with torch.no_grad():
        losses = [float(F.mse_loss(torch.sigmoid(model(x)), dense[r.to(DEV)])) for x, r, _ in DataLoader(sets['val'], batch_size=8)]
    assert abs(sum(losses) / len(losses) - min(vh)) <= 1e-6 * min(vh)


def test_expression_net_head_is_the_linear_layer_of_its_features():
    """z = features W^T + b through the HIP GEMM: within (F + 1) 2^-24 (|h| |W|^T + |b|) of the float64 product, per element."""
    import gridnext_amd as ga
    torch.manual_seed(3)
    net = ga.ExpressionNet(ga.DenseNet(**TINY), 23).to(DEV).eval()
    x = torch.rand(5, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        h, z = net.backbone(x), net(x)
    assert z.shape == (5, 23) and h.shape == (5, net.head.in_features) and net.head.in_features == net.backbone.num_features
    h64, W, b = h.double().cpu(), net.head.weight.detach().double().cpu(), net.head.bias.detach().double().cpu()
    bound = (h.shape[1] + 1) * 2.0 ** -24 * (h64.abs() @ W.abs().t() + b.abs())
    assert bool(((z.double().cpu() - (h64 @ W.t() + b)).abs() <= bound).all())
    z2 = net(x)
    z2.square().mean().backward()
    assert bool(((z2.detach().double().cpu() - (h64 @ W.t() + b)).abs() <= 2 * bound).all())       # the taped forward: other kernels
    assert net.head.weight.grad is not None and torch.isfinite(net.head.weight.grad).all()
    assert next(net.backbone.parameters()).grad is not None
