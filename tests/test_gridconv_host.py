"""Host logic of the Cartesian corrector's HIP route (no GPU needed): which nn.Conv2d configurations `GF.gridconv` takes,
GridNet's unchanged state dict, and GridNet on CPU tensors - forward, forward_nhwc, all_fgd_predictions - still being the
stock torch layers, bit for bit."""
import copy

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from conftest import load_golden


def _model(use_bn=True, seed=0, G=24, C=5, hw=(7, 6)):
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    torch.manual_seed(seed)
    return ga.GridNet(count_mlp(G, C), (G,), hw, C, use_bn=use_bn)


def test_eligibility_rule_on_module_configurations():
    from gridnext_amd import functional as GF
    ok = [nn.Conv2d(4, 8, 3, padding=1), nn.Conv2d(4, 8, 5, padding=2), nn.Conv2d(4, 8, 7, padding=3),
          nn.Conv2d(4, 8, (3, 5), padding=(1, 2)), nn.Conv2d(4, 8, (1, 7), padding=(0, 3)), nn.Conv2d(4, 8, 1),
          nn.Conv2d(4, 8, 3, padding='same'), nn.Conv2d(4, 8, 3, padding=1, bias=False),
          nn.Conv2d(4, 8, (1, 217), padding=(0, 108)), nn.Conv2d(4, 8, 13, padding=6)]
    no = [nn.Conv2d(4, 8, 3, padding=1, stride=2), nn.Conv2d(4, 8, 3, padding=2, dilation=2),
          nn.Conv2d(4, 8, 3, padding=1, groups=2), nn.Conv2d(4, 8, 3, padding=1, padding_mode='reflect'),
          nn.Conv2d(4, 8, 2, padding='same'), nn.Conv2d(4, 8, (3, 4), padding=(1, 2)), nn.Conv2d(4, 8, 3),
          nn.Conv2d(4, 8, 3, padding=2), nn.Conv2d(4, 8, 3, padding='valid'), nn.Conv2d(4, 8, (3, 5), padding=(2, 1)),
          nn.Conv2d(4, 8, 15, padding=7), nn.Conv2d(4, 8, (1, 219), padding=(0, 109)),
          nn.ConvTranspose2d(4, 8, 3, padding=1), nn.Conv1d(4, 8, 3, padding=1), nn.Linear(4, 8), nn.ReLU()]
    for m in ok:
        assert GF.gridconv_layer(m), m
    for m in no:
        assert not GF.gridconv_layer(m), m
    # the tensor side: nothing on the CPU, nothing that is not fp32, is sent to the HIP kernels
    assert GF.GRIDCONV_MAX_TAPS == 217
    x = torch.zeros(1, 4, 4, 4)
    assert not GF.gridconv_eligible(ok[0], x)
    assert not GF.gridconv_eligible(copy.deepcopy(ok[0]).double(), x.double())


def test_state_dict_keys_and_initialisation_unchanged():
    g = load_golden('gridwise_cartesian')
    m = _model(seed=3)
    assert list(m.state_dict()) == [k[5:] for k in g if k.startswith('init/')]
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(g['init/' + k].shape), k
    assert [type(x) for x in m.corrector] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU] * 3 + [nn.Conv2d]
    assert [type(x) for x in _model(use_bn=False).corrector] == [nn.Conv2d, nn.ReLU] * 3 + [nn.Conv2d]
    assert [tuple(c.kernel_size) for c in m.corrector if isinstance(c, nn.Conv2d)] == [(3, 3), (5, 5), (5, 5), (3, 3)]
    # default initialisation and RNG consumption: the corrector is what the same seed gives the stock layers in that order
    from gridnext_amd.synthetic import count_mlp
    torch.manual_seed(3)
    count_mlp(24, 5)
    ref = nn.Sequential(nn.Conv2d(5, 5, 3, padding=1), nn.BatchNorm2d(5), nn.ReLU(), nn.Conv2d(5, 5, 5, padding=2),
                        nn.BatchNorm2d(5), nn.ReLU(), nn.Conv2d(5, 5, 5, padding=2), nn.BatchNorm2d(5), nn.ReLU(),
                        nn.Conv2d(5, 5, 3, padding=1))
    for (n, a), (_, b) in zip(m.corrector.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), n
    # every default layer is one the HIP route takes
    from gridnext_amd import functional as GF
    assert all(GF.gridconv_layer(c) for c in m.corrector if isinstance(c, nn.Conv2d))


def test_cpu_forward_is_the_stock_layers_bit_for_bit():
    for use_bn in (True, False):
        for train in (False, True):
            m = _model(use_bn=use_bn, seed=5)
            m.train(train)
            m.patch_classifier.eval()
            stock = copy.deepcopy(m)
            x = torch.rand(2, 7, 6, 24)
            with torch.no_grad():
                want = stock.corrector(stock.patch_predictions(x))
                got = m(x)
            assert got.shape == (2, 5, 7, 6)
            assert torch.equal(got, want)
            m2 = copy.deepcopy(stock)
            stock2 = copy.deepcopy(stock)
            with torch.no_grad():
                got2 = m2.forward_nhwc(x)
                want2 = stock2.corrector(stock2.patch_predictions(x))
            assert got2.shape == (2, 7, 6, 5)
            assert torch.equal(got2.permute(0, 3, 1, 2), want2)
            for (n, a), (_, b) in zip(m.state_dict().items(), stock.state_dict().items()):
                assert torch.equal(a, b), n                       # running statistics moved as the stock layers move them


def test_cpu_backward_is_the_stock_layers_bit_for_bit():
    m = _model(seed=6)
    m.train()
    stock = copy.deepcopy(m)
    x = torch.rand(2, 7, 6, 24)
    m(x).square().sum().backward()
    stock.corrector(stock.patch_predictions(x)).square().sum().backward()
    for (n, a), (_, b) in zip(m.named_parameters(), stock.named_parameters()):
        assert torch.equal(a.grad, b.grad), n


def test_all_fgd_predictions_runs_on_a_gridnet():
    """On a machine without a HIP device the model stays on the CPU and `all_fgd_predictions` picks up `forward_nhwc`, which
    there is the stock layers: the reference's softmax / argmax, exactly.  (With a device the helper moves the model there;
    tests/test_gpu_gridconv.py checks that route.)"""
    from gridnext_amd.utils import all_fgd_predictions
    m = _model(seed=7)
    g = torch.Generator().manual_seed(1)
    x, y = torch.rand(4, 7, 6, 24, generator=g), torch.randint(0, 6, (4, 7, 6), generator=g)
    stock = copy.deepcopy(m).eval()
    true, pred, smax = all_fgd_predictions(DataLoader(TensorDataset(x, y), batch_size=2), m)
    with torch.no_grad():
        rows = torch.cat([stock(x[i:i + 2]).permute(0, 2, 3, 1).reshape(-1, 5) for i in (0, 2)])   # the loader's batches
    keep = y.reshape(-1) > 0
    assert true.shape == pred.shape == (int(keep.sum()),) and smax.shape == (int(keep.sum()), 5)
    np.testing.assert_array_equal(true, (y.reshape(-1)[keep] - 1).numpy())
    if not torch.cuda.is_available():
        np.testing.assert_array_equal(smax, torch.softmax(rows, 1)[keep].numpy())
        np.testing.assert_array_equal(pred, torch.argmax(rows, 1)[keep].numpy())
    else:
        np.testing.assert_allclose(smax, torch.softmax(rows, 1)[keep].numpy(), atol=1e-4)        # (two fp32 routes)
