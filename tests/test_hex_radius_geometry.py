"""CPU: the geometry and module contract of radius-k hexagonal convolutions (hexagdly.Conv2d(kernel_size=k)).

 * the tap table of tests/hex_radius_ref.py (the one include/gridnext_hip.h states for gnx_hexconv_k_*) is the set of cells
   within k steps of the size-1 stencil of oracle/hexconv.py, for both parities;
 * its gather form and hexagdly's sub-convolution decomposition agree in float64 on odd, even and degenerate grids, and at
   k = 1 both equal the size-1 oracle's forms;
 * gridnext_amd.hexconv.Conv2d builds hexagdly's parameters for every kernel_size (names, shapes, order, init, state_dict).
"""
import pytest
import torch

import hex_radius_ref as R
from oracle import hexconv as ohex

torch.set_num_threads(1)


def _closure(k, parity):
    """Offsets (dp, dq) of the cells reached from a cell of the given parity in at most k steps of the size-1 stencil."""
    cells = {(parity, 0)}                               # (column, row), absolute: each step looks up its own column's parity
    for _ in range(k):
        cells = cells | {(c + dc, r + dr) for c, r in cells for dr, dc, _t, _a, _b in ohex.hex_taps(c % 2)}
    return {(c - parity, r) for c, r in cells}


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("parity", [0, 1])
def test_tap_table_is_the_k_step_closure_of_the_size1_stencil(k, parity):
    table = R.tap_table(k, parity)
    offsets = [(dp, dq) for dp, dq, _j, _a, _b in table]
    assert len(table) == R.n_taps(k) == len(set(offsets))
    assert set(offsets) == _closure(k, parity)
    # parameter order: kernel0's column, then kernel1 .. kernel{k}, (a, b) row-major inside each
    assert [(j, a, b) for _dp, _dq, j, a, b in table] == \
        [(0, a, 0) for a in range(2 * k + 1)] + [(j, a, b) for j in range(1, k + 1) for a in range(2 * k + 1 - j) for b in (0, 1)]


def _layer(O, I, k, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=torch.float64) for s in R.kernel_shapes(O, I, k)], \
        torch.randn(O, generator=g, dtype=torch.float64)


GRIDS = [(78, 64), (7, 5), (1, 1), (2, 3), (4, 1), (1, 6), (6, 7), (3, 2)]


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("R_,C", GRIDS)
def test_gather_and_subconvolution_forms_agree(k, R_, C):
    ks, b = _layer(3, 2, k, 100 * k + R_ + C)
    x = torch.randn(2, 2, R_, C, generator=torch.Generator().manual_seed(R_ * C + k), dtype=torch.float64)
    ga, sc = R.gather_k(x, ks, b), R.subconv_k(x, ks, b)
    assert (ga - sc).abs().max().item() <= 1e-10 * max(1.0, ga.abs().max().item())
    go, so = R.oddr(R.gather_k, x, ks, b), R.oddr(R.subconv_k, x, ks, b)
    assert (go - so).abs().max().item() <= 1e-10 * max(1.0, go.abs().max().item())
    if k == 1:
        assert torch.equal(ga, ohex.hexconv_gather(x, ks[0], ks[1], b))
        assert (sc - ohex.hexconv_subconv(x, ks[0], ks[1], b)).abs().max().item() <= 1e-12 * max(1.0, sc.abs().max().item())
        assert torch.equal(go, ohex.hexconv_oddr(x, ks[0], ks[1], b))


def test_a_single_tap_moves_a_point_to_its_table_offset():
    """One nonzero weight per tap: the output is the input shifted by exactly that tap's offset (both parities, away from the
    border), so the table, not just the tap set, is what the layer applies."""
    k = 3
    for parity in (0, 1):
        for t, (dp, dq, j, a, b) in enumerate(R.tap_table(k, parity)):
            ks = [torch.zeros(s, dtype=torch.float64) for s in R.kernel_shapes(1, 1, k)]
            ks[j][0, 0, a, b] = 1.0
            x = torch.zeros(1, 1, 16, 16, dtype=torch.float64)
            r0, c0 = 8 + dq, 8 + parity + dp               # the cell the output cell (8, 8 + parity) reads
            x[0, 0, r0, c0] = 1.0
            for form in (R.gather_k, R.subconv_k):
                y = form(x, ks)
                # (cells of the other parity read that point through other offsets of the same weight)
                assert y[0, 0, 8, 8 + parity].item() == 1.0 and y[..., parity::2].sum().item() == 1.0, (t, form.__name__)


# ------------------------------------------------------------------------------------------------ module contract
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_module_parameters_follow_hexagdly(k):
    import gridnext_amd.hexconv as hexagdly
    m = hexagdly.Conv2d(5, 7, kernel_size=k, stride=1, bias=True)
    names = [n for n, _ in m.named_parameters()]
    assert names == ['kernel%d' % j for j in range(k + 1)] + ['bias_tensor']
    assert [tuple(p.shape) for _, p in m.named_parameters()] == [tuple(s) for s in R.kernel_shapes(7, 5, k)] + [(7,)]
    assert sum(p[0, 0].numel() for p in m.kernels()) == R.n_taps(k)
    assert m.kernel_size == k and 'kernel_size=%d' % k in repr(m)
    assert torch.all(m.bias_tensor == 0.01)
    for p in m.kernels():                                   # xavier_uniform_ bound per kernel tensor
        fan_in, fan_out = p.shape[1] * p.shape[2] * p.shape[3], p.shape[0] * p.shape[2] * p.shape[3]
        assert p.abs().max().item() <= (6.0 / (fan_in + fan_out)) ** 0.5
    assert list(hexagdly.Conv2d(5, 7, kernel_size=k, bias=False).state_dict()) == ['kernel%d' % j for j in range(k + 1)]
    # state_dict round trip into a fresh layer
    n = hexagdly.Conv2d(5, 7, kernel_size=k)
    n.load_state_dict(m.state_dict())
    for (a, p), (b, q) in zip(m.named_parameters(), n.named_parameters()):
        assert a == b and torch.equal(p, q)
    d = hexagdly.Conv2d(5, 7, kernel_size=k, debug=True)
    assert all(torch.all(p == 1.0) for p in d.parameters())


def test_module_rejects_what_it_does_not_implement():
    import gridnext_amd.hexconv as hexagdly
    with pytest.raises(NotImplementedError):
        hexagdly.Conv2d(4, 4, kernel_size=2, stride=2)
    with pytest.raises(NotImplementedError):
        hexagdly.Conv2d(4, 4, kernel_size=1, stride=2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            hexagdly.Conv2d(4, 4, kernel_size=bad)


def test_size1_layer_parameters_are_unchanged():
    """kernel_size=1 draws the same parameters as before (and as the oracle's module from the same seed)."""
    import gridnext_amd.hexconv as hexagdly
    torch.manual_seed(11)
    m = hexagdly.Conv2d(6, 9, kernel_size=1)
    torch.manual_seed(11)
    o = ohex.HexConv2d(6, 9)
    assert [n for n, _ in m.named_parameters()] == ['kernel0', 'kernel1', 'bias_tensor']
    for n in ('kernel0', 'kernel1', 'bias_tensor'):
        assert torch.equal(getattr(m, n).detach(), getattr(o, n).detach()), n
