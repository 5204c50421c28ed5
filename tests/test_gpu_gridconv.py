"""GPU: the Cartesian corrector on HIP (nn.Conv2d of stride 1, zero "same" padding, odd sizes; gnx_gridconv_*).

 * kernels through the C ABI: y, dx, dweight and dbias against float64 torch.nn.functional.conv2d + autograd at each
   contraction's rounding bound (y: kh kw I terms, dx: kh kw O, weight and bias: B H W): the default corrector's layers on
   a whole 78 x 64 array and on 35 x 33 (the classic ST array) with B = 2, scalar widths (5, 7), matrix-core widths, chunked
   widths (33, 70, 130), 7x7 and rectangular sizes, grids smaller than the kernel, no bias; repeatability, `accumulate`,
   NULL destinations, argument checks; batch and row isolation;
 * the autograd node, frozen weight and frozen bias included;
 * one whole-array step of GridNet against the float64 oracle; the same step with torch's convolution patched to raise;
 * the reference fixture through forward_nhwc; train_gridwise captured and replayed against the float64 oracle and against
   the eager loop bit for bit; the torch fallback of layers the kernels do not take; all_fgd_predictions.
"""
import contextlib
import copy
import io
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset

from conftest import load_golden, sub

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TMAX = 217


@pytest.fixture(scope='module')
def L():
    from gridnext_amd import _lib
    return _lib


def _rounding_gate(got, ref, length, what, c=32.0):
    """max |got - ref| <= c * sqrt(length) * 2^-24 * max |ref|: the rounding bound of an fp32 contraction of `length` terms
    against a float64 reference (the rule of tests/test_gpu_hex_radius.py:_rounding_gate).  Returns error / gate."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    gate = c * length ** 0.5 * 2.0 ** -24 * (ref.abs().max().item() if ref.numel() else 0.0)
    assert err <= gate, "%s: max abs err %.3e > gate %.3e (%.1f x the gate)" % (what, err, gate, err / max(gate, 1e-300))
    return err / gate if gate > 0 else 0.0


def _reference(x, w, b, dy):
    """float64 (y, dx, dweight, dbias) in the GPU's channels-last layout; x / dy: [B, H, W, C]; b may be None."""
    kh, kw = w.shape[2:]
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.double().clone().requires_grad_(True)
    br = None if b is None else b.double().clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br, padding=(kh // 2, kw // 2))
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad, None if br is None else br.grad


def _case(B, H, W, I, O, kh, kw, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, I, generator=g)
    w = torch.randn(O, I, kh, kw, generator=g) * (kh * kw * I) ** -0.5
    b = torch.randn(O, generator=g) if bias else None
    dy = torch.randn(B, H, W, O, generator=g)
    return x, w, b, dy


def _run(L, x, w, b, dy, dw='new', db='new', accumulate=0):
    B, H, W, I = x.shape
    O, _, kh, kw = w.shape
    y, dx = torch.empty(B, H, W, O, device=DEV), torch.empty(B, H, W, I, device=DEV)
    L.call('gnx_gridconv_fwd', L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), B, H, W, I, O, kh, kw, L.stream())
    L.call('gnx_gridconv_bwd_data', L.ptr(dy), L.ptr(w), L.ptr(dx), B, H, W, I, O, kh, kw, L.stream())
    if isinstance(dw, str):
        dw = torch.empty_like(w)
    if isinstance(db, str):
        db = torch.empty(O, device=DEV)
    ws = torch.empty(max(1, L.query('gnx_gridconv_bwd_weight_workspace', B, H, W, I, O, kh, kw)), device=DEV)
    L.call('gnx_gridconv_bwd_weight', L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), L.ptr(ws), B, H, W, I, O, kh, kw, accumulate,
           L.stream())
    torch.cuda.synchronize()
    return y, dx, dw, db


ARRAYS = [(1, 78, 64), (2, 35, 33)]       # one whole Visium-sized array; the classic ST array size (domain knowledge), B = 2
# (B, H, W, I, O, kh, kw, bias)
CASES = [a + l + (True,) for a in ARRAYS for l in ((16, 8, 3, 3), (8, 8, 5, 5), (8, 8, 3, 3))] + \
        [(2, 35, 33, c, c, k, k, True) for c in (5, 7) for k in (3, 5)] + [(1, 78, 64, 5, 5, 5, 5, True)] + \
        [(1, 78, 64, 32, 32, 5, 5, True), (2, 35, 33, 32, 32, 5, 5, True), (1, 78, 64, 64, 8, 3, 3, True),
         (2, 35, 33, 64, 8, 3, 3, True)] + \
        [(1, 9, 7, 33, 70, 3, 3, True), (1, 9, 7, 130, 33, 3, 3, True), (1, 6, 5, 70, 130, 5, 5, True)] + \
        [(2, 35, 33, 8, 8, 7, 7, True), (1, 12, 9, 5, 7, 7, 7, True), (2, 13, 10, 8, 16, 3, 5, True),
         (1, 13, 10, 7, 5, 3, 5, True), (2, 13, 10, 16, 8, 1, 7, True), (1, 13, 10, 3, 4, 1, 7, True),
         (1, 13, 10, 8, 8, 1, 1, True)] + \
        [(1, 1, 1, 8, 8, 5, 5, True), (1, 1, 1, 5, 5, 5, 5, True), (1, 2, 3, 8, 8, 5, 5, True), (2, 2, 3, 7, 7, 5, 5, True),
         (1, 1, 1, 16, 8, 3, 3, True)] + \
        [(2, 35, 33, 8, 8, 5, 5, False), (1, 11, 9, 5, 5, 3, 3, False), (1, 1, 1, 8, 8, 5, 5, False)]


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d %d->%d %dx%d%s" % (c[:7] + ('' if c[7] else ' nobias',)) for c in CASES])
def test_gridconv_kernels_against_fp64(L, case):
    B, H, W, I, O, kh, kw, bias = case
    x, w, b, dy = _case(B, H, W, I, O, kh, kw, seed=CASES.index(case) + 11, bias=bias)
    yr, dxr, dwr, dbr = _reference(x, w, b, dy)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), dy.to(DEV)
    y, dx, dw, db = _run(L, xd, wd, bd, dyd)
    _rounding_gate(y, yr, kh * kw * I, 'y')
    _rounding_gate(dx, dxr, kh * kw * O, 'dx')
    _rounding_gate(dw, dwr, B * H * W, 'dweight')
    dbr = dbr if dbr is not None else dy.double().sum((0, 1, 2))        # (the bias gradient does not depend on a bias)
    _rounding_gate(db, dbr, B * H * W, 'dbias')
    # two calls: the same bits
    y2, dx2, dw2, db2 = _run(L, xd, wd, bd, dyd)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    # accumulate = 1 adds onto the destination
    acc_w, acc_b = torch.full_like(wd, 0.5), torch.full((O,), 0.25, device=DEV)
    _run(L, xd, wd, bd, dyd, dw=acc_w, db=acc_b, accumulate=1)
    assert torch.equal(acc_w, torch.full_like(wd, 0.5) + dw), 'accumulate: dweight'
    assert torch.equal(acc_b, torch.full((O,), 0.25, device=DEV) + db), 'accumulate: dbias'
    # NULL destinations are skipped, the other one is written
    _, _, only_w, none_b = _run(L, xd, wd, bd, dyd, db=None)
    assert none_b is None and torch.equal(only_w, dw)
    _, _, none_w, only_b = _run(L, xd, wd, bd, dyd, dw=None)
    assert none_w is None and torch.equal(only_b, db)
    ws = torch.full((max(1, L.query('gnx_gridconv_bwd_weight_workspace', B, H, W, I, O, kh, kw)),), 7.0, device=DEV)
    L.call('gnx_gridconv_bwd_weight', L.ptr(xd), L.ptr(dyd), None, None, L.ptr(ws), B, H, W, I, O, kh, kw, 0, L.stream())
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all()), 'both destinations NULL: nothing is launched'


def test_gridconv_argument_checks(L):
    x = torch.randn(1, 4, 4, 8, device=DEV)
    y = torch.empty(1, 4, 4, 8, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    st = L.stream()
    for (kh, kw), rc in (((2, 3), -1), ((3, 4), -1), ((0, 3), -1), ((15, 15), L.ERR_UNSUPPORTED), ((1, TMAX + 2), L.ERR_UNSUPPORTED)):
        w = torch.zeros(8, 8, max(kh, 1), kw, device=DEV)
        sentinel = torch.full_like(y, 3.0)
        assert L.query('gnx_gridconv_fwd', L.ptr(x), L.ptr(w), None, L.ptr(sentinel), 1, 4, 4, 8, 8, kh, kw, st) == rc
        assert L.query('gnx_gridconv_bwd_data', L.ptr(x), L.ptr(w), L.ptr(sentinel), 1, 4, 4, 8, 8, kh, kw, st) == rc
        assert L.query('gnx_gridconv_bwd_weight', L.ptr(x), L.ptr(x), L.ptr(w), None, L.ptr(ws), 1, 4, 4, 8, 8, kh, kw, 0, st) == rc
        assert L.query('gnx_gridconv_bwd_weight_workspace', 1, 4, 4, 8, 8, kh, kw) == 0
        torch.cuda.synchronize()
        assert bool((sentinel == 3.0).all()), 'nothing is launched'
    w = torch.zeros(8, 8, 3, 3, device=DEV)
    assert L.query('gnx_gridconv_fwd', L.ptr(x), None, None, L.ptr(y), 1, 4, 4, 8, 8, 3, 3, st) == -1
    assert L.query('gnx_gridconv_bwd_data', L.ptr(x), None, L.ptr(y), 1, 4, 4, 8, 8, 3, 3, st) == -1
    assert L.query('gnx_gridconv_fwd', None, L.ptr(w), None, L.ptr(y), 1, 4, 4, 8, 8, 3, 3, st) == -1
    assert L.query('gnx_gridconv_bwd_weight', L.ptr(x), L.ptr(x), L.ptr(w), None, None, 1, 4, 4, 8, 8, 3, 3, 0, st) == -1
    # the widest table that is taken: 1 x 217
    xw = torch.randn(1, 2, 230, 8, device=DEV)
    ww = torch.randn(8, 8, 1, TMAX, device=DEV) * (TMAX * 8) ** -0.5
    yw = torch.empty(1, 2, 230, 8, device=DEV)
    L.call('gnx_gridconv_fwd', L.ptr(xw), L.ptr(ww), None, L.ptr(yw), 1, 2, 230, 8, 8, 1, TMAX, st)
    ref = F.conv2d(xw.double().cpu().permute(0, 3, 1, 2), ww.double().cpu(), None, padding=(0, TMAX // 2)).permute(0, 2, 3, 1)
    _rounding_gate(yw, ref, TMAX * 8, 'y 1x217')


@pytest.mark.parametrize("I,O,kh,kw", [(8, 8, 5, 5), (5, 5, 5, 5), (7, 3, 3, 7), (32, 32, 3, 3)])
def test_batch_and_row_isolation(L, I, O, kh, kw):
    """Positions are flat: no tap may reach into the next array of the batch or round a row's end."""
    B, H, W = 3, 6, 7
    g = torch.Generator().manual_seed(I + O + kh)
    w = torch.randn(O, I, kh, kw, generator=g).to(DEV)
    b = torch.randn(O, generator=g).to(DEV)
    x = torch.zeros(B, H, W, I)
    x[1] = torch.randn(H, W, I, generator=g)
    y, _, _, _ = _run(L, x.to(DEV), w, b, torch.zeros(B, H, W, O, device=DEV))
    for other in (0, 2):
        assert torch.equal(y[other], b.expand(H, W, O)), 'array %d of the batch saw its neighbour' % other
    # the data gradient of a gradient that lives in one array stays in that array
    dy = torch.zeros(B, H, W, O)
    dy[1] = torch.randn(H, W, O, generator=g)
    _, dx, _, _ = _run(L, x.to(DEV), w, b, dy.to(DEV))
    assert not dx[0].any() and not dx[2].any()
    # a one-hot input at a row's end (and one at a row's start): only its own kh x kw window moves, the next row's start does not
    for (r, c) in ((2, W - 1), (3, 0), (H - 1, W - 1), (0, 0)):
        x = torch.zeros(B, H, W, I)
        x[1, r, c, I - 1] = 1.0
        y, _, _, _ = _run(L, x.to(DEV), w, b, torch.zeros(B, H, W, O, device=DEV))
        moved = (y != b).any(-1).cpu()
        window = torch.zeros(B, H, W, dtype=torch.bool)
        window[1, max(0, r - kh // 2):r + kh // 2 + 1, max(0, c - kw // 2):c + kw // 2 + 1] = True
        assert not (moved & ~window).any(), 'one-hot at (%d, %d) reached %s' % (r, c, (moved & ~window).nonzero().tolist())
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().cpu(), b.double().cpu(), padding=(kh // 2, kw // 2))
        _rounding_gate(y, ref.permute(0, 2, 3, 1), kh * kw * I, 'one-hot y')
        dy = torch.zeros(B, H, W, O)
        dy[1, r, c, O - 1] = 1.0
        _, dx, _, _ = _run(L, x.to(DEV), w, b, dy.to(DEV))
        assert not (dx.cpu().ne(0).any(-1) & ~window).any(), 'one-hot gradient at (%d, %d) left its window' % (r, c)


# ------------------------------------------------------------------------------------------------ autograd node
@pytest.mark.parametrize("frozen", ['none', 'weight', 'bias', 'input', 'nobias'])
def test_gridconv_autograd_against_fp64_twin(frozen):
    from gridnext_amd import functional as GF
    B, H, W, I, O, kh, kw = 2, 13, 10, 16, 24, 5, 3
    x, w, b, dy = _case(B, H, W, I, O, kh, kw, seed=77, bias=frozen != 'nobias')
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(frozen != 'input')
    wr = w.double().clone().requires_grad_(frozen != 'weight')
    br = None if b is None else b.double().clone().requires_grad_(frozen != 'bias')
    ref = F.conv2d(xr, wr, br, padding=(kh // 2, kw // 2))
    ref.backward(dy.double().permute(0, 3, 1, 2))
    xd = x.to(DEV).requires_grad_(frozen != 'input')
    wd = w.to(DEV).requires_grad_(frozen != 'weight')
    bd = None if b is None else b.to(DEV).requires_grad_(frozen != 'bias')
    y = GF.gridconv(xd, wd, bd)
    y.backward(dy.to(DEV))
    _rounding_gate(y, ref.permute(0, 2, 3, 1), kh * kw * I, 'y')
    for name, got, want, length in (('input', xd, xr, kh * kw * O), ('weight', wd, wr, B * H * W), ('bias', bd, br, B * H * W)):
        if got is None:
            continue
        if frozen == name:
            assert got.grad is None, 'a frozen %s got a gradient' % name
        else:
            _rounding_gate(got.grad, want.grad.permute(0, 2, 3, 1) if name == 'input' else want.grad, length, 'd' + name)


def test_frozen_parameters_launch_nothing_for_them(monkeypatch):
    """needs_input_grad is honoured: with weight and bias frozen the weight-gradient entry point is not called at all, with only
    the bias frozen it gets a NULL dbias."""
    from gridnext_amd import _lib, functional as GF
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', spy)
    x, w, b, dy = _case(1, 6, 5, 8, 8, 3, 3, seed=5)
    xd, wd, bd = x.to(DEV).requires_grad_(True), w.to(DEV), b.to(DEV)
    GF.gridconv(xd, wd, bd).backward(dy.to(DEV))
    assert [n for n, _ in calls] == ['gnx_gridconv_fwd', 'gnx_gridconv_bwd_data']
    del calls[:]
    wd.requires_grad_(True)
    GF.gridconv(x.to(DEV), wd, bd).backward(dy.to(DEV))
    assert [n for n, _ in calls] == ['gnx_gridconv_fwd', 'gnx_gridconv_bwd_weight']
    assert calls[1][1][3] is None and wd.grad is not None and bd.grad is None


# ------------------------------------------------------------------------------------------------ model level
FULL_G = 2000


@contextlib.contextmanager
def _oracle_threads():
    keep = torch.get_num_threads()
    torch.set_num_threads(int(os.environ.get('OMP_NUM_THREADS', '8')))
    try:
        yield
    finally:
        torch.set_num_threads(keep)


def _oracle_twin(m, cls=None):
    """The float64 oracle twin of a (CPU-resident) HIP model: same weights, same frozen parameters."""
    from oracle import gridnet as ogn
    om = (cls or ogn.GridNet)(copy.deepcopy(m.patch_classifier), m.patch_shape, m.grid_shape, m.n_classes, use_bn=m.use_bn)
    om.corrector.load_state_dict(m.corrector.state_dict())
    for p, q in zip(m.corrector.parameters(), om.corrector.parameters()):
        q.requires_grad_(p.requires_grad)
    return om.double()


def _gate_grads_and_stats(m, om, ce, ce_ref, what, capsys):
    """Every corrector gradient within 1e-4 of its float64 range (the conv biases right before a train-mode BatchNorm, whose
    true gradient is 0: of their own layer's weight-gradient range), running statistics within 1e-4 of theirs, |dCE| <= 1e-4
    (the gates of tests/test_gpu_hex_radius.py:_gate_grads_and_stats)."""
    ref = dict(om.corrector.named_parameters())
    mods = list(m.corrector)
    zero_true = {'%d.bias' % i: '%d.weight' % i for i, mod in enumerate(mods[:-1])
                 if isinstance(mod, nn.Conv2d) and isinstance(mods[i + 1], nn.BatchNorm2d) and m.training}
    worst, n = (0.0, ''), 0
    for name, p in m.corrector.named_parameters():
        q = ref[name]
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is None:
            continue
        scale = ref[zero_true[name]].grad.abs().max().item() if name in zero_true else q.grad.abs().max().item()
        err = (p.grad.detach().double().cpu() - q.grad).abs().max().item()
        assert err <= 1e-4 * scale, "%s: max abs err %.3e > 1e-4 x %.3e" % (name, err, scale)
        worst = max(worst, (err / (1e-4 * scale), name))
        n += 1
    for a, b in zip(m.corrector.modules(), om.corrector.modules()):
        if isinstance(a, nn.BatchNorm2d):
            for buf in ('running_mean', 'running_var'):
                got, r = getattr(a, buf).double().cpu(), getattr(b, buf)
                assert (got - r).abs().max().item() <= 1e-4 * r.abs().max().item(), buf
    with capsys.disabled():
        print("\n[%s] CE hip %.7f fp64 %.7f; %d gradients, worst %s at %.3f x its gate" % (what, ce, ce_ref, n, worst[1], worst[0]))
    assert abs(ce - ce_ref) <= 1e-4, (ce, ce_ref)
    return n


@contextlib.contextmanager
def _hip_relu_masks():
    """Which elements each HIP ReLU (fused after a BatchNorm or alone) let through, in call order: rows [M, C]."""
    from gridnext_amd import functional as GF
    masks, bn_relu, relu_rows = [], GF.batch_norm_relu, GF.relu_rows

    def rec_bn(x2d, bn, relu):
        y = bn_relu(x2d, bn, relu)
        if relu:
            masks.append((y.detach() > 0).reshape(-1, y.shape[-1]).cpu())
        return y

    def rec_relu(x2d):
        y = relu_rows(x2d)
        masks.append((y.detach() > 0).reshape(-1, y.shape[-1]).cpu())
        return y
    GF.batch_norm_relu, GF.relu_rows = rec_bn, rec_relu
    try:
        yield masks
    finally:
        GF.batch_norm_relu, GF.relu_rows = bn_relu, relu_rows


def _align_oracle_relus(om, masks):
    """Forward hooks on the oracle's ReLUs: a pre-activation within 1e-5 of its tensor's range of 0 takes the HIP path's side of
    the kink (an O(dy) difference there says nothing about either side); farther from the kink a disagreement FAILS - the rule
    of tests/test_gpu_hex_radius.py.  Returns (per ReLU [elements aligned, largest |x| / range], hooks)."""
    aligned = []

    def hook(mod, inp, out):
        x = inp[0]
        B, C, H, W = x.shape
        hip = masks[len(aligned)].reshape(B, H, W, C).permute(0, 3, 1, 2)
        off = hip != (x.detach() > 0)
        rng = x.detach().abs().max().item()
        worst = x.detach()[off].abs().max().item() / rng if off.any() else 0.0
        aligned.append([int(off.sum()), worst])
        assert worst <= 1e-5, "ReLU %d: HIP mask differs from float64 %.2e of the range from 0" % (len(aligned) - 1, worst)
        return torch.where(off, x * hip.to(x.dtype), out)
    return aligned, [mod.register_forward_hook(hook) for mod in om.corrector if isinstance(mod, nn.ReLU)]


def _arrays(seeds, C, hw):
    """x (B, H, W, genes) as GridNet takes it, labels (B, H, W)."""
    from gridnext_amd.synthetic import visium_array
    arrs = [visium_array(s, FULL_G, C, h=hw[0], w=hw[1], image=False) for s in seeds]
    return torch.stack([a[1].permute(1, 2, 0) for a in arrs]).contiguous(), torch.stack([a[2] for a in arrs])


def _gridnet_step(C, hw, B, use_bn, seed, capsys, what, hip_context=contextlib.nullcontext):
    """forward_nhwc -> fused masked CE -> backward of a GridNet (count MLP frozen in eval mode, corrector in train mode) on B
    whole arrays, gated against the float64 oracle twin.  The oracle's ReLUs take the HIP side of a kink that lies within 1e-5
    of the tensor's range (how many did is printed; one farther out fails)."""
    import gridnext_amd as ga
    from gridnext_amd import functional as GF
    from gridnext_amd.synthetic import count_mlp
    from oracle import masked_ce as oce
    with _oracle_threads():
        torch.manual_seed(seed)
        m = ga.GridNet(count_mlp(FULL_G, C), (FULL_G,), hw, C, use_bn=use_bn)
        for p in m.patch_classifier.parameters():
            p.requires_grad = False
        om = _oracle_twin(m)
        m.to(DEV)
        for mod in (m, om):
            mod.train()
            mod.patch_classifier.eval()
        x, y = _arrays(range(500 + seed, 500 + seed + B), C, hw)
        masks, correct = [], m._correct_nhwc

        def recorded(grid):                     # (the corrector's ReLUs only: f has its own)
            with _hip_relu_masks() as seen:
                out = correct(grid)
            masks.extend(seen)
            return out
        m._correct_nhwc = recorded
        with hip_context():
            logits = m.forward_nhwc(x.to(DEV))
            assert logits.shape == (B,) + tuple(hw) + (C,)
            loss, _, _ = GF.masked_cross_entropy(logits.reshape(-1, C), y.to(DEV), 1)
            loss.backward()
            torch.cuda.synchronize()
        aligned, hooks = _align_oracle_relus(om, masks)
        try:
            ref = oce.masked_ce(om(x.double()), y, 1)[0]
        finally:
            for h in hooks:
                h.remove()
        ref.backward()
        assert len(aligned) == len(masks) == 3
        n = _gate_grads_and_stats(m, om, loss.item(), ref.item(), what + '; ReLU elements aligned [count, |x| / range] %s' % aligned,
                                  capsys)
    assert n == (14 if use_bn else 8)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("C,hw,B,use_bn", [(8, (78, 64), 1, True), (8, (78, 64), 1, False), (5, (35, 33), 2, True)],
                         ids=['C8 78x64', 'C8 78x64 no BN', 'C5 35x33 B2'])
def test_gridnet_whole_array_step_against_fp64(capsys, C, hw, B, use_bn):
    _gridnet_step(C, hw, B, use_bn, seed=3 + C + use_bn, capsys=capsys,
                  what='GridNet C=%d %dx%d B=%d use_bn=%s, one step' % (C, hw[0], hw[1], B, use_bn))


@pytest.mark.timeout(180)
def test_no_torch_convolution_on_the_path(capsys):
    """The same whole-array step with torch.nn.functional.conv2d and nn.Conv2d._conv_forward patched to raise around the HIP
    forward and backward (the float64 oracle twin, which IS torch's convolution, runs after the patch is lifted): the
    corrector runs on the project's own kernels."""
    def refuse(*a, **k):
        raise AssertionError("torch's convolution was called on the HIP path")

    @contextlib.contextmanager
    def no_torch_conv():
        keep = torch.nn.functional.conv2d, nn.Conv2d._conv_forward
        torch.nn.functional.conv2d, nn.Conv2d._conv_forward = refuse, refuse
        try:
            yield
        finally:
            torch.nn.functional.conv2d, nn.Conv2d._conv_forward = keep
    with pytest.raises(AssertionError, match="torch's convolution"), no_torch_conv():       # the patch bites
        nn.Conv2d(2, 2, 3, padding=1)(torch.zeros(1, 2, 4, 4))
    _gridnet_step(8, (78, 64), 1, True, seed=21, capsys=capsys, what='GridNet, torch convolution refused, one step',
                  hip_context=no_torch_conv)


def test_reference_fixture_through_forward_nhwc():
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    g = load_golden('gridwise_cartesian')
    G, H, W, C = 24, 7, 6, 5
    m = ga.GridNet(count_mlp(G, C), (G,), (H, W), C, use_bn=True)
    m.load_state_dict(sub(g, 'init'))
    m.to(DEV).eval()
    with torch.no_grad():
        out = m.forward_nhwc(torch.from_numpy(g['x'])[:2].to(DEV))
    assert out.shape == (2, H, W, C)
    got, want = out.permute(0, 3, 1, 2).double().cpu(), torch.from_numpy(g['fwd0']).double()
    assert (got - want).abs().max().item() <= 1e-5 + 2e-4 * want.abs().max().item()


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.mark.timeout(300)
def test_gridnet_train_gridwise_replayed_against_fp64(monkeypatch, capsys):
    """train_gridwise for 2 epochs on 4 train and 2 val whole arrays (batch 1, Adam on g, the count MLP frozen): the step is
    captured after graphs.WARMUP eager ones and replayed (counted: an eager fallback fails); histories against
    oracle.loops.train_gridwise on the float64 twin (first train loss 1e-4, rtol 3e-4); the replayed loop equals the
    GNX_GRAPH=0 loop bit for bit (histories, weights, running statistics)."""
    import warnings
    import gridnext_amd as ga
    from gridnext_amd import graphs
    from gridnext_amd.synthetic import count_mlp
    from oracle import loops as oloops
    C, hw = 8, (78, 64)
    replays = {True: 0, False: 0}
    real_replay = graphs.GridStepGraph.replay

    def counting_replay(self, inputs, labels):
        replays[self.train] += 1
        return real_replay(self, inputs, labels)
    monkeypatch.setattr(graphs.GridStepGraph, 'replay', counting_replay)
    with _oracle_threads():
        xs, ys = _arrays(range(600, 606), C, hw)
        torch.manual_seed(81)
        m0 = ga.GridNet(count_mlp(FULL_G, C), (FULL_G,), hw, C, use_bn=True)
        for p in m0.patch_classifier.parameters():
            p.requires_grad = False
        om = _oracle_twin(m0)
        lr = 1e-3
        runs = {}
        for flag in ('', '0'):
            monkeypatch.setenv('GNX_GRAPH', flag) if flag else monkeypatch.delenv('GNX_GRAPH', raising=False)
            m = copy.deepcopy(m0).to(DEV)
            dl = {'train': DataLoader(TensorDataset(xs[:4].to(DEV), ys[:4].to(DEV)), batch_size=1),
                  'val': DataLoader(TensorDataset(xs[4:].to(DEV), ys[4:].to(DEV)), batch_size=1)}
            opt = torch.optim.Adam(m.corrector.parameters(), lr=lr)
            before = dict(replays)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                m, vh, th = _quiet(ga.train_gridwise, m, dl, nn.CrossEntropyLoss(), opt, num_epochs=2)
            failed = [str(w.message) for w in caught if 'capture failed' in str(w.message)]
            assert not failed, failed
            runs[flag] = (m, vh, th, {k: replays[k] - before[k] for k in replays})
        odl = {'train': DataLoader(TensorDataset(xs[:4].double(), ys[:4]), batch_size=1),
               'val': DataLoader(TensorDataset(xs[4:].double(), ys[4:]), batch_size=1)}
        o_opt = torch.optim.Adam(om.corrector.parameters(), lr=lr)
        om, ovh, oth = _quiet(oloops.train_gridwise, om, odl, nn.CrossEntropyLoss(), o_opt, num_epochs=2)
    m, vh, th, rep = runs['']
    with capsys.disabled():
        print("\n[GridNet, train_gridwise] train %s vs fp64 %s; val %s vs fp64 %s; replays %s"
              % (np.round(th, 7), np.round(oth, 7), np.round(vh, 7), np.round(ovh, 7), rep))
    assert rep == {True: 2 * 4 - graphs.WARMUP, False: 2 * 2 - graphs.WARMUP}, rep
    assert runs['0'][3] == {True: 0, False: 0}
    assert abs(th[0] - oth[0]) <= 1e-4
    np.testing.assert_allclose(th, oth, rtol=3e-4)
    np.testing.assert_allclose(vh, ovh, rtol=3e-4)
    me, vhe, the, _ = runs['0']
    assert list(th) == list(the) and list(vh) == list(vhe)
    for (n, a), (_, b) in zip(m.state_dict().items(), me.state_dict().items()):
        assert torch.equal(a, b), "replayed and eager loops differ at %s" % n


# ------------------------------------------------------------------------------------------------ fallback and routes
def _odd_corrector(f_dim, c):
    """A user's corrector: two layers the HIP convolution takes, a dilated one, a strided-then-restored pair's stand-in (stride
    cannot keep the array's size, so dilation 2 sits in the middle) and an even-sized one that it does not."""
    return nn.Sequential(nn.Conv2d(f_dim, 8, 3, padding=1), nn.ReLU(),
                         nn.Conv2d(8, 8, 3, padding=2, dilation=2), nn.BatchNorm2d(8), nn.ReLU(),
                         nn.Conv2d(8, 8, 2, padding='same'), nn.ReLU(),
                         nn.Conv2d(8, c, (3, 5), padding=(1, 2)))


@contextlib.contextmanager
def _route_counts():
    """How many layers went to GF.gridconv and how many device tensors to torch's nn.Conv2d forward."""
    from gridnext_amd import functional as GF
    counts = {'hip': 0, 'torch': 0}
    real_gc, real_fw = GF.gridconv, nn.Conv2d._conv_forward

    def gc(*a, **k):
        counts['hip'] += 1
        return real_gc(*a, **k)

    def fw(self, x, *a, **k):
        counts['torch'] += int(x.is_cuda)
        return real_fw(self, x, *a, **k)
    GF.gridconv, nn.Conv2d._conv_forward = gc, fw
    try:
        yield counts
    finally:
        GF.gridconv, nn.Conv2d._conv_forward = real_gc, real_fw


@pytest.mark.timeout(120)
def test_ineligible_layers_fall_back_to_torch_and_match_fp64(capsys):
    import gridnext_amd as ga
    from gridnext_amd import functional as GF
    from gridnext_amd.synthetic import count_mlp
    from oracle import gridnet as ogn, masked_ce as oce

    class Odd(ga.GridNet):
        def _init_corrector(self):
            return _odd_corrector(self.f_dim, self.n_classes)

    class OddTwin(ogn.GridNet):
        def _init_corrector(self):
            return _odd_corrector(self.f_dim, self.n_classes)
    C, hw, B = 6, (35, 33), 2
    with _oracle_threads():
        torch.manual_seed(9)
        m = Odd(count_mlp(FULL_G, C), (FULL_G,), hw, C)
        for p in m.patch_classifier.parameters():
            p.requires_grad = False
        om = _oracle_twin(m, OddTwin)
        m.to(DEV)
        for mod in (m, om):
            mod.train()
            mod.patch_classifier.eval()
        x, y = _arrays(range(700, 700 + B), C, hw)
        with _route_counts() as counts:
            logits = m.forward_nhwc(x.to(DEV))
        assert counts == {'hip': 2, 'torch': 2}, counts
        loss, _, _ = GF.masked_cross_entropy(logits.reshape(-1, C), y.to(DEV), 1)
        loss.backward()
        ref = oce.masked_ce(om(x.double()), y, 1)[0]
        ref.backward()
        torch.cuda.synchronize()
        n = _gate_grads_and_stats(m, om, loss.item(), ref.item(), 'custom corrector with torch fallbacks, one step', capsys)
    assert n == 4 * 2 + 2


def test_eligible_layer_in_a_hex_corrector_takes_the_hip_route():
    import gridnext_amd as ga
    import gridnext_amd.hexconv as hexagdly
    import hex_radius_ref as R
    from gridnext_amd.synthetic import count_mlp
    from oracle import gridnet as ogn

    def corrector(f_dim, c, hexconv):
        return nn.Sequential(hexconv(f_dim, 16), nn.Conv2d(16, 16, 3, padding=1), nn.BatchNorm2d(16), nn.ReLU(), hexconv(16, c))

    class Mixed(ga.GridNetHex):                  # (hexagdly addressing: the oracle's odd-right class rotates the grid under g)
        def _init_corrector(self):
            return corrector(self.f_dim, self.n_classes, lambda i, o: hexagdly.Conv2d(i, o, kernel_size=1, stride=1, bias=True))

    class MixedTwin(ogn.GridNetHex):
        def _init_corrector(self):
            return corrector(self.f_dim, self.n_classes, lambda i, o: R.HexConvK64(i, o, 1))
    G, C, hw = 40, 4, (9, 8)
    torch.manual_seed(4)
    m = Mixed(count_mlp(G, C), (G,), hw, C)
    om = _oracle_twin(m, MixedTwin)
    m.to(DEV).eval()
    om.eval()
    x = torch.randint(0, 10, (2,) + hw + (G,)).float()
    with torch.no_grad(), _route_counts() as counts:
        out = m(x.to(DEV))
    assert counts == {'hip': 1, 'torch': 0}, counts
    with torch.no_grad():
        ref = om(x.double())
    assert (out.double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_all_fgd_predictions_on_a_hip_gridnet():
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    from gridnext_amd.utils import all_fgd_predictions
    G, C, hw = 50, 5, (12, 9)
    torch.manual_seed(12)
    m = ga.GridNet(count_mlp(G, C), (G,), hw, C)
    g = torch.Generator().manual_seed(2)
    x, y = torch.rand(4, hw[0], hw[1], G, generator=g), torch.randint(0, C + 1, (4,) + hw, generator=g)
    dl = DataLoader(TensorDataset(x, y), batch_size=2)
    with _route_counts() as counts:
        true, pred, smax = all_fgd_predictions(dl, m)
    assert counts == {'hip': 8, 'torch': 0}, counts
    assert next(m.parameters()).is_cuda and not m.training
    with torch.no_grad():
        rows = torch.cat([m(xb.to(DEV)).permute(0, 2, 3, 1).reshape(-1, C) for xb, _ in dl])
    keep = (y.reshape(-1) > 0)
    np.testing.assert_array_equal(true, (y.reshape(-1)[keep] - 1).numpy())
    np.testing.assert_allclose(smax, torch.softmax(rows, 1).cpu()[keep].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(pred, torch.argmax(rows, 1).cpu()[keep].numpy())
