"""GPU: radius-k hexagonal convolutions (hexagdly.Conv2d(kernel_size=k); gnx_hexconv_k_*) against float64.

 * kernels: y, dx, every dkernel{j} and dbias against the float64 gather form of tests/hex_radius_ref.py at each contraction's
   rounding bound (y: T I terms, dx: T O, weights and bias: B H W), k = 1..4 and 6, both addressings, matrix-core widths
   (8/16/32/64) and chunked ones (1/3/33/70/130), whole 78 x 64 arrays down to 1 x 1; `accumulate`, NULL destinations and
   repeatability; k = 1 against the size-1 entry points;
 * the module and its autograd node, frozen kernels and bias included;
 * one whole-array step of GridNetHexOddr / GridNetHex subclasses whose corrector mixes k = 2 and k = 1 layers, and
   train_gridwise replayed from a captured step, against the float64 oracle; replayed == eager bit for bit.
"""
import contextlib
import copy
import ctypes
import io
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

import hex_radius_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KMAX = 8


@pytest.fixture(scope='module')
def L():
    from gridnext_amd import _lib
    return _lib


def _rounding_gate(got, ref, length, what, c=32.0):
    """max |got - ref| <= c * sqrt(length) * 2^-24 * max |ref|: the rounding bound of an fp32 contraction of `length` terms
    against a float64 reference (the rule of tests/test_gpu_kernels.py:_rounding_gate).  Returns error / gate."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    gate = c * length ** 0.5 * 2.0 ** -24 * (ref.abs().max().item() if ref.numel() else 0.0)
    assert err <= gate, "%s: max abs err %.3e > gate %.3e (%.1f x the gate)" % (what, err, gate, err / max(gate, 1e-300))
    return err / gate if gate > 0 else 0.0


def _ptrs(L, ts):
    return (ctypes.c_void_p * len(ts))(*[L.ptr(t) for t in ts])


def _reference(x, ks, b, dy, mode):
    """float64 (y, dx, dkernels, dbias) in the GPU's channels-last layout; x / dy: [B, H, W, C]."""
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    kr = [t.double().clone().requires_grad_(True) for t in ks]
    br = b.double().clone().requires_grad_(True)
    y = R.oddr(R.gather_k, xr, kr, br) if mode else R.gather_k(xr, kr, br)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), [t.grad for t in kr], br.grad


def _case(B, H, W, I, O, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, I, generator=g)
    ks = [torch.randn(s, generator=g) * (R.n_taps(k) * I) ** -0.5 for s in R.kernel_shapes(O, I, k)]
    b = torch.randn(O, generator=g)
    dy = torch.randn(B, H, W, O, generator=g)
    return x, ks, b, dy


def _run(L, x, ks, b, dy, k, mode, dks=None, db=None, accumulate=0):
    B, H, W, I = x.shape
    O = ks[0].shape[0]
    y, dx = torch.empty(B, H, W, O, device=DEV), torch.empty(B, H, W, I, device=DEV)
    kp = _ptrs(L, ks)
    L.call('gnx_hexconv_k_fwd', L.ptr(x), ctypes.addressof(kp), L.ptr(b), L.ptr(y), B, H, W, I, O, k, mode, L.stream())
    L.call('gnx_hexconv_k_bwd_data', L.ptr(dy), ctypes.addressof(kp), L.ptr(dx), B, H, W, I, O, k, mode, L.stream())
    if dks is None:
        dks, db = [torch.empty_like(t) for t in ks], torch.empty(O, device=DEV)
    ws = torch.empty(max(1, L.query('gnx_hexconv_k_bwd_weight_workspace', B, H, W, I, O, k)), device=DEV)
    dp = _ptrs(L, dks)
    L.call('gnx_hexconv_k_bwd_weight', L.ptr(x), L.ptr(dy), ctypes.addressof(dp), L.ptr(db), L.ptr(ws), B, H, W, I, O, k, mode,
           accumulate, L.stream())
    torch.cuda.synchronize()
    return y, dx, dks, db


FULL = [(1, 78, 64, I, O) for I, O in ((16, 32), (32, 32), (32, 7), (14, 32))]
SMALL = [(2, 7, 5, 8, 16), (1, 11, 3, 64, 8), (1, 1, 1, 16, 64), (1, 2, 3, 33, 3), (3, 5, 9, 1, 70), (1, 9, 7, 130, 33),
         (1, 6, 5, 70, 130)]
CASES = [(s, k, mode) for k in (1, 2, 3, 4) for mode in (0, 1) for s in FULL + SMALL] + \
        [(s, 6, mode) for mode in (0, 1) for s in [(1, 78, 64, 32, 32), (2, 7, 5, 8, 16), (1, 9, 7, 130, 33), (1, 1, 1, 3, 1)]]


@pytest.mark.parametrize("shape,k,mode", CASES, ids=["%dx%dx%d %d->%d k%d m%d" % (s + (k, m)) for s, k, m in CASES])
def test_hexconv_k_kernels_against_fp64(L, shape, k, mode):
    B, H, W, I, O = shape
    T = R.n_taps(k)
    x, ks, b, dy = _case(B, H, W, I, O, k, seed=hash((shape, k, mode)) % 100003)
    yr, dxr, dkr, dbr = _reference(x, ks, b, dy, mode)
    xd, kd, bd, dyd = x.to(DEV), [t.to(DEV) for t in ks], b.to(DEV), dy.to(DEV)
    y, dx, dks, db = _run(L, xd, kd, bd, dyd, k, mode)
    _rounding_gate(y, yr, T * I, 'y')
    _rounding_gate(dx, dxr, T * O, 'dx')
    for j, (a, r) in enumerate(zip(dks, dkr)):
        _rounding_gate(a, r, B * H * W, 'dkernel%d' % j)
    _rounding_gate(db, dbr, B * H * W, 'dbias')
    # two calls: the same bits
    y2, dx2, dks2, db2 = _run(L, xd, kd, bd, dyd, k, mode)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(db, db2)
    assert all(torch.equal(a, c) for a, c in zip(dks, dks2))
    # accumulate = 1 adds onto the destination; NULL destinations (every other kernel, the bias) are left untouched
    base = [torch.full_like(t, 0.5) for t in kd]
    acc = [t.clone() for t in base]
    _run(L, xd, kd, bd, dyd, k, mode, dks=acc, db=torch.full((O,), 0.5, device=DEV), accumulate=1)
    for j in range(k + 1):
        assert torch.equal(acc[j], base[j] + dks[j]), 'accumulate: dkernel%d' % j
    sentinel = [torch.full_like(t, 7.0) for t in kd]
    part = [None if j % 2 else sentinel[j] for j in range(k + 1)]
    _run(L, xd, kd, bd, dyd, k, mode, dks=part, db=None)
    for j in range(k + 1):
        assert torch.equal(sentinel[j], torch.full_like(sentinel[j], 7.0) if j % 2 else dks[j]), 'NULL dkernels: %d' % j
    if k == 1:
        # the size-1 entry points on the same inputs, within the same bound
        y1, dx1 = torch.empty_like(y), torch.empty_like(dx)
        dk01, dk11, db1 = torch.empty_like(kd[0]), torch.empty_like(kd[1]), torch.empty_like(bd)
        L.call('gnx_hexconv_fwd', L.ptr(xd), L.ptr(kd[0]), L.ptr(kd[1]), L.ptr(bd), L.ptr(y1), B, H, W, I, O, mode, L.stream())
        L.call('gnx_hexconv_bwd_data', L.ptr(dyd), L.ptr(kd[0]), L.ptr(kd[1]), L.ptr(dx1), B, H, W, I, O, mode, L.stream())
        ws = torch.empty(L.query('gnx_hexconv_bwd_weight_workspace', B, H, W, I, O), device=DEV)
        L.call('gnx_hexconv_bwd_weight', L.ptr(xd), L.ptr(dyd), L.ptr(dk01), L.ptr(dk11), L.ptr(db1), L.ptr(ws), B, H, W, I, O,
               mode, 0, L.stream())
        torch.cuda.synchronize()
        _rounding_gate(y, y1, T * I, 'y vs size-1')
        _rounding_gate(dx, dx1, T * O, 'dx vs size-1')
        _rounding_gate(dks[0], dk01, B * H * W, 'dkernel0 vs size-1')
        _rounding_gate(dks[1], dk11, B * H * W, 'dkernel1 vs size-1')
        _rounding_gate(db, db1, B * H * W, 'dbias vs size-1')


def test_hexconv_k_argument_checks(L):
    x = torch.randn(1, 4, 4, 8, device=DEV)
    y = torch.empty(1, 4, 4, 8, device=DEV)
    for k, rc in ((KMAX + 1, L.ERR_UNSUPPORTED), (0, -1)):
        ks = [torch.zeros(s, device=DEV) for s in R.kernel_shapes(8, 8, max(k, 1))]
        kp = _ptrs(L, ks)
        assert L.query('gnx_hexconv_k_fwd', L.ptr(x), ctypes.addressof(kp), None, L.ptr(y), 1, 4, 4, 8, 8, k, 0, L.stream()) == rc
        assert L.query('gnx_hexconv_k_bwd_data', L.ptr(x), ctypes.addressof(kp), L.ptr(y), 1, 4, 4, 8, 8, k, 0, L.stream()) == rc
        assert L.query('gnx_hexconv_k_bwd_weight', L.ptr(x), L.ptr(x), ctypes.addressof(kp), None, L.ptr(y), 1, 4, 4, 8, 8, k, 0,
                       0, L.stream()) == rc
    ks = [torch.zeros(s, device=DEV) for s in R.kernel_shapes(8, 8, 2)]
    kp = _ptrs(L, ks[:2] + [None])
    assert L.query('gnx_hexconv_k_fwd', L.ptr(x), ctypes.addressof(kp), None, L.ptr(y), 1, 4, 4, 8, 8, 2, 0, L.stream()) == -1


# ------------------------------------------------------------------------------------------------ module and autograd
@pytest.mark.parametrize("k,oddr", [(2, False), (3, True), (2, True)])
def test_module_forward_backward_against_fp64_twin(k, oddr):
    import gridnext_amd.hexconv as hexagdly
    torch.manual_seed(5 + k)
    m = hexagdly.Conv2d(16, 24, kernel_size=k)
    twin = R.HexConvK64(16, 24, k)
    twin.load_state_dict({n: t.double() for n, t in m.state_dict().items()})
    x = torch.randn(2, 16, 13, 10)
    dy = torch.randn(2, 24, 13, 10)
    xr = x.double().requires_grad_(True)
    ref = (twin(xr.transpose(2, 3)).transpose(2, 3) if oddr else twin(xr))
    ref.backward(dy.double())
    m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    if oddr:                                       # GridNetHexOddr's channels-last entry on the Visium grid
        y = m.forward_nhwc(xd.permute(0, 2, 3, 1), oddr=True).permute(0, 3, 1, 2)
    else:
        y = m(xd)
    y.backward(dy.to(DEV))
    T = R.n_taps(k)
    _rounding_gate(y, ref, T * 16, 'y')
    _rounding_gate(xd.grad, xr.grad, T * 24, 'dx')
    for (n, p), (_, q) in zip(m.named_parameters(), twin.named_parameters()):
        _rounding_gate(p.grad, q.grad, 2 * 13 * 10, n)


def test_frozen_kernel_and_bias_get_no_gradient():
    import gridnext_amd.hexconv as hexagdly
    torch.manual_seed(8)
    m = hexagdly.Conv2d(8, 32, kernel_size=3)
    twin = R.HexConvK64(8, 32, 3)
    twin.load_state_dict({n: t.double() for n, t in m.state_dict().items()})
    for mod in (m, twin):
        mod.kernel1.requires_grad_(False)
        mod.bias_tensor.requires_grad_(False)
    x, dy = torch.randn(1, 8, 9, 11), torch.randn(1, 32, 9, 11)
    twin(x.double()).backward(dy.double())
    m.to(DEV)
    m(x.to(DEV)).backward(dy.to(DEV))
    assert m.kernel1.grad is None and m.bias_tensor.grad is None
    for n in ('kernel0', 'kernel2', 'kernel3'):
        _rounding_gate(getattr(m, n).grad, getattr(twin, n).grad, 9 * 11, n)


# ------------------------------------------------------------------------------------------------ model level
FULL_G, FULL_C, FULL_HW = 2000, 8, (78, 64)


def _mixed_corrector(f_dim, n_classes, conv):
    """A custom corrector as a user writes one: the default's shape, its first layer of each pair widened to radius 2."""
    return nn.Sequential(conv(f_dim, 32, 2), conv(32, 32, 1), nn.BatchNorm2d(32), nn.ReLU(),
                         conv(32, 32, 2), conv(32, 32, 1), nn.BatchNorm2d(32), nn.ReLU(),
                         conv(32, n_classes, 1))


def _hip_models():
    import gridnext_amd as ga
    import gridnext_amd.hexconv as hexagdly

    def conv(i, o, k):
        return hexagdly.Conv2d(i, o, kernel_size=k, stride=1, bias=True)

    class WideHexOddr(ga.GridNetHexOddr):
        def _init_corrector(self):
            return _mixed_corrector(self.f_dim, self.n_classes, conv)

    class WideHex(ga.GridNetHex):
        def _init_corrector(self):
            return _mixed_corrector(self.f_dim, self.n_classes, conv)
    return WideHexOddr, WideHex


def _oracle_twin(m, oddr):
    """The float64 oracle twin of a (CPU-resident) HIP model: same weights, same frozen parameters."""
    from oracle import gridnet as ogn
    base = ogn.GridNetHexOddr if oddr else ogn.GridNetHex

    class Twin(base):
        def _init_corrector(self):
            return _mixed_corrector(self.f_dim, self.n_classes, lambda i, o, k: R.HexConvK64(i, o, k))
    om = Twin(copy.deepcopy(m.patch_classifier), m.patch_shape, m.grid_shape, m.n_classes, use_bn=m.use_bn)
    om.corrector.load_state_dict(m.corrector.state_dict())
    for p, q in zip(m.corrector.parameters(), om.corrector.parameters()):
        q.requires_grad_(p.requires_grad)
    return om.double()


@contextlib.contextmanager
def _oracle_threads():
    keep = torch.get_num_threads()
    torch.set_num_threads(int(os.environ.get('OMP_NUM_THREADS', '8')))
    try:
        yield
    finally:
        torch.set_num_threads(keep)


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


def _align_oracle_relus(om, masks, oddr):
    """Forward hooks on the oracle's ReLUs: a pre-activation within 1e-5 of its tensor's range of 0 takes the HIP path's side of
    the kink (an O(dy) difference there says nothing about either side; farther from the kink a disagreement fails) - the rule
    of the full-grid tests in tests/test_gpu_models.py.  Returns (per ReLU [elements aligned, largest |x| / range], hooks)."""
    aligned = []

    def hook(mod, inp, out):
        x = inp[0]
        hip = masks[len(aligned)]
        if x.dim() == 4:
            B, C = x.shape[0], x.shape[1]
            if oddr:                               # the oracle's corrector runs on the rot90/flip of the Visium grid
                H, W = x.shape[3], x.shape[2]
                hip = torch.flip(torch.rot90(hip.reshape(B, H, W, C).permute(0, 3, 1, 2), 1, [3, 2]), [3])
            else:
                hip = hip.reshape(B, x.shape[2], x.shape[3], C).permute(0, 3, 1, 2)
        hip = hip.reshape(x.shape)
        off = hip != (x.detach() > 0)
        rng = x.detach().abs().max().item()
        worst = x.detach()[off].abs().max().item() / rng if off.any() else 0.0
        aligned.append([int(off.sum()), worst])
        assert worst <= 1e-5, "ReLU %d: HIP mask differs from float64 %.2e of the range from 0" % (len(aligned) - 1, worst)
        return torch.where(off, x * hip.to(x.dtype), out)
    return aligned, [mod.register_forward_hook(hook) for mod in om.modules() if isinstance(mod, nn.ReLU)]


def _gate_grads_and_stats(m, om, ce, ce_ref, what, capsys):
    """Every corrector gradient within 1e-4 of its float64 range (the biases right before a train-mode BatchNorm, whose true
    gradient is 0: of their layer's kernel-gradient range), running statistics within 1e-4 of theirs, |dCE| <= 1e-4."""
    ref = dict(om.corrector.named_parameters())
    zero_true = {'%d.bias_tensor' % i: ['%d.kernel0' % i, '%d.kernel1' % i] for i in (1, 5)}
    worst, n = (0.0, ''), 0
    for name, p in m.corrector.named_parameters():
        q = ref[name]
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is None:
            continue
        scale = max(ref[w].grad.abs().max().item() for w in zero_true[name]) if name in zero_true else q.grad.abs().max().item()
        err = (p.grad.detach().double().cpu() - q.grad).abs().max().item()
        assert err <= 1e-4 * scale, "%s: max abs err %.3e > 1e-4 x %.3e" % (name, err, scale)
        worst = max(worst, (err / (1e-4 * scale), name))
        n += 1
    for a, b in zip(m.corrector.modules(), om.corrector.modules()):
        if isinstance(a, nn.BatchNorm2d):
            for buf in ('running_mean', 'running_var'):
                got, r = getattr(a, buf).double().cpu(), getattr(b, buf)
                assert (got - r).abs().max().item() <= 1e-4 * r.abs().max().item(), buf
    assert abs(ce - ce_ref) <= 1e-4, (ce, ce_ref)
    with capsys.disabled():
        print("\n[%s] CE hip %.7f fp64 %.7f; %d gradients, worst %s at %.3f x its gate" % (what, ce, ce_ref, n, worst[1], worst[0]))
    return n


@pytest.mark.timeout(180)
@pytest.mark.parametrize("oddr", [True, False])
def test_mixed_radius_corrector_full_grid_step_against_fp64(capsys, oddr):
    """One whole 78 x 64 array through a GridNetHexOddr (Visium grid) or GridNetHex (hexagdly addressing) subclass whose
    corrector mixes radius-2 and radius-1 layers with BatchNorm and ReLU, the count MLP frozen in eval mode: masked CE,
    every corrector gradient and the running statistics against the float64 oracle twin."""
    from gridnext_amd import functional as GF
    from gridnext_amd.synthetic import count_mlp, visium_array
    from oracle import masked_ce as oce
    WideHexOddr, WideHex = _hip_models()
    G, C = FULL_G, FULL_C
    with _oracle_threads():
        torch.manual_seed(61 + oddr)
        m = (WideHexOddr if oddr else WideHex)(count_mlp(G, C), (G,), FULL_HW, C, use_bn=True)
        for p in m.patch_classifier.parameters():
            p.requires_grad = False
        om = _oracle_twin(m, oddr)
        m.to(DEV)
        for mod in (m, om):
            mod.train()
            mod.patch_classifier.eval()
        _, xc, y = visium_array(300 + oddr, G, C, image=False)
        x = xc.unsqueeze(0) if oddr else xc.permute(1, 2, 0).contiguous().unsqueeze(0)   # (B, genes, H, W) | (B, H, W, genes)
        y = y.unsqueeze(0)
        with _hip_relu_masks() as masks:
            logits = m.forward_nhwc(x.to(DEV))
        loss, _, _ = GF.masked_cross_entropy(logits.reshape(-1, C), y.to(DEV), 1)
        loss.backward()
        aligned, hooks = _align_oracle_relus(om, masks, oddr)
        try:
            ref = oce.masked_ce(om(x.double()), y, 1)[0]
        finally:
            for h in hooks:
                h.remove()
        ref.backward()
        torch.cuda.synchronize()
        assert len(aligned) == len(masks) == 4
        n = _gate_grads_and_stats(m, om, loss.item(), ref.item(), 'mixed-radius corrector, %s, one step; ReLU elements '
                                  'aligned %s' % ('GridNetHexOddr' if oddr else 'GridNetHex', aligned), capsys)
    assert n == 4 + 3 + 2 + 4 + 3 + 2 + 3


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.mark.timeout(240)
def test_mixed_radius_corrector_train_gridwise_replayed_against_fp64(monkeypatch, capsys):
    """train_gridwise for 2 epochs on 4 train and 2 val whole arrays (batch 1, Adam on g, the count MLP frozen) with the
    mixed-radius GridNetHexOddr subclass: the step is captured after graphs.WARMUP eager ones and replayed (counted: an eager
    fallback fails); histories against oracle.loops.train_gridwise on the float64 twin (first train loss 1e-4, rtol 3e-4, as
    test_full_grid_train_gridwise_replayed_against_fp64); the replayed loop equals the GNX_GRAPH=0 loop bit for bit
    (histories, weights, running statistics)."""
    import warnings
    import gridnext_amd as ga
    from gridnext_amd import graphs
    from gridnext_amd.synthetic import count_mlp, visium_array
    from oracle import loops as oloops
    WideHexOddr, _ = _hip_models()
    G, C = FULL_G, FULL_C
    replays = {True: 0, False: 0}
    real_replay = graphs.GridStepGraph.replay

    def counting_replay(self, inputs, labels):
        replays[self.train] += 1
        return real_replay(self, inputs, labels)
    monkeypatch.setattr(graphs.GridStepGraph, 'replay', counting_replay)
    with _oracle_threads():
        arrays = [visium_array(400 + i, G, C, image=False) for i in range(6)]
        xs, ys = torch.stack([a[1] for a in arrays]), torch.stack([a[2] for a in arrays])
        del arrays
        torch.manual_seed(71)
        m0 = WideHexOddr(count_mlp(G, C), (G,), FULL_HW, C, use_bn=True)
        for p in m0.patch_classifier.parameters():
            p.requires_grad = False
        om = _oracle_twin(m0, True)
        lr = 1e-3
        crit = nn.CrossEntropyLoss()
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
                m, vh, th = _quiet(ga.train_gridwise, m, dl, crit, opt, num_epochs=2)
            failed = [str(w.message) for w in caught if 'capture failed' in str(w.message)]
            assert not failed, failed
            runs[flag] = (m, vh, th, {k: replays[k] - before[k] for k in replays})
        odl = {'train': DataLoader(TensorDataset(xs[:4].double(), ys[:4]), batch_size=1),
               'val': DataLoader(TensorDataset(xs[4:].double(), ys[4:]), batch_size=1)}
        o_opt = torch.optim.Adam(om.corrector.parameters(), lr=lr)
        om, ovh, oth = _quiet(oloops.train_gridwise, om, odl, nn.CrossEntropyLoss(), o_opt, num_epochs=2)
    m, vh, th, rep = runs['']
    assert rep == {True: 2 * 4 - graphs.WARMUP, False: 2 * 2 - graphs.WARMUP}, rep
    assert runs['0'][3] == {True: 0, False: 0}
    with capsys.disabled():
        print("\n[mixed-radius corrector, train_gridwise] train %s vs fp64 %s; val %s vs fp64 %s; replays %s"
              % (np.round(th, 7), np.round(oth, 7), np.round(vh, 7), np.round(ovh, 7), rep))
    assert abs(th[0] - oth[0]) <= 1e-4
    np.testing.assert_allclose(th, oth, rtol=3e-4)
    np.testing.assert_allclose(vh, ovh, rtol=3e-4)
    me, vhe, the, _ = runs['0']
    assert list(th) == list(the) and list(vh) == list(vhe)
    for (n, a), (_, b) in zip(m.state_dict().items(), me.state_dict().items()):
        assert torch.equal(a, b), "replayed and eager loops differ at %s" % n
