"""The gradient of a DenseNet with respect to its input patches on the HIP path (gnx_conv0_dgrad behind densenet_train's stem
backward), at model level: both BatchNorm modes, a frozen network, DenseNet-121, the recompute paths, `mfma = 'f16'`, a module
with parameters in front of the DenseNet inside a grid model, and `utils.patch_saliency`.

Networks are randomly initialised (oracle.densenet.init_state, seeded): the closed-form state has pre-activations that are
exactly zero, which flip ReLU masks at rounding level.  The bar is the project's own (test_gpu_models.py,
test_densenet121_gradients_as_accurate_as_fp32_reference): per tensor, the HIP gradient is as close to the float64 oracle as the
oracle's own fp32 CPU run is - err_hip <= max(4 err_cpu32, 1e-3 max |ref|)."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

TINY_LARGE = dict(growth_rate=4, block_config=(2, 2), num_init_features=8, bn_size=2, num_classes=5,
                  small_inputs=False)
TINY_SMALL = dict(growth_rate=6, block_config=(2, 3, 2), num_init_features=10, bn_size=2, num_classes=7,
                  small_inputs=True, classify=False, compression=0.5)
NETS = {'tiny_large': (TINY_LARGE, 32), 'tiny_small': (TINY_SMALL, 16)}


def meets_bar(got, ref64, ref32, what):
    """err_hip <= max(4 err_cpu32, 1e-3 max |ref|), errors as the largest absolute difference from the float64 oracle."""
    got, ref32 = got.detach().double().cpu(), ref32.detach().double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err_hip, err_cpu = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    floor = 1e-3 * ref64.abs().max().item()
    print(' %s: err_hip %.3e, err_cpu32 %.3e, max |ref| %.3e' % (what, err_hip, err_cpu, ref64.abs().max().item()))
    assert err_hip <= max(4 * err_cpu, floor), (what, err_hip, err_cpu, floor)


def _cfg(kw):
    from oracle import densenet as odn
    return odn.DenseNetCfg(**{k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()})


@functools.lru_cache(maxsize=None)
def _state(name, seed=0):
    """(cfg, state dict) of a randomly initialised net: 'tiny_large', 'tiny_small' or 'densenet121'.  Shared: not written to."""
    from oracle import densenet as odn
    cfg = odn.DenseNetCfg(num_classes=8, **odn.DENSENET121) if name == 'densenet121' else _cfg(NETS[name][0])
    return cfg, odn.init_state(cfg, torch.Generator().manual_seed(1234 + seed))


def patches(n, P, seed=0):
    return torch.rand(n, 3, P, P, generator=torch.Generator().manual_seed(77 + seed))


def oracle_grads(cfg, sd, x, labels, training, dtype):
    """(dx, {key: gradient}, logits) of cross_entropy(forward(x), labels) from the CPU oracle in `dtype`."""
    from oracle import densenet as odn
    ref_sd = {}
    for k, v in sd.items():
        v = v.to(dtype).clone() if v.is_floating_point() else v.clone()
        ref_sd[k] = v.requires_grad_(True) if v.is_floating_point() and 'running' not in k else v
    xr = x.to(dtype).clone().requires_grad_(True)
    out = odn.forward(ref_sd, xr, cfg, training=training)
    F.cross_entropy(out, labels).backward()
    return xr.grad.double(), {k: v.grad.double() for k, v in ref_sd.items() if v.is_floating_point() and v.grad is not None}, out.detach()


@functools.lru_cache(maxsize=None)
def _oracle(name, n, P, training):
    cfg, sd = _state(name)
    x, labels = patches(n, P), torch.arange(n) % 5
    return oracle_grads(cfg, sd, x, labels, training, torch.float64), oracle_grads(cfg, sd, x, labels, training, torch.float32)


def hip_net(name, **attrs):
    import gridnext_amd as ga
    from oracle import densenet as odn
    _, sd = _state(name)
    m = ga.DenseNet(num_classes=8, **odn.DENSENET121) if name == 'densenet121' else ga.DenseNet(**NETS[name][0])
    m.load_state_dict(sd)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m.to(DEV)


def hip_grads(m, x, labels, x_grad=True):
    m.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(x_grad)
    F.cross_entropy(m(xd), labels.to(DEV)).backward()
    return xd.grad, {k: p.grad for k, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------ 1. tiny nets, both modes
@pytest.mark.parametrize('training', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('name', ['tiny_large', 'tiny_small'])
def test_tiny_nets_input_and_parameter_gradients(name, training):
    """5 spots: x.grad and every parameter gradient against the float64 oracle, and the parameter gradients bit-equal to those
    of the same call whose input asks for no gradient - the feature does not perturb the path that exists."""
    P = NETS[name][1]
    (dx64, g64, _), (dx32, g32, _) = _oracle(name, 5, P, training)
    x, labels = patches(5, P), torch.arange(5) % 5
    m = hip_net(name).train(training)
    dx, grads = hip_grads(m, x, labels)
    assert dx is not None and dx.shape == (5, 3, P, P)
    meets_bar(dx, dx64, dx32, 'x.grad')
    grads = {k: g for k, g in grads.items() if g is not None}        # (classify = False: the classifier takes no part)
    assert set(grads) == set(g64)
    for k, g in grads.items():
        meets_bar(g, g64[k], g32[k], k)
    none, grads0 = hip_grads(m, x, labels, x_grad=False)
    assert none is None
    for k, g in grads.items():
        assert torch.equal(g, grads0[k]), k


# ------------------------------------------------------------------------------------------------ 2. frozen, eval mode
@pytest.mark.parametrize('name', ['tiny_large', 'tiny_small'])
def test_frozen_network_gives_only_the_input_gradient(name):
    P = NETS[name][1]
    (dx64, _, _), (dx32, _, _) = _oracle(name, 5, P, False)
    m = hip_net(name).eval().requires_grad_(False)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    dx, grads = hip_grads(m, patches(5, P), torch.arange(5) % 5)
    meets_bar(dx, dx64, dx32, 'x.grad')
    assert all(g is None for g in grads.values())
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())


# ------------------------------------------------------------------------------------------------ 3. DenseNet-121
def test_densenet121_input_gradient():
    """8 spots of 64 px, eval mode, direct-form conv2: O = 64, the full-width kernels on the way down to the stem."""
    (dx64, _, _), (dx32, _, _) = _oracle('densenet121', 8, 64, False)
    m = hip_net('densenet121', winograd=False).eval()
    dx, _ = hip_grads(m, patches(8, 64), torch.arange(8) % 5)
    meets_bar(dx, dx64, dx32, 'x.grad')


# ------------------------------------------------------------------------------------------------ 4. recompute paths
def test_recompute_paths_give_the_taped_input_gradient():
    """`efficient = True` (one recomputed chunk) and a `tape_budget` that forces chunks of 8 over 24 spots: x.grad has the bits
    of the taped call (eval mode: spots are independent)."""
    from gridnext_amd.densenet_train import tape_bytes_per_spot
    x, labels = patches(24, 32, seed=1), torch.arange(24) % 5
    m = hip_net('tiny_large').eval()
    taped, _ = hip_grads(m, x, labels)
    assert taped is not None
    m.efficient = True
    eff, _ = hip_grads(m, x, labels)
    assert torch.equal(eff, taped)
    m.efficient = False
    m.tape_budget = 8 * tape_bytes_per_spot(m, 32)
    chunked, _ = hip_grads(m, x, labels)
    assert torch.equal(chunked, taped)


# ------------------------------------------------------------------------------------------------ 5. mfma = 'f16'
def test_f16_model_takes_the_fp32_tape_for_an_input_gradient():
    """`mfma = 'f16'` with an input that requires grad, on a call the fp16 tape DOES take when the input requires none:
    DenseNet-121, 8 spots of 128 px, eval mode.  densenet_train_f16.eligible declines it for the input's sake only, `_f16_pad`
    pads nothing for it, and the call runs the fp32 tape - with `winograd = False` the same kernels as `mfma = 'f32'` (whose
    taped forward would otherwise take the Winograd conv2), so the same bits; `efficient = True` picks the same tape in its
    forward and in its recompute and gives them again."""
    from gridnext_amd import densenet_train as dt, densenet_train_f16 as f16
    x, labels = patches(8, 128, seed=2), torch.arange(8) % 5
    m = hip_net('densenet121', winograd=False).eval()
    dx32, _ = hip_grads(m, x, labels)
    assert dx32 is not None and bool(torch.isfinite(dx32).all()) and bool((dx32 != 0).any())
    m.mfma = 'f16'
    xd = x.to(DEV)
    assert f16.eligible(m, xd) and dt._taped(m, xd) is f16._DenseNetF16Fn             # the fp16 tape is this call's, but for ...
    xg = xd.clone().requires_grad_(True)
    assert not f16.eligible(m, xg) and dt._taped(m, xg) is dt._DenseNetFn             # ... an input that requires grad
    assert m._f16_pad(xd[:5]) == 3 and m._f16_pad(xg[:5]) == 0
    dx16, _ = hip_grads(m, x, labels)
    assert dx16 is not None and torch.equal(dx16, dx32)
    m.efficient = True
    dxe, _ = hip_grads(m, x, labels)
    assert dxe is not None and torch.equal(dxe, dx32)


# ------------------------------------------------------------------------------------------------ 6. a module in front
class Affine(nn.Module):
    """A learnable per-channel scale and offset: a stand-in for a stain normalisation in front of the patch classifier."""

    def __init__(self, channels):
        super().__init__()
        self.scale = nn.Parameter(torch.linspace(0.8, 1.2, channels))
        self.offset = nn.Parameter(torch.linspace(-0.1, 0.1, channels))

    def forward(self, x):
        return x * self.scale.view(1, -1, 1, 1) + self.offset.view(1, -1, 1, 1)


GRID_HW, GRID_C, GRID_P = (4, 4), 5, 32


def grid_inputs():
    g = torch.Generator().manual_seed(9)
    x = torch.rand((1,) + GRID_HW + (3, GRID_P, GRID_P), generator=g)
    y = torch.randint(0, GRID_C + 1, (1,) + GRID_HW, generator=g)
    y[0, 0, 0], y[0, 1, 2] = 1, 3                                    # foreground for certain
    return x, y


def hip_grid(front, limit):
    import gridnext_amd as ga
    torch.manual_seed(21)                                            # the corrector's initial weights
    f = hip_net('tiny_large')
    f = nn.Sequential(Affine(3), f) if front else f
    return ga.GridNetHexOddr(f, (3, GRID_P, GRID_P), GRID_HW, GRID_C, atonce_patch_limit=limit).to(DEV)


@functools.lru_cache(maxsize=None)
def _oracle_affine_grads():
    """Affine's gradients from the same model built from the oracle, in float64 and in float32, + the corrector it used."""
    from oracle import densenet as odn, gridnet as ogn, masked_ce as oce
    m = hip_grid(True, None)
    x, y = grid_inputs()
    res = []
    for dtype in (torch.float64, torch.float32):
        of = odn.DenseNet(**TINY_LARGE)
        of.load_named_state(_state('tiny_large')[1])
        og = ogn.GridNetHexOddr(nn.Sequential(Affine(3), of), (3, GRID_P, GRID_P), GRID_HW, GRID_C)
        og.corrector.load_state_dict({k: v.cpu() for k, v in m.corrector.state_dict().items()})
        og.to(dtype).train()
        og.patch_classifier.eval()
        loss, _, _ = oce.masked_ce(og(x.to(dtype)), y, 1)
        loss.backward()
        res.append((og.patch_classifier[0].scale.grad.double(), og.patch_classifier[0].offset.grad.double(), loss.item()))
    return res


@pytest.mark.parametrize('limit', [None, 7], ids=['whole', 'chunks_of_7'])
def test_module_in_front_of_the_densenet_gets_its_gradient(limit):
    """patch_classifier = Sequential(Affine, DenseNet) inside GridNetHexOddr, 4 x 4 grid, one array: the masked cross-entropy of
    forward(x) back-propagated to Affine's scale and offset - through the corrector, the DenseNet and its input gradient."""
    from gridnext_amd import functional as GF
    (s64, o64, loss64), (s32, o32, loss32) = _oracle_affine_grads()
    m = hip_grid(True, limit)
    m.train()
    m.patch_classifier.eval()
    x, y = grid_inputs()
    logits = m.forward_nhwc(x.to(DEV))
    loss, _, _ = GF.masked_cross_entropy(logits.reshape(-1, GRID_C), y.to(DEV), 1)
    loss.backward()
    assert abs(loss.item() - loss64) <= max(4 * abs(loss32 - loss64), 1e-4), (loss.item(), loss64, loss32)
    aff = m.patch_classifier[0]
    meets_bar(aff.scale.grad, s64, s32, 'Affine.scale.grad')
    meets_bar(aff.offset.grad, o64, o32, 'Affine.offset.grad')


def test_grid_model_chunks_give_the_unchunked_input_gradient():
    """A bare DenseNet as f, the array itself requires grad: with atonce_patch_limit = 7 the 16 spots go through checkpointed
    chunks of 7, 7 and 2 (densenet_recompute) and x.grad has the bits of the unchunked call (eval mode)."""
    from gridnext_amd import functional as GF
    x, y = grid_inputs()
    got = {}
    for limit in (None, 7):
        m = hip_grid(False, limit).eval()
        xd = x.to(DEV).requires_grad_(True)
        loss, _, _ = GF.masked_cross_entropy(m.forward_nhwc(xd).reshape(-1, GRID_C), y.to(DEV), 1)
        loss.backward()
        got[limit] = xd.grad
        assert xd.grad is not None and xd.grad.shape == x.shape and bool((xd.grad != 0).any())
    assert torch.equal(got[7], got[None])


# ------------------------------------------------------------------------------------------------ 7. patch_saliency
def test_patch_saliency():
    from gridnext_amd.utils import patch_saliency
    from oracle import densenet as odn
    cfg, sd = _state('tiny_large')
    x = patches(6, 32, seed=3)
    m = hip_net('tiny_large')
    m.train()                                                # the mode to come back to
    frozen = [p for i, p in enumerate(m.parameters()) if i % 3 == 0]
    for p in frozen:
        p.requires_grad_(False)
    marked = [p for i, p in enumerate(m.parameters()) if i % 3 == 1]
    for p in marked:
        p.grad = torch.full_like(p, 0.25)
    flags = [p.requires_grad for p in m.parameters()]
    buffers = {k: v.clone() for k, v in m.named_buffers()}
    with torch.no_grad():
        m.eval()
        targets = m(x.to(DEV)).argmax(1)
        m.train()
    sal = patch_saliency(m, x.to(DEV))
    assert sal.shape == (6, 32, 32) and sal.dtype == torch.float32
    assert torch.equal(sal, patch_saliency(m, x.to(DEV), targets))            # the default targets: the argmax
    other = patch_saliency(m, x.to(DEV), (targets + 1) % 5)
    assert not torch.equal(other, sal)
    # ... and the classifier is as it was
    assert m.training and all(mod.training for mod in m.modules())
    assert [p.requires_grad for p in m.parameters()] == flags
    for i, p in enumerate(m.parameters()):
        if i % 3 == 1:
            assert torch.equal(p.grad, torch.full_like(p, 0.25))
        else:
            assert p.grad is None
    assert all(torch.equal(v, buffers[k]) for k, v in m.named_buffers())
    # against the oracle: max over the colour channels of |d logit[target] / d patch|
    ref = []
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).requires_grad_(True)
        out = odn.forward({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, xr, cfg, training=False)
        g, = torch.autograd.grad(out.gather(1, targets.cpu().view(-1, 1)).sum(), xr)
        ref.append(g.abs().amax(1).double())
    meets_bar(sal, ref[0], ref[1], 'saliency')
    # mixed modes come back module by module: a module in front in train mode, the DenseNet in eval mode (the loops' own
    # arrangement), one of its BatchNorms in train mode again
    seq = nn.Sequential(Affine(3).to(DEV), m).train()
    m.eval()
    m.features.norm_final.train()
    modes = [mod.training for mod in seq.modules()]
    assert any(modes) and not all(modes)
    front = patch_saliency(seq, x.to(DEV), targets)
    assert front.shape == (6, 32, 32) and not torch.equal(front, sal)
    assert [mod.training for mod in seq.modules()] == modes
    assert seq[0].scale.grad is None and '_input_grad_only' not in m.__dict__
    m.train()
    # uint8 patches with input_norm: the saliency of the floats the classifier's own conversion gives
    m.input_norm = ([0.6, 0.5, 0.4], [0.25, 0.2, 0.3])
    xu = (x * 255).round().to(torch.uint8).to(DEV)
    floats = m._float_patches(xu)
    assert floats.dtype == torch.float32 and not torch.equal(floats, xu.float() / 255)
    assert torch.equal(patch_saliency(m, xu, targets), patch_saliency(m, floats, targets))
