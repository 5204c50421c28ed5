"""`DenseNet.input_resize` / `input_crop`: the tutorials' Resize + CenterCrop in front of the classifier, on the device.

The reference for every test is THE SAME network with the switches off, fed the uint8 patches Pillow makes of the stored ones
on the host (tests/resize_ref.py: pillow_resize_crop).  Stored 146-px patches -> 128 px take the route that hands the fused
uint8 stems bytes; 40 -> 32 px takes the route that hands the float stems floats (gnx_resize_crop_u8_f32).  Every comparison
is torch.equal: logits, every parameter gradient, running statistics, saliency maps."""
import copy

import pytest
import torch

import resize_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
ROUTES = [(146, 128), (40, 32)]          # (stored px, network px): bytes to the fused uint8 stem / floats to the float stems

_STORE = {}


def _patches(n, P0, P, empty=()):
    """(stored uint8 patches on the device, Pillow's Resize(P) + CenterCrop(P) of them on the device), made once per shape."""
    key = (n, P0, P, tuple(empty))
    if key not in _STORE:
        host = R.patterns((n, 3, P0, P0), seed=n + P0)['random']
        for i in empty:
            host[i] = 0
        _STORE[key] = (torch.from_numpy(host).to(DEV), torch.from_numpy(R.pillow_resize_crop(host, P, P)).to(DEV))
    return _STORE[key]


def _tiny(C=4, seed=0):
    import gridnext_amd as ga
    torch.manual_seed(seed)
    f = ga.DenseNet(growth_rate=8, block_config=(2, 2), num_init_features=16, bn_size=2, num_classes=C, small_inputs=False)
    for m in f._bn_modules():                                  # statistics that do something
        m.running_mean.normal_(0, 0.1)
        m.running_var.uniform_(0.5, 1.5)
    return f.to(DEV).eval()


def _densenet121(C=8):
    import gridnext_amd as ga
    from oracle import densenet as odn
    m = ga.DenseNet(num_classes=C, **odn.DENSENET121)
    m.load_state_dict(odn.closed_form_state(odn.DenseNetCfg(num_classes=C, **odn.DENSENET121)))      # (no overflow in fp16)
    return m.to(DEV).eval()


def _nets(P):
    """The tiny net on both routes; DenseNet-121 where its maps are the ones it is run on (128 px)."""
    return (_tiny(), _densenet121()) if P == 128 else (_tiny(),)


def _pair(f, P, norm=NORM):
    """(f with the device transform on, a copy with it off): both with the same Normalize."""
    ref = copy.deepcopy(f)
    f.input_resize, f.input_crop, f.input_norm = P, P, norm
    ref.input_norm = norm
    return f, ref


@pytest.mark.parametrize("P0,P", ROUTES)
def test_eval_logits_equal_the_preprocessed_call(P0, P):
    stored, pre = _patches(8, P0, P)
    for net in _nets(P):
        for norm in (NORM, None):
            f, ref = _pair(net, P, norm)
            with torch.no_grad():
                got, want = f(stored), ref(pre)
                assert got.shape == want.shape and torch.equal(got, want) and bool(torch.isfinite(want).all())
                f.atonce = ref.atonce = 3                      # chunks of 3, 3, 2 spots
                assert torch.equal(f(stored), ref(pre))
                f.atonce = ref.atonce = None
            if net.growth_rate == 32:
                f.mfma = ref.mfma = 'f16'                      # the fp16 stem receives the bytes like any other uint8 call
                with torch.no_grad():
                    got16, want16 = f(stored), ref(pre)
                assert torch.equal(got16, want16) and bool(torch.isfinite(want16).all()) and not torch.equal(want16, want)
                f.mfma = ref.mfma = 'f32'


def test_set_input_transform_and_refusals():
    from gridnext_amd import transforms as T
    stored, pre = _patches(8, 146, 128)
    f, ref = _pair(_tiny(), 128)
    f.input_resize = f.input_crop = f.input_norm = None
    f.set_input_transform(T.Compose([T.Resize(128), T.CenterCrop(128), T.ToTensor(), T.Normalize(*NORM)]))
    assert (f.input_resize, f.input_crop, f.input_norm) == (128, 128, NORM)
    with torch.no_grad():
        assert torch.equal(f(stored), ref(pre))
        # the square check applies to the result: 130 x 146 stored patches, Resize((128, 128))
        f.input_resize, f.input_crop = (128, 128), None
        wide = torch.randint(0, 256, (2, 3, 130, 146), device=DEV, dtype=torch.uint8)
        want = ref(torch.from_numpy(R.pillow_resize_crop(wide.cpu().numpy(), (128, 128), None)).to(DEV))
        assert torch.equal(f(wide), want)
        f.input_resize = 128                                   # 130 x 146 -> 128 x 143: not square
        with pytest.raises(ValueError, match="square"):
            f(wide)
        with pytest.raises(ValueError, match="uint8"):         # the transform is defined on bytes
            f(torch.rand(2, 3, 146, 146, device=DEV))
        with pytest.raises(ValueError, match="uint8"):
            f._float_patches(torch.rand(2, 3, 146, 146, device=DEV))
        with pytest.raises(ValueError, match="larger"):
            f.input_crop = 200
            f(stored)


def _grads(f, x, weights, train):
    f.train(train)
    f.zero_grad(set_to_none=True)
    out = f(x)
    (out * weights).sum().backward()
    torch.cuda.synchronize()
    state = {k: v.clone() for k, v in f.state_dict().items()}
    f.eval()
    return out.detach(), {k: p.grad.clone() for k, p in f.named_parameters()}, state


@pytest.mark.parametrize("P0,P", ROUTES)
@pytest.mark.parametrize("train", [False, True])
def test_gradients_in_both_batchnorm_modes(P0, P, train):
    """Logits, every parameter's gradient and (train mode) the moved running statistics: the tiny net and DenseNet-121."""
    stored, pre = _patches(8, P0, P)
    for net in _nets(P):
        f, ref = _pair(net, P)
        w = torch.randn(8, net.classifier.out_features, device=DEV)
        for efficient, budget in ((False, None), (True, None), (False, 1)):      # taped; recomputed; recomputed in tape-budget chunks
            if train and budget:
                continue                                       # (batch statistics do not go in chunks)
            for m in (f, ref):
                m.efficient = efficient
                if budget:
                    m.tape_budget = budget
            o1, g1, s1 = _grads(f, stored, w, train)
            o2, g2, s2 = _grads(ref, pre, w, train)
            assert torch.equal(o1, o2)
            assert g1.keys() == g2.keys() and len(g1) > 10
            for k in g1:
                assert torch.equal(g1[k], g2[k]), k
            for k in s1:
                assert torch.equal(s1[k], s2[k]), k


def test_efficient_chunks_resize_per_chunk():
    """16 spots against a tape budget of one chunk of 8: two recomputed chunks, each resized on its own."""
    stored, pre = _patches(16, 146, 128)
    f, ref = _pair(_tiny(), 128)
    w = torch.randn(16, 4, device=DEV)
    for m in (f, ref):
        m.efficient, m.tape_budget = True, 1
    o1, g1, _ = _grads(f, stored, w, False)
    o2, g2, _ = _grads(ref, pre, w, False)
    assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)


@pytest.mark.parametrize("P0,P", ROUTES)
def test_gridnet_hex_oddr_forward_backward_with_atonce_patch_limit(P0, P):
    import gridnext_amd as ga
    H, W, C, B = 4, 3, 4, 2
    stored, pre = _patches(B * H * W, P0, P)
    f, fref = _pair(_tiny(C), P)
    torch.manual_seed(3)
    g = ga.GridNetHexOddr(f, (3, P0, P0), (H, W), C, atonce_patch_limit=7).to(DEV)        # the STORED size is the patch shape
    gref = ga.GridNetHexOddr(fref, (3, P, P), (H, W), C, atonce_patch_limit=7).to(DEV)
    gref.corrector.load_state_dict(g.corrector.state_dict())
    wts = torch.randn(B, C, H, W, device=DEV)
    outs = []
    for m, x in ((g, stored.view(B, H, W, 3, P0, P0)), (gref, pre.view(B, H, W, 3, P, P))):
        m.train()
        m.patch_classifier.eval()                              # the grid recipe: f on running statistics
        with torch.no_grad():
            ev = m(x).clone()                                  # no tape: chunks inside the eval forward
        m.zero_grad(set_to_none=True)
        out = m(x)                                             # f's parameters require grad: recomputed chunks of 7 spots
        (out * wts).sum().backward()
        torch.cuda.synchronize()
        outs.append((ev, out.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    (e1, o1, g1), (e2, o2, g2) = outs
    assert torch.equal(e1, e2) and torch.equal(o1, o2)
    assert g1.keys() == g2.keys() and any(k.startswith('patch_classifier.') for k in g1)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_skip_empty_finds_the_background_after_the_resize():
    from gridnext_amd.densenet import EMPTY_GRANULE
    n = 3 * EMPTY_GRANULE
    empty = (1, 2, 5, 7, 8, 9, 10, 13, 14, 15, 17, 20, 21, 22)
    stored, pre = _patches(n, 146, 128, empty)
    for net in (_tiny(), _densenet121()):
        f, ref = _pair(net, 128)
        with torch.no_grad():
            got, skipped = f(stored), f._skipped_empty
            want, skipped_ref = ref(pre), ref._skipped_empty
        assert skipped == skipped_ref and skipped >= EMPTY_GRANULE
        assert torch.equal(got, want)
        assert torch.equal(got[list(empty)], got[1:2].expand(len(empty), -1))


def test_f_cache_misses_after_input_crop_changes():
    import gridnext_amd as ga
    H, W, C = 4, 3, 4
    stored, pre = _patches(2 * H * W, 146, 128)
    f, fref = _pair(_tiny(C), 128)
    f.input_crop = None                                        # Resize(128) of a square patch is the whole transform
    for p in list(f.parameters()) + list(fref.parameters()):
        p.requires_grad = False
    g = ga.GridNetHexOddr(f, (3, 146, 146), (H, W), C).to(DEV).eval()
    gref = ga.GridNetHexOddr(fref, (3, 128, 128), (H, W), C).to(DEV).eval()
    x = stored.view(2, H, W, 3, 146, 146)
    with torch.no_grad():
        want = gref.patch_predictions(pre.view(2, H, W, 3, 128, 128))
        cache = g.enable_f_cache()
        assert torch.equal(g.patch_predictions(x), want) and (cache.hits, cache.misses, cache.bypassed) == (0, 2, 0)
        assert torch.equal(g.patch_predictions(x), want) and (cache.hits, cache.misses) == (2, 2)
        f.input_crop = 128                                     # another transform (here with the same result): nothing is served
        assert torch.equal(g.patch_predictions(x), want) and (cache.hits, cache.misses) == (2, 4)
        f.input_resize = (128, 128)
        assert torch.equal(g.patch_predictions(x), want) and (cache.hits, cache.misses) == (2, 6)
        assert torch.equal(g.patch_predictions(x), want) and (cache.hits, cache.misses) == (4, 6)


@pytest.mark.parametrize("P0,P", ROUTES)
def test_patch_saliency_of_resized_input(P0, P):
    from gridnext_amd.utils import patch_saliency
    stored, pre = _patches(8, P0, P)
    f, ref = _pair(_tiny(), P)
    targets = torch.arange(8, device=DEV) % 4
    got = patch_saliency(f, stored, targets)
    want = patch_saliency(ref, pre, targets)
    assert got.shape == (8, P, P) and torch.equal(got, want) and float(got.abs().sum()) > 0
    assert (f.input_resize, f.input_crop) == (P, P)            # the switches are what they were
    assert torch.equal(f._float_patches(stored), ref._float_patches(pre))
