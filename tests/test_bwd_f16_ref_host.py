"""tests/bwd_f16_ref.py proved on the CPU: its references equal float64 torch.autograd on the composed operations (with the kernels'
rounding points carried as straight-through values), its recipe keeps what it promises, every case of the grid is detectable,
the restated plans give every slab a tile, the workspace sizes are the documented ones, the grid reaches every body and every
named edge, and the sequential fp32 chain - one of the two figures behind bwd_f16_ref.G - stays within its recorded ratio."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bwd_f16_ref as R
from gridnext_amd import _lib as L

D = torch.float64
CASES = [(fam, c) for fam, cases in R.GRID.items() for c in cases]
case_id = lambda fc: fc[0] + '-' + R.ids(fc[1]) if isinstance(fc, tuple) else str(fc)


def close(got, want, rel=1e-12):
    return bool(((got - want).abs() <= rel * (1 + want.abs().max())).all())


def _ste(v, rounded):
    """`rounded` as the value, the gradient of `v`."""
    return v + (rounded - v).detach()


# --------------------------------------------------------------------------------------- the references against autograd
def test_dense_layer_references_equal_float64_autograd():
    """norm1 -> relu -> conv1 -> norm2 -> relu -> conv2 differentiated by torch.autograd in float64 against the chain wgrad3,
    dgrad3, dgrad1 (with its wgrad1).  The activated operand of conv1 is the fp16 value the kernels multiply, the tape point A
    is the stored fp16 activation and norm2's x_hat is recovered from it, exactly as the kernels see them."""
    g = torch.Generator().manual_seed(11)
    imgs, S, K, mid = 3, 5, 40, 24
    M = imgs * S * S
    x = R._signed(g, 0.5, 1.5, M, K).requires_grad_()
    bn1 = R._bn(g, K, tight=False)
    gamma1, beta1 = R._chan(g, 0.75, 1.25, K).requires_grad_(), R._chan(g, 0.125, 0.25, K).requires_grad_()
    W1 = (R._signed(g, 0.5, 0.75, mid, K) * 0.2).requires_grad_()
    W2 = R._signed(g, 0.5, 0.75, 32, mid, 3, 3).requires_grad_()
    mean2, invstd2 = R._chan(g, 0.125, 0.25, mid), R._chan(g, 0.75, 1.25, mid, True)
    gamma2, beta2 = R._chan(g, 0.75, 1.25, mid).requires_grad_(), R._chan(g, 1 / 32, 1 / 16, mid).requires_grad_()
    dY = R._signed(g, 0.5, 1.5, M, 32)
    # forward
    scale1 = gamma1 * bn1.invstd
    shift1 = beta1 - bn1.mean * scale1
    z1 = x * scale1 + shift1
    a_ref, z_ref = R.act16(x.detach(), scale1.detach(), shift1.detach())
    assert torch.equal(z1.detach().float().double(), z_ref) and bool((z_ref != 0).all())
    a1 = _ste(torch.relu(z1), a_ref)
    h = a1 @ W1.t()
    xhat = (h - mean2) * invstd2
    A = torch.relu(gamma2 * xhat + beta2).detach().half().double()                 # the tape
    assert bool((A > 0).any()) and bool((A == 0).any())
    recovered = torch.where(A > 0, (A - beta2.detach()) / gamma2.detach(), xhat.detach())
    z2 = gamma2 * _ste(xhat, recovered) + beta2
    assert bool(((z2.detach() > 0) == (A > 0)).all())
    out = F.conv2d(torch.relu(z2).view(imgs, S, S, mid).permute(0, 3, 1, 2), W2, padding=1)
    (out * dY.view(imgs, S, S, 32).permute(0, 3, 1, 2)).sum().backward()
    # the references, last kernel first
    s = 4.0
    scale2 = (gamma2 * invstd2).detach()
    o3 = R.dgrad3(dY * s, W2.detach(), A, imgs, S, scale2, gamma2.detach(), beta2.detach(), s)
    assert close(R.wgrad3(dY * s, A, imgs, S, s).ref, W2.grad)
    assert close(o3['dgamma'].ref, gamma2.grad) and close(o3['dbeta'].ref, beta2.grad)
    bn = R.NS(scale=scale1.detach(), shift=shift1.detach(), mean=bn1.mean, invstd=bn1.invstd)
    G0 = R._signed(g, 0.5, 1.5, M, K)
    o1 = R.dgrad1(o3['dB'].ref, W1.detach(), x.detach(), G0, bn, s)
    assert close(o1['G'].ref - G0, x.grad * s)
    assert close(o1['dW'].ref, W1.grad) and close(o1['dgamma'].ref, gamma1.grad) and close(o1['dbeta'].ref, beta1.grad)
    assert close(R.wgrad1(o3['dB'].ref, a_ref, s).ref, W1.grad)


def _bn_leaves(g, C):
    bn = R._bn(g, C, tight=False)
    gamma, beta = R._chan(g, 0.75, 1.25, C).requires_grad_(), R._chan(g, 0.125, 0.25, C).requires_grad_()
    scale = gamma * bn.invstd
    shift = beta - bn.mean * scale
    return gamma, beta, scale, shift, R.NS(scale=scale.detach(), shift=shift.detach(), mean=bn.mean, invstd=bn.invstd)


@pytest.mark.parametrize("imgs,S,C", [(3, 2, 8), (2, 6, 16)])
def test_transition_reference_equals_float64_autograd(imgs, S, C):
    g = torch.Generator().manual_seed(S)
    M, So = imgs * S * S, S // 2
    x = R._signed(g, 0.5, 1.5, M, C).requires_grad_()
    gamma, beta, scale, shift, bn = _bn_leaves(g, C)
    dP = R._signed(g, 0.5, 1.5, imgs * So * So, C)
    P = F.avg_pool2d(torch.relu(x * scale + shift).view(imgs, S, S, C).permute(0, 3, 1, 2), 2, 2)
    (P * dP.view(imgs, So, So, C).permute(0, 3, 1, 2)).sum().backward()
    s = 8.0
    o = R.trans(dP * s, x.detach(), imgs, S, bn, s)
    assert close(o['G'].ref, x.grad * s) and close(o['dgamma'].ref, gamma.grad) and close(o['dbeta'].ref, beta.grad)


@pytest.mark.parametrize("imgs,S2,C", [(3, 1, 8), (2, 9, 16)])
def test_tail_reference_equals_float64_autograd(imgs, S2, C):
    g = torch.Generator().manual_seed(S2)
    x = R._signed(g, 0.5, 1.5, imgs * S2, C).requires_grad_()
    gamma, beta, scale, shift, bn = _bn_leaves(g, C)
    dfeats = R._signed(g, 0.5, 1.5, imgs, C)
    (torch.relu(x * scale + shift).view(imgs, S2, C).mean(1) * dfeats).sum().backward()
    s = 16.0
    o = R.tail(dfeats, x.detach(), S2, bn, s)
    assert close(o['G'].ref, x.grad * s) and close(o['dgamma'].ref, gamma.grad) and close(o['dbeta'].ref, beta.grad)


def test_conv2_as_a_matrix_product_equals_the_transposed_convolution():
    r = R.recipe_conv2(3, 5)
    assert close(R.conv2_cols(r.dY, 3, 5) @ R.conv2_weight_matrix(r.W2), R.conv2_input_grad(r.dY, r.W2, 3, 5))


def test_h16_reference_is_the_rounded_product():
    r = R.recipe_h16(9, 16, 24)
    o = R.h16(r.X, r.W, r.pro, r.con)
    a = torch.relu((r.X * r.pro[0] + r.pro[1]).float()).half().double()
    assert torch.equal(o.ref, torch.relu(F.linear(a, r.W) * r.con[0] + r.con[1])) and bool((o.T >= o.ref.abs()).all())
    assert torch.equal(R.h16(r.X, r.W).ref, F.linear(r.X, r.W))


# ------------------------------------------------------------------------------------------------------ the recipe
def _fp16_valued(*ts):
    return all(t.dtype == D and torch.equal(t, t.half().double()) for t in ts)


def _within(t, lo, hi, zero_ok=False):
    m = t.abs()
    if zero_ok:
        m = m[m != 0]
    return m.min().item() >= lo and m.max().item() <= hi


@pytest.mark.parametrize("fc", CASES, ids=case_id)
def test_recipe_keeps_its_promises(fc):
    """fp16 values throughout, magnitudes in their ranges, both signs present, and no pre-activation nearer to 0 than 2^-6:
    the excluded share of every comparison is 0."""
    fam, c = fc
    M = R.rows_of(fam, c)
    hi = 0.625 if fam in ('wgrad3', 'dgrad3', 'conv3', 'dgrad1') else R._hi(M)
    if fam == 'wgrad1':
        r = R.recipe_wgrad1(c)
        assert _fp16_valued(r.dY, r.X, r.bn.scale, r.bn.shift, r.dW0) and _within(r.dY, 0.5, hi) and _within(r.X, 0.5, hi)
        assert R.min_fma(r.X, r.bn) >= 2 ** -6
        bns = [r.bn]
    elif fam in ('wgrad3', 'dgrad3', 'conv3'):
        r = R.recipe_conv2(c.imgs, c.S)
        assert _fp16_valued(r.dY, r.A, r.W2, r.scale2, r.gamma2, r.beta2, r.dW0, r.dg0, r.db0)
        assert _within(r.dY, 0.5, hi) and _within(r.A, 0.5, hi, zero_ok=True) and bool((r.A >= 0).all()) and _within(r.W2, 0.5, 0.75)
        assert _within(r.gamma2, 0.75, 1.25) and _within(r.scale2, 0.75, 1.25) and _within(r.beta2, 1 / 32, 1 / 16)
        assert bool((r.gamma2 < 0).any()) and bool((r.gamma2 > 0).any())                       # negative gamma channels
        # every 64-row tile keeps live elements, every channel has some
        tiles = r.A.split(64)
        assert all(bool((t > 0).any()) for t in tiles) and bool((r.A > 0).any(0).all())
        bns = []
    elif fam == 'dgrad1':
        r = R.recipe_dgrad1(c.M, c.K)
        assert _fp16_valued(r.dB, r.W1, r.X, r.G0, r.dW0, r.dg0, r.db0) and _within(r.dB, 0.5, hi) and _within(r.W1, 0.5, 0.75)
        assert _within(r.X, 0.5, hi) and _within(r.G0, 0.5, 1.5)
        z = R.act16(r.X, r.bn.scale, r.bn.shift)[1]
        assert all(bool((t > 0).any()) for t in z.split(64)) and (c.M < 64 or bool((z > 0).any(0).all()))
        bns = [r.bn]
    elif fam in ('tail', 'trans'):
        r = R.recipe_tail(c.imgs, c.C, c.S2) if fam == 'tail' else R.recipe_trans(c.imgs, c.C, c.S)
        g = r.dfeats if fam == 'tail' else r.dP
        assert _fp16_valued(g, r.X, r.dg0, r.db0) and _within(g, 0.5, hi) and _within(r.X, 0.5, hi)
        bns = [r.bn]
    elif fam == 'h16':
        r = R.recipe_h16(c.M, c.N, c.K)
        assert _fp16_valued(r.X, r.W, *r.pro, *r.con) and _within(r.X, 0.5, 1.5) and _within(r.W, 0.5, 0.75)
        assert R.act16(r.X, *r.pro)[1].abs().min().item() >= 2 ** -6
        bns = []
    else:
        return
    for bn in bns:
        assert _fp16_valued(bn.scale, bn.shift, bn.mean, bn.invstd) and _within(bn.scale, 0.75, 1.25) and _within(bn.shift, 1 / 32, 0.25)
        assert bool((bn.invstd > 0).all()) and (bn.scale.numel() < 16 or (bool((bn.scale < 0).any()) and bool((bn.scale > 0).any())))
        assert R.min_fma(r.X, bn) >= 2 ** -6, R.min_fma(r.X, bn)


# ------------------------------------------------------------------------------------------------- detectability
def _outputs(fam, c, s=1.0):
    """Every (name, output) a GPU case compares, without and with a prior."""
    if fam == 'wgrad1':
        r = R.recipe_wgrad1(c)
        outs = [('dW pro %d' % p, R.reference_wgrad1(c, p, s)['dW'], r.dW0) for p in (0, 1)]
    elif fam in ('wgrad3', 'dgrad3', 'conv3'):
        r = R.recipe_conv2(c.imgs, c.S)
        o = R.reference_conv2(c.imgs, c.S, s)
        names = dict(wgrad3=['dW'], dgrad3=['dB', 'dgamma', 'dbeta'], conv3=['dW', 'dB', 'dgamma', 'dbeta'])[fam]
        outs = [(n, o[n], dict(dW=r.dW0, dgamma=r.dg0, dbeta=r.db0).get(n)) for n in names]
        if R.thinned(fam, c):                                   # the second run: a dense mask, no BatchNorm sums
            o = R.reference_conv2(c.imgs, c.S, s, dense=True)
            outs += [(n + ' dense', o[n], dict(dW=r.dW0).get(n)) for n in names if n in ('dW', 'dB')]
    elif fam == 'dgrad1':
        r = R.recipe_dgrad1(c.M, c.K)
        o = R.reference_dgrad1(c.M, c.K, s)
        outs = [(n, o[n], dict(dW=r.dW0, dgamma=r.dg0, dbeta=r.db0).get(n)) for n in ('G', 'dW', 'dgamma', 'dbeta')]
        if R.thinned(fam, c):
            o = R.reference_dgrad1(c.M, c.K, s, dense=True)
            outs += [(n + ' dense', o[n], dict(dW=r.dW0).get(n)) for n in ('G', 'dW')]
    elif fam in ('tail', 'trans'):
        r = R.recipe_tail(c.imgs, c.C, c.S2) if fam == 'tail' else R.recipe_trans(c.imgs, c.C, c.S)
        o = R.reference_tail(c.imgs, c.C, c.S2, s) if fam == 'tail' else R.reference_trans(c.imgs, c.C, c.S, s)
        outs = [(n, o[n], dict(dgamma=r.dg0, dbeta=r.db0).get(n)) for n in ('G', 'dgamma', 'dbeta')]
    elif fam == 'h16':
        outs = [('out act %d' % a, R.reference_h16(c.M, c.N, c.K, a)['out'], None) for a in (0, 1)]
    else:
        outs = []
    return outs


@pytest.mark.parametrize("fc", CASES, ids=case_id)
def test_grid_cases_are_detectable(fc):
    fam, c = fc
    for name, o, prior in _outputs(fam, c):
        assert bool(torch.isfinite(o.ref).all()) and o.term > 0, (fam, c, name)
        assert R.detectable(o), (fam, c, name, o.term, 4 * R.tol(o).max().item())
        if prior is not None:
            p = R.with_prior(o, prior)
            assert R.detectable(p), (fam, c, name, 'accumulate', p.term, 4 * R.tol(p).max().item())


def test_thinned_cases_are_the_long_ones_and_their_dense_recipe_is_half_live():
    thin = [(fam, c) for fam, c in CASES if R.thinned(fam, c)]
    assert {fam for fam, _ in thin} == {'wgrad3', 'dgrad3', 'conv3', 'dgrad1'}
    assert all(R.rows_of(fam, c) * (128 if fam == 'dgrad1' else 288) > 2 * R.TERMS for fam, c in thin)
    r = R.recipe_conv2(4104, 4, dense=True)
    assert 0.49 < (r.A > 0).double().mean().item() < 0.51 and torch.equal(r.dY, R.recipe_conv2(4104, 4).dY)
    r = R.recipe_dgrad1(64 * 600 + 7, 32, dense=True)
    assert 0.49 < (R.act16(r.X, r.bn.scale, r.bn.shift)[1] > 0).double().mean().item() < 0.51 and R.min_fma(r.X, r.bn) >= 2 ** -6


def test_a_loss_scale_moves_term_and_tolerance_together():
    c = R.WG1_GRID[4]
    a, b = R.reference_wgrad1(c, 1, 1.0)['dW'], R.reference_wgrad1(c, 1, 4096.0)['dW']
    assert torch.equal(a.ref, b.ref * 4096) and torch.equal(R.tol(a), R.tol(b) * 4096) and a.term == b.term * 4096


# ------------------------------------------------------------------------------------------------- the dispatch
def test_plan_slabs_is_the_source_s():
    assert [vars(R.plan_slabs(M, 64, 768)) for M in (1, 64, 65)] == [dict(tiles=1, slabs=1, per=1), dict(tiles=1, slabs=1, per=1),
                                                                      dict(tiles=2, slabs=2, per=1)]
    assert vars(R.plan_slabs(64 * 770 + 5, 64, 768)) == dict(tiles=771, slabs=386, per=2)
    assert [R.slabs_for(768, b) for b in (1, 2, 3, 4, 5, 6, 7, 8, 32, 200)] == [768, 384, 256, 192, 152, 128, 104, 96, 24, 8]
    assert [R.slabs_for(512, b) for b in (1, 2, 3, 8)] == [512, 256, 168, 64]
    assert vars(R.plan_wgrad1(1600, 512, 1024)) == dict(tiles=25, slabs=13, per=2)
    assert vars(R.plan_wgrad1(64 * 257 + 1, 8, 264)) == dict(tiles=258, slabs=129, per=2)
    assert vars(R.plan_wgrad1(513, 8, 136)) == dict(tiles=9, slabs=9, per=1)
    assert (R.plan_dgrad1(64 * 600 + 7, 32, False).slabs, R.plan_dgrad1(64 * 600 + 7, 32, True).slabs) == (601, 301)
    assert [R.conv3_bwd_grid(128 * t) for t in (1, 255, 256, 257, 1000)] == [1, 255, 256, 256, 256]
    assert [(p.slabs, p.per) for p in (R.plan_of('conv3', R.C3('', 8 * t, 4, '')) for t in (1, 256, 257, 511, 513))] == [
        (1, 1), (256, 1), (129, 2), (256, 2), (171, 3)]
    assert [R.tail_slots(n, 1024) for n in (1, 1024, 1025, 2051)] == [1, 1024, 1024, 1024] and R.tail_slots(10 ** 6, 8) == 131072
    assert [R.trans_slots(n, 1024) for n in (4096, 4097)] == [4096, 4096] and R.trans_slots(10 ** 7, 8) == 524288
    assert R.cols_blocks(16400, 512) == 4096 and R.cols_blocks(16400, 512) < 16400 * 64 / 256 and R.cols_blocks(77, 8) == 1


@pytest.mark.parametrize("fc", [fc for fc in CASES if fc[0] in ('wgrad1', 'wgrad3', 'dgrad3', 'conv3', 'dgrad1')], ids=case_id)
def test_every_planned_slab_owns_a_tile(fc):
    fam, c = fc
    for wg in ((False, True) if fam == 'dgrad1' else (False,)):
        p = R.plan_of(fam, c, wg)
        assert p.slabs >= 1 and p.per >= 1 and (p.slabs - 1) * p.per < p.tiles <= p.slabs * p.per, (fam, c, vars(p))


@pytest.mark.parametrize("fc", [fc for fc in CASES if fc[0] in ('tail', 'trans')], ids=case_id)
def test_every_slot_owns_an_image_or_a_pixel(fc):
    fam, c = fc
    n = c.imgs if fam == 'tail' else c.imgs * (c.S // 2) ** 2
    slots = R.tail_slots(n, c.C) if fam == 'tail' else R.trans_slots(n, c.C)
    assert 1 <= slots <= n


def test_workspace_sizes_are_the_documented_formulas():
    for c in R.WG1_GRID:
        assert R.ws_wgrad1(c.M, c.N, c.K) == R.plan_of('wgrad1', c).slabs * c.N * c.K
    for c in R.WG3_GRID:
        assert R.ws_wgrad3(R.rows_of('wgrad3', c)) == R.plan_of('wgrad3', c).slabs * 9 * 32 * 128
    for c in R.DG3_GRID:
        assert R.ws_dgrad3(R.rows_of('dgrad3', c)) == R.plan_of('dgrad3', c).slabs * 256
    for c in R.C3_GRID:
        M = R.rows_of('conv3', c)
        assert R.ws_conv3(M) == min(256, M // 128) * (256 + 36864)
    for c in R.DG1_GRID:
        cw = (c.K + 127) // 128 * 128
        assert R.ws_dgrad1(c.M, c.K, False) == R.plan_of('dgrad1', c, False).slabs * 2 * cw
        assert R.ws_dgrad1(c.M, c.K, True) == R.plan_of('dgrad1', c, True).slabs * 130 * cw
    for c in R.TAIL_GRID:
        assert R.ws_tail(c.imgs, c.C) == min(c.imgs, 131072 * 8 // c.C) * 2 * c.C
    for c in R.TRANS_GRID:
        assert R.ws_trans(c.imgs, c.C, c.S) == min(c.imgs * (c.S // 2) ** 2, 524288 * 8 // c.C) * 2 * c.C


def _fake_args(**kw):
    """Arguments with every pointer present and 16-B aligned."""
    return R.NS(**kw)


def test_grid_covers_every_body_and_every_edge_by_name():
    for fam, cases in R.GRID.items():
        assert {c.edge for c in cases} == R.EDGES[fam], fam
    P = 4096
    bodies = set()
    for c in R.WG1_GRID:
        for sc in (None, P):
            bodies.add(R.form_wgrad1(_fake_args(dY16=P, lddy=c.N, X16=P, ldx=c.K, scale=sc, shift=sc, dW=P, workspace=P, M=c.M, N=c.N,
                                                K=c.K, ls=P)).body)
    for fam, form in (('wgrad3', R.form_wgrad3), ('dgrad3', R.form_dgrad3), ('conv3', R.form_conv3)):
        by = {}
        for c in R.GRID[fam]:
            f = form(_fake_args(dY16=P, lddy=32, W2b16=P, A16=P, lda=128, bsa=32, dB16=P, dW=P, workspace=P, M=R.rows_of(fam, c), S=c.S,
                                scale2=P, gamma2=P, beta2=P, ls=P))
            by.setdefault(f.body, []).append(c)
        bodies |= set(by)
        if fam != 'conv3':
            pad, gen = by[{'wgrad3': 'WG3_PAD', 'dgrad3': 'DG3_PAD'}[fam]], by[{'wgrad3': 'WG3', 'dgrad3': 'DG3'}[fam]]
            assert {c.S for c in pad} == set(R.POW2_MAPS) and {c.edge for c in pad} >= {'padded'}
            assert {c.S for c in gen} >= {1, 2, 3, 7, 63} and any(c.S in R.POW2_MAPS for c in gen)
            assert any(R.plan_of(fam, c).per == 2 for c in pad) and (fam == 'dgrad3' or any(R.plan_of(fam, c).per == 2 for c in gen))
        else:
            assert {c.S for c in by['C3']} == set(R.POW2_MAPS)
    for c in R.DG1_GRID:
        for dW in (None, P):
            bodies.add(R.form_dgrad1(_fake_args(dB16=P, W1t16=P, X16=P, ldx=c.K, bsx=32, G16=P, ldg=c.K, bsg=32, M=c.M, K=c.K, scale=P,
                                                shift=P, mean=P, invstd=P, dW=dW, workspace=P, ls=P)).body)
    bodies |= {'TAIL', 'TRANS'}
    assert bodies == set(R.BODIES)
    assert {R.form_h16(_fake_args(A16=P, lda16=c.K, W16=P, out16=P, ldc16=c.N, rows_total=c.M, M=c.M, N=c.N, K=c.K, scale=None, shift=None,
                                  out_scale=None, out_shift=None), c.cb).body for c in R.H16_GRID} == set(R.H16_BODIES)
    # edges that are arithmetic claims
    assert any(R.plan_of('wgrad1', c).slabs % 8 and (c.K > 128 or c.N > 128) for c in R.WG1_GRID)
    short = R.plan_of('wgrad1', R.Wg1('', 64 * 770 + 5, 8, 8))
    assert short.per == 2 and short.tiles % 2 == 1
    assert any(-(-c.K // 128) * -(-c.N // 128) == 32 and R.plan_of('wgrad1', c).slabs == 13 for c in R.WG1_GRID)
    assert {-(-c.K // 128) for c in R.DG1_GRID} >= {1, 2, 3, 8}
    assert any(R.plan_of('dgrad1', c, False).slabs % 8 and c.K > 128 for c in R.DG1_GRID)
    assert any(R.tail_slots(c.imgs, c.C) < c.imgs for c in R.TAIL_GRID) and {c.imgs for c in R.TAIL_GRID if c.lay == 'blocked'} >= {1, 15, 16, 17}
    assert any(R.trans_slots(c.imgs * (c.S // 2) ** 2, c.C) < c.imgs * (c.S // 2) ** 2 for c in R.TRANS_GRID)
    assert {c.S for c in R.TRANS_GRID} >= {2, 4, 6, 14} and {c.S2 for c in R.TAIL_GRID} >= {1, 4, 16, 49}
    assert any(R.cols_blocks(c.M, c.C) * 256 < c.M * c.C // 8 for c in R.COLS_GRID)
    assert {c.M for c in R.H16_GRID} >= {131071, 131072, 131072 + 129} and {c.K for c in R.H16_GRID} >= {8, 40, 64, 72}
    assert {c.N for c in R.H16_GRID if not c.cb} >= {8, 32, 136} and {c.N for c in R.H16_GRID if c.cb} >= {32, 64}


def test_refusals_are_restated():
    P = 4096
    a = dict(dY16=P, lddy=8, X16=P, ldx=8, scale=None, shift=None, dW=P, workspace=P, M=5, N=8, K=8, ls=P)
    for kw, code in ((dict(lddy=7), R.ERR_BAD_ARG), (dict(scale=P), R.ERR_BAD_ARG), (dict(M=0), R.ERR_BAD_ARG), (dict(ls=None), R.ERR_BAD_ARG),
                     (dict(N=4, lddy=8), R.ERR_UNSUPPORTED), (dict(ldx=12), R.ERR_UNSUPPORTED), (dict(X16=P + 8), R.ERR_UNSUPPORTED)):
        f = R.form_wgrad1(R.NS(**dict(a, **kw)))
        assert (f.code, f.workgroups, f.slabs, f.per) == (code, 0, 0, 0), kw
    b = dict(dY16=P, lddy=32, W2b16=P, A16=P, lda=128, bsa=32, dB16=P, dW=P, workspace=P, M=4225, S=65, scale2=P, gamma2=P, beta2=P, ls=P)
    assert R.form_wgrad3(R.NS(**b)).code == R.form_dgrad3(R.NS(**b)).code == R.ERR_UNSUPPORTED
    assert R.form_wgrad3(R.NS(**dict(b, M=4224))).code == R.ERR_BAD_ARG
    assert R.form_conv3(R.NS(**dict(b, M=49 * 128, S=7))).code == R.ERR_UNSUPPORTED
    assert R.form_conv3(R.NS(**dict(b, M=64, S=4))).code == R.ERR_UNSUPPORTED and R.form_conv3(R.NS(**dict(b, M=128, S=4))).code == R.CODES['C3']


# ------------------------------------------------------------------------ the library's own answers (nothing is launched)
FAKE = 1 << 20                                # a 16-B aligned address: the queries read no operand


def _fake_call(fam, c, **kw):
    """(form query, out values, restated form, arguments by the header's names) of a case on row-major operands."""
    M = R.rows_of(fam, c)
    bn = dict(scale=FAKE, shift=FAKE, mean=FAKE, invstd=FAKE, dgamma=FAKE, dbeta=FAKE, workspace=FAKE, ls=FAKE, accumulate=0, flag=FAKE)
    if fam == 'wgrad1':
        p = dict(bn, dY16=FAKE, lddy=c.N, X16=FAKE, ldx=c.K, dW=FAKE, M=M, N=c.N, K=c.K)
        q = ('gnx_wgrad1x1_f16_form', 3, R.form_wgrad1)
    elif fam in ('wgrad3', 'dgrad3', 'conv3'):
        p = dict(bn, dY16=FAKE, lddy=32, W2b16=FAKE, A16=FAKE, lda=128, bsa=32, dB16=FAKE, dW=FAKE, M=M, S=c.S, scale2=FAKE, gamma2=FAKE,
                 beta2=FAKE)
        q = dict(wgrad3=('gnx_wgrad3x3_f16_form', 3, R.form_wgrad3), dgrad3=('gnx_conv3x3_dgrad_bnrelu_bwd_f16_form', 3, R.form_dgrad3),
                 conv3=('gnx_conv3x3_bwd_f16_form', 2, R.form_conv3))[fam]
    elif fam == 'dgrad1':
        p = dict(bn, dB16=FAKE, W1t16=FAKE, X16=FAKE, ldx=c.K, bsx=32, G16=FAKE, ldg=c.K, bsg=32, M=M, K=c.K, dW=FAKE)
        q = ('gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_form', 3, R.form_dgrad1)
    elif fam == 'tail':
        p = dict(bn, dfeats=FAKE, ldf=c.C, X16=FAKE, ldx=c.C, bsx=32, G16=FAKE, ldg=c.C, bsg=32, imgs=c.imgs, C=c.C, S2=c.S2)
        q = ('gnx_tail_bwd_f16_form', 3, R.form_tail)
    elif fam == 'trans':
        p = dict(bn, dP16=FAKE, ldp=c.C, bsp=32, X16=FAKE, ldx=c.C, bsx=32, G16=FAKE, ldg=c.C, bsg=32, imgs=c.imgs, C=c.C, S=c.S)
        q = ('gnx_trans_bwd_f16_form', 3, R.form_trans)
    else:
        p = dict(A16=FAKE, lda16=c.K, W16=FAKE, out16=FAKE, ldc16=c.N, rows_total=c.M, M=c.M, N=c.N, K=c.K, scale=None, shift=None,
                 out_scale=None, out_shift=None)
        q = ('gnx_conv1x1_bnrelu_h16_cb_form' if c.cb else 'gnx_conv1x1_bnrelu_h16_form', 1, lambda a: R.form_h16(a, c.cb))
    p.update(kw)
    form, nout, restate = q
    outs = [ctypes.c_int(-7) for _ in range(nout)]
    names = L.PARAMS[form]
    rc = L.query(form, *[p[k] for k in names[:len(names) - nout]], *[ctypes.addressof(o) for o in outs])
    f = restate(R.NS(**p))
    want = {1: lambda: (f.code, f.workgroups), 2: lambda: (f.code, f.workgroups, f.per),
            3: lambda: (f.code, f.slots, f.workgroups, f.blocked) if 'slots' in names else (f.code, f.workgroups, f.slabs, f.per)}[nout]()
    return (rc,) + tuple(o.value for o in outs), want, form, p


@pytest.mark.parametrize("fc", [fc for fc in CASES if fc[0] != 'cols'], ids=case_id)
def test_form_queries_agree_with_the_restated_dispatch(fc):
    """gnx_*_form on every case of the grid (and on what turns a case into a refusal) against bwd_f16_ref.form_*: the queries
    launch nothing and read no operand, so they run here.  NULL out-pointers are accepted."""
    fam, c = fc
    variants = [dict()]
    if fam == 'wgrad1':
        variants += [dict(scale=None, shift=None), dict(shift=None), dict(N=c.N + 4), dict(lddy=c.N - 1), dict(X16=FAKE + 8), dict(M=0)]
    elif fam in ('wgrad3', 'dgrad3', 'conv3'):
        variants += [dict(lda=32, bsa=64 * 1024), dict(S=65, M=4225), dict(S=7, M=49 * 128), dict(M=c.imgs * c.S * c.S + 1), dict(bsa=36),
                     dict(A16=None), dict(dY16=FAKE + 8)]
    elif fam == 'dgrad1':
        variants += [dict(dW=None), dict(ldx=32, bsx=4096 * 32, ldg=32, bsg=4100 * 32), dict(K=c.K + 8, ldx=1024, ldg=1024), dict(ldx=c.K + 4),
                     dict(bsg=36), dict(G16=FAKE + 8), dict(invstd=None), dict(ldx=c.K - 8)]
    elif fam in ('tail', 'trans'):
        variants += [dict(ldx=32, bsx=1 << 20), dict(ldg=32, bsg=1 << 20), dict(C=c.C + 4), dict(ldx=c.C - 8), dict(X16=FAKE + 8), dict(imgs=0)]
        variants += [dict(S2=0)] if fam == 'tail' else [dict(S=c.S + 1), dict(S=0)]
    else:
        variants += [dict(scale=FAKE, shift=FAKE, out_scale=FAKE, out_shift=FAKE), dict(M=0), dict(M=131071), dict(M=131072), dict(scale=FAKE),
                     dict(K=c.K + 4, lda16=1024), dict(lda16=c.K - 8), dict(W16=FAKE + 8)]
    for kw in variants:
        said, want, form, p = _fake_call(fam, c, **kw)
        assert said == want, (form, kw, said, want)
        assert said[0] >= 0 or set(said[1:]) == {0}, (form, kw, said)
        names = L.PARAMS[form]
        nout = len(said) - 1
        assert L.query(form, *[p[k] for k in names[:len(names) - nout]], *([None] * nout)) == said[0], (form, kw)


# --------------------------------------------------------------------------------------------------- where G comes from
def test_G_is_what_the_measured_ratios_make_it():
    assert R.G == max(8.0, 4 * R.TORCH_FP32_RATIO, 4 * R.CHAIN_FP32_RATIO)


@pytest.mark.parametrize("fc", [fc for fc in CASES if fc[0] != 'cols'], ids=case_id)
def test_sequential_fp32_chain_stays_within_the_ratio_G_was_set_from(fc, capsys):
    """One of the two figures behind bwd_f16_ref.G, kept runnable: every contraction of the case as a sequential fp32
    multiply-add chain against float64, |err| / (2^-24 T), on evenly spread outputs."""
    fam, c = fc
    ratio, name = R.plain_ratio(fam, c, R.chain_fp32, nrows=16, ncols=16)
    with capsys.disabled():
        print(' fp32 chain ratio at %s: %.4f (%s)' % (case_id(fc), ratio, name))
    assert ratio <= R.CHAIN_FP32_RATIO, (ratio, name)
