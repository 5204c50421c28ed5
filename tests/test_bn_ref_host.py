"""tests/bn_ref.py proved before test_gpu_bn_forms.py uses it as the reference: against a float64 nn.BatchNorm1d under autograd,
its forms against each other, and - for every input recipe of the GPU file - the detectability condition (the smallest
single-row term of each reduced quantity is at least four tolerances).  Runs on the CPU."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_ref as R


def rel_close(a, b, what, rel=1e-12):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    tol = rel * max(b.abs().max().item(), 1.0)
    err = (a - b).abs().max().item()
    assert err <= tol, "%s: %.3e > %.3e" % (what, err, tol)


def _torch_bn(rec, affine, momentum, eps, training, relu):
    bn = nn.BatchNorm1d(rec.C, eps=eps, momentum=momentum, affine=affine).double()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(rec.gamma.double())
            bn.bias.copy_(rec.beta.double())
        bn.running_mean.copy_(rec.running_mean.double())
        bn.running_var.copy_(rec.running_var.double())
    bn.train(training)
    x = rec.x.double().requires_grad_(True)
    y = bn(x)
    if relu:
        y = torch.relu(y)
    y.backward(rec.dy.double())
    return bn, x, y


@pytest.mark.parametrize("M,C", [(2, 4), (7, 3), (257, 12), (1000, 5)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("affine,momentum,eps", [(True, 0.1, 1e-5), (True, 0.3, 1e-3), (False, 0.3, 1e-5)])
def test_ref_equals_float64_batchnorm1d(M, C, training, relu, affine, momentum, eps):
    rec = R.recipe(M, C, seed=3)
    assert (rec.gamma < 0).any() or C < 8                     # negative gammas are part of every wide enough recipe
    bn, x, y = _torch_bn(rec, affine, momentum, eps, training, relu)
    gamma, beta = (rec.gamma, rec.beta) if affine else (None, None)
    if training:
        s = R.stats(rec.x, gamma, beta, rec.running_mean, rec.running_var, momentum, eps)
        rel_close(s.running_mean, bn.running_mean, 'running_mean')
        rel_close(s.running_var, bn.running_var, 'running_var')
        rel_close(s.mean, rec.x.double().mean(0), 'mean')
        rel_close(s.invstd, 1 / torch.sqrt(rec.x.double().var(0, unbiased=False) + eps), 'invstd')
    else:
        s = R.fold_eval(gamma, beta, rec.running_mean, rec.running_var, eps)
        rel_close(s.mean, rec.running_mean, 'mean')
    rel_close(R.apply(rec.x, s.scale, s.shift, relu).y, y.detach(), 'y')
    b = R.bwd(rec.dy, rec.x, s.scale, s.shift, s.mean, s.invstd, relu, training)
    rel_close(b.dx, x.grad, 'dx')
    if affine:
        rel_close(b.dgamma, bn.weight.grad, 'dgamma')
        rel_close(b.dbeta, bn.bias.grad, 'dbeta')
    else:                                                      # gamma = 1: d/dgamma of the same map, by hand
        xhat = (rec.x.double() - s.mean) * s.invstd
        dz = rec.dy.double() * ((xhat > 0) if relu else 1)     # gamma 1, beta 0: the map is relu(xhat)
        rel_close(b.dgamma, (dz * xhat).sum(0), 'dgamma')
        rel_close(b.dbeta, dz.sum(0), 'dbeta')
    # the magnitudes are what they say
    rel_close(b.s1_abs, (rec.dy.double().abs() * b.mask).sum(0), 's1_abs')
    assert (b.s2_abs >= b.s2.abs() - 1e-9).all() and (b.s1_abs >= b.s1.abs() - 1e-9).all()
    live = torch.isfinite(b.s1_min)
    assert (b.s1_min[live] >= 0.5 - 1e-6).all() and (b.s1_min[live] * b.mask.sum(0)[live] <= b.s1_abs[live] + 1e-9).all()


@pytest.mark.parametrize("M,C", [(5, 4), (257, 12)])
def test_activated_input_form_equals_relu1(M, C):
    rec = R.recipe(M, C, seed=5)
    o = R.bwd_operands(rec, 2, 0, 1e-5)
    a64 = R.apply(o.x, o.scale, o.shift, 1).y                  # unrounded: the identity is exact up to float64 round-off
    b1 = R.bwd(rec.dy, o.x, o.scale, o.shift, o.mean, o.invstd, 1, 0)
    b2 = R.bwd(rec.dy, a64, o.scale, o.shift, o.mean, o.invstd, 2, 0)
    for k in ('dx', 'dgamma', 'dbeta'):
        rel_close(getattr(b2, k), getattr(b1, k), k)
    assert torch.equal(b1.mask, b2.mask)
    assert ((b2.s2_extra > 0) == b2.mask.any(0)).all() and (b1.s2_extra == 0).all()   # (a large -beta can mask a whole channel)
    assert (o.scale < 0).any()                                  # the form divides by scale: both signs


@pytest.mark.parametrize("S", [4, 5, 7])
@pytest.mark.parametrize("imgs", [1, 3])
def test_pooled_forms_equal_avg_pool2d(S, imgs):
    C = 12
    rec = R.recipe(imgs * S * S, C, seed=S)
    o = R.bwd_operands(rec, 1, 0, 1e-5)
    So = S // 2
    dYp = R.recipe(imgs * So * So, C, seed=S + 50).dy
    # forward: relu(bn(x)) as an NCHW map through F.avg_pool2d (floor mode)
    act = R.apply(o.x, o.scale, o.shift, 1).y.view(imgs, S, S, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    pooled = F.avg_pool2d(act, 2)
    rel_close(R.bnrelu_avgpool2(o.x, o.scale, o.shift, S).out, pooled.detach().permute(0, 2, 3, 1).reshape(-1, C), 'pooled')
    pooled.backward(dYp.double().view(imgs, So, So, C).permute(0, 3, 1, 2))
    dAct = act.grad.permute(0, 2, 3, 1).reshape(-1, C)
    want = R.bwd(dAct, o.x, o.scale, o.shift, o.mean, o.invstd, 1, 0)
    got = R.pooled_bwd(dYp, o.x, o.scale, o.shift, o.mean, o.invstd, S)
    for k in ('dx', 'dgamma', 'dbeta'):
        rel_close(getattr(got, k), getattr(want, k), k)
    if S % 2:                                                   # the last row and column of an odd map get no gradient
        assert (got.dx.view(imgs, S, S, C)[:, S - 1] == 0).all() and (got.dx.view(imgs, S, S, C)[:, :, S - 1] == 0).all()
        assert not got.mask.view(imgs, S, S, C)[:, S - 1].any()


def test_accumulate_forms_are_old_plus_new():
    rec = R.recipe(300, 12, seed=9)
    for relu, training in ((0, 1), (1, 1), (1, 0)):
        o = R.bwd_operands(rec, relu, training, 1e-5)
        args = (rec.dy, o.x, o.scale, o.shift, o.mean, o.invstd, relu, training)
        new = R.bwd(*args)
        acc = R.bwd(*args, dx_old=rec.dx_old, dgamma_old=rec.dgamma_old, dbeta_old=rec.dbeta_old)
        rel_close(acc.dx, rec.dx_old.double() + new.dx, 'dx')
        rel_close(acc.dgamma, rec.dgamma_old.double() + new.dgamma, 'dgamma')
        rel_close(acc.dbeta, rec.dbeta_old.double() + new.dbeta, 'dbeta')
        assert (acc.dx_mag >= new.dx_mag).all()
    c = R.colsum(rec.x, rec.dbeta_old)
    rel_close(c.out, rec.dbeta_old.double() + rec.x.double().sum(0), 'colsum')


# ---------------------------------------------------------------------------------------- detectability of every GPU recipe
def _assert_detectable(what, r_min, tol):
    assert R.detectable(r_min, tol), "%s: smallest term %.3e < 4 x tolerance %.3e" % (
        what, r_min.min().item(), tol[r_min.argmin()].item())


@pytest.mark.parametrize("M,C", sorted(set(R.GRID) | {R.DX_VEC4_LOOP}))
def test_grid_recipes_are_detectable(M, C):
    K = R.K
    rec = R.recipe(M, C)
    for i in (0, 1):
        momentum, eps = R.mom_eps(i)
        s = R.stats(rec.x, rec.gamma, rec.beta, rec.running_mean, rec.running_var, momentum, eps)
        t = R.stats_tol(s, K)
        _assert_detectable('sum', s.sum_min, t.sum)
        _assert_detectable('m2', s.m2_min, t.m2)
        for relu in (0, 1):
            for training in (0, 1):
                o = R.bwd_operands(rec, relu, training, eps)
                b = R.bwd(rec.dy, o.x, o.scale, o.shift, o.mean, o.invstd, relu, training)
                tb = R.bwd_tol(b, K)
                _assert_detectable('s1 relu %d training %d' % (relu, training), b.s1_min, tb.s1)
                _assert_detectable('s2 relu %d training %d' % (relu, training), b.s2_min, tb.s2)
    c = R.colsum(rec.x)
    _assert_detectable('colsum', c.sum_min, R.colsum_tol(c, K))


@pytest.mark.parametrize("M,C", sorted({(M, C) for M, C, _ in R.COLSUM_CASES}))
def test_colsum_recipes_are_detectable(M, C):
    c = R.colsum(R.recipe(M, C).x)
    _assert_detectable('colsum', c.sum_min, R.colsum_tol(c, R.K))


@pytest.mark.parametrize("M,C", R.ACT_GRID)
def test_activated_recipes_are_detectable(M, C):
    rec = R.recipe(M, C)
    o = R.bwd_operands(rec, 2, 0, R.mom_eps(0)[1])
    b = R.bwd(rec.dy, o.a, o.scale, o.shift, o.mean, o.invstd, 2, 0)
    tb = R.bwd_tol(b, R.K)
    _assert_detectable('s1', b.s1_min, tb.s1)
    _assert_detectable('s2', b.s2_min, tb.s2)


@pytest.mark.parametrize("S,imgs,C", R.POOL_GRID)
def test_pooled_recipes_are_detectable(S, imgs, C):
    rec = R.recipe(imgs * S * S, C)
    o = R.bwd_operands(rec, 1, 0, 1e-5)
    dYp = R.recipe(imgs * (S // 2) ** 2, C, seed=1).dy
    b = R.pooled_bwd(dYp, o.x, o.scale, o.shift, o.mean, o.invstd, S)
    tb = R.bwd_tol(b, R.K)
    _assert_detectable('s1', b.s1_min, tb.s1)
    _assert_detectable('s2', b.s2_min, tb.s2)


# ------------------------------------------------------------------------------- the dispatch restatement and what GRID covers
def _forward_forms(M, C):
    """bn_ref.form of every forward call test_gpu_bn_forms.py makes on a shape: statistics alone, with y in x's layout, and y off
    16 B beside an x of any layout."""
    for lay in R.LAYOUTS:
        for ylay in (None, lay, 'misaligned'):
            yield R.form_of(M, C, lay, ylay)


def _backward_forms(M, C):
    for lay in R.BWD_LAYOUTS:
        if lay == 'dx_misaligned' and C % 4:
            continue
        xlay, dxlay = R.bwd_layouts(lay)
        for relu, training, _, _, dx_null, _, _ in R.BWD_COMBOS:
            yield R.bwd_form_of(M, C, xlay, None if dx_null else dxlay, relu, training)


def test_each_grid_group_lands_in_the_form_it_is_there_for():
    assert len(set(R.GRID)) == len(R.GRID) == len(R.GRID_FORM)
    for (M, C), body in R.GRID_FORM.items():
        lay = 'window' if C % 4 == 0 else 'misaligned'
        assert R.form_of(M, C, lay).body == body, (M, C)
        # with 16-B operands the training backward takes the same rows form; the eval one fuses where the forward takes slabs
        if C % 4 == 0:
            assert R.bwd_form_of(M, C, lay, lay, 1, 1).body == body
            assert R.bwd_form_of(M, C, lay, lay, 1, 0).body == ('eval_fused' if body == 'slab_vec' else body)
        else:
            assert {R.bwd_form_of(M, C, lay, lay, 1, t).body for t in (0, 1)} == {'slab'}
    for M, C in R.ACT_GRID:
        assert {R.bwd_form_of(M, C, 'window', dx, 2, 0).body for dx in (None, 'window')} == {R.ACT_FORM}
        assert R.bwd_form_of(M, C, 'window', 'window', 2, 1).body is None                   # batch statistics: unsupported
        assert R.bwd_form_of(M, C, 'window', 'misaligned', 2, 0).body is None
    for M, C, lay in R.COLSUM_CASES:                            # gnx_colsum: the forward's slab bodies, whatever the row count
        assert R.COLSUM_FORM[lay] == R.form(8193, C, R.layout(lay, C)[0], R.aligned(lay)).body, (M, C, lay)
    M, C = R.DX_VEC4_LOOP
    f = R.bwd_form_of(M, C, 'window', 'window', 1, 1)
    assert (f.body, f.dx_vec4) == ('slab_vec', 1)


def test_every_form_code_is_reached_by_a_grid_case():
    fwd = {f.body for M, C in R.GRID for f in _forward_forms(M, C)}
    bwd = {f.body for M, C in R.GRID for f in _backward_forms(M, C)}
    assert fwd == set(R.FORMS) - {'eval_fused'}
    assert bwd == set(R.FORMS)
    assert sorted(R.CODES.values()) == list(range(len(R.FORMS)))
    # both values of each flag, on the forms that have it
    assert {(f.body, f.fused) for M, C in R.GRID for f in _forward_forms(M, C)} >= {
        (b, v) for b in ('multi', 'small_keep', 'small_strip') for v in (0, 1)}
    assert {(f.body, f.dx_vec4) for M, C in R.GRID for f in _backward_forms(M, C)} >= {
        ('slab_vec', 0), ('slab_vec', 1), ('slab', 0)}


def test_each_row_threshold_has_a_case_on_both_sides():
    """2048 | 2049 (rows kept in registers | four workgroups), 4992 | 4993 where C > 1024 (strip | slabs), 8192 | 8193."""
    assert [(lo[0], hi[0]) for lo, hi, _, _ in R.ROW_EDGES] == [(8 * R.BN_SL, 8 * R.BN_SL + 1), (R.BN_SMALL_M, R.BN_SMALL_M + 1),
                                                                (R.BN_MULTI_M, R.BN_MULTI_M + 1)]
    for lo, hi, below, above in R.ROW_EDGES:
        assert lo in R.GRID and hi in R.GRID and lo[1] % 4 == 0 and hi[1] % 4 == 0
        assert (lo[1] > 1024 and hi[1] > 1024) == (lo[0] == R.BN_SMALL_M)
        assert (R.form_of(*lo, 'window').body, R.form_of(*hi, 'window').body) == (below, above) and below != above
        assert R.bwd_form_of(*lo, 'window', 'window', 0, 1).body == below
        assert R.bwd_form_of(*hi, 'window', 'window', 0, 1).body == above
