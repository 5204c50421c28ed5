"""tests/wgrad_ref.py proved before test_gpu_wgrad_forms.py uses it: the float64 references against float64 torch autograd, the
input recipe, detectability of every case of GRID and STEM_GRID, and - through `form` / `stem_form`, the Python restatements of
gnx_wgrad_bnrelu's and gnx_conv0_wgrad's dispatch - that the grids reach every kernel body, both sides of every edge between two
of them and every empty-split case.  Runs on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as R


def _close(got, want):
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


# ------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("act", [0, 1])
def test_wgrad1_equals_float64_autograd(act):
    c = R.one(37, 21, 13)
    r = R.recipe(c)
    a = R.activate(r.X, r.scale, r.shift) if act else R.activate(r.X)
    w = torch.zeros(c.N, c.K, dtype=torch.float64, requires_grad=True)
    F.linear(a, w).backward(r.dY)
    ref, T = R.wgrad1(r.dY, a)
    _close(ref, w.grad)
    assert torch.equal(T, r.dY.abs().t() @ a.abs()) and (T >= ref.abs() - 1e-9).all()
    if act:
        # relu(scale x + shift) from the float32 inputs, one rounding
        want = torch.relu(r.X * r.scale + r.shift)
        assert torch.equal(a, want.float().double()) and (a == 0).any() and (a > 0).any()


@pytest.mark.parametrize("imgs,S", [(1, 2), (3, 3), (2, 6), (2, 7)])
@pytest.mark.parametrize("act", [0, 1])
def test_pooled_wgrad_equals_float64_autograd(imgs, S, act):
    c = R.pooled(imgs, S, 5, 6)
    r = R.recipe(c)
    a = R.activate(r.X, r.scale, r.shift) if act else R.activate(r.X)
    p = R.pool2(a, imgs, S)
    want = F.avg_pool2d(a.view(imgs, S, S, c.K).permute(0, 3, 1, 2), 2, 2)                  # floor: torch's default
    assert p.shape == (c.M, c.K)
    _close(p, want.permute(0, 2, 3, 1).reshape(c.M, c.K))
    w = torch.zeros(c.N, c.K, 1, 1, dtype=torch.float64, requires_grad=True)
    y = F.avg_pool2d(F.conv2d(a.view(imgs, S, S, c.K).permute(0, 3, 1, 2), w), 2, 2)         # the transition: conv, then pool
    y.backward(r.dY.view(imgs, S // 2, S // 2, c.N).permute(0, 3, 1, 2))
    ref, T, term = R.reference(c, act, 0)
    _close(ref, w.grad.view(c.N, c.K, 1))
    assert (T >= ref.abs() - 1e-9).all() and term > 0


@pytest.mark.parametrize("imgs,S", [(3, 1), (2, 2), (2, 3), (2, 5), (2, 8)])
@pytest.mark.parametrize("act", [0, 1])
def test_wgrad9_equals_float64_autograd(imgs, S, act):
    c = R.nine(imgs, S, 7, 6)
    r = R.recipe(c)
    a = R.activate(r.X, r.scale, r.shift) if act else R.activate(r.X)
    w = torch.zeros(c.N, c.K, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a.view(imgs, S, S, c.K).permute(0, 3, 1, 2), w, padding=1)
    y.backward(r.dY.view(imgs, S, S, c.N).permute(0, 3, 1, 2))
    ref, T = R.wgrad9(r.dY, a, imgs, S)
    _close(ref, w.grad)
    assert (T >= ref.abs() - 1e-9).all()
    ref2, T2, _ = R.reference(c, act, 1)                                                       # [N][K][taps] is torch's [N][K][3][3]
    _close(ref2, (w.grad + r.dW0.view(c.N, c.K, 3, 3)).reshape(c.N, c.K, 9))
    assert torch.equal(T2, T.reshape(c.N, c.K, 9) + r.dW0.abs())


@pytest.mark.parametrize("s", [R.stem7(2, 16, 32, O=5), R.stem7(2, 20, 30, O=5, pad=2), R.stem7(1, 16, 32, O=3, pad=0),
                               R.stem3(2, 9, 9, 5, 0), R.stem3(2, 8, 33, 5, 1)])
def test_stem_wgrad_equals_float64_autograd(s):
    r = R.stem_recipe(s)
    Ho, Wo = R.stem_out(s)
    w = torch.zeros(s.O, 3, s.KH, s.KH, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(r.x, w, stride=s.stride, padding=s.pad)
    assert y.shape == (s.imgs, s.O, Ho, Wo)
    y.backward(r.dS.view(s.imgs, Ho, Wo, s.O).permute(0, 3, 1, 2))
    ref, T = R.stem_wgrad(r.x, r.dS, s.KH, s.stride, s.pad)
    _close(ref, w.grad)
    assert (T >= ref.abs() - 1e-9).all()


def test_recipe_keeps_every_term_zero_or_away_from_zero():
    c = R.one(300, 9, 64)
    r = R.recipe(c)
    for t, lo, hi in ((r.X, 0.5, 1.5), (r.dY, 0.5, 1.5), (r.dW0, 0.5, 1.5), (r.scale, 0.75, 1.25), (r.shift, 0.125, 0.25)):
        assert t.dtype == torch.float64 and torch.equal(t, t.float().double())               # float32 values
        assert t.abs().min().item() >= lo and t.abs().max().item() <= hi
        assert (t < 0).any() and (t > 0).any()
    a = R.activate(r.X, r.scale, r.shift)
    assert a[a != 0].min().item() >= 0.125 and 0.2 < (a == 0).double().mean().item() < 0.8
    # |scale x| > |shift|: the mask is the sign of scale x, so another channel's scale flips every mask of the column where the
    # signs differ (about half of the channel pairs), and changes every live value everywhere
    b = R.activate(r.X, r.scale.roll(1), r.shift.roll(1))
    differ = r.scale.sign() != r.scale.roll(1).sign()
    assert 8 <= int(differ.sum()) <= 56 and ((a == 0) != (b == 0))[:, differ].all()
    assert (a != b)[(a != 0) | (b != 0)].all()
    r2 = R.recipe(R.one(300, 9, 64))
    assert torch.equal(r.X, r2.X) and torch.equal(r.dW0, r2.dW0)                             # reproducible
    s = R.stem_recipe(R.stem7(2, 16, 32))
    assert s.x.abs().min().item() >= 0.5 and s.dS.abs().min().item() >= 0.5 and (s.x < 0).any() and (s.dS < 0).any()
    assert s.x.abs().max().item() > 1.4 and s.dS.abs().max().item() > 1.4
    # the narrowed range above NARROW_ABOVE positions: only the two cases with more tiles than workgroups
    assert [t for t in R.STEM_GRID if t.imgs * R.stem_out(t)[0] * R.stem_out(t)[1] > R.NARROW_ABOVE] == [R.STEM_FAST_MANY, R.STEM_PLAIN_MANY]
    for many in (R.STEM_FAST_MANY, R.STEM_PLAIN_MANY):
        m = R.stem_recipe(many)
        for t in (m.x, m.dS):
            assert 0.5 <= t.abs().min().item() and t.abs().max().item() <= 0.625 and (t < 0).any() and (t > 0).any()
            assert t.unique().numel() > 100000


# ------------------------------------------------------------------------------------------------------- detectability, G
def test_G_is_what_the_measured_ratios_make_it():
    assert R.G == max(8.0, 4 * R.TORCH_FP32_RATIO, 4 * R.CHAIN_FP32_RATIO)


@pytest.mark.parametrize("c", R.GRID, ids=lambda c: '-'.join(str(v) for v in c))
def test_grid_cases_are_detectable(c):
    for act, acc in R.FLAGS:
        ref, T, term = R.reference(c, act, acc)
        assert ref.shape == (c.N, c.K, c.taps) and bool(torch.isfinite(ref).all())
        assert term >= (0.0625 if act else 0.25) * (0.25 if c.pool else 1.0)
        assert R.detectable(term, R.tol(T)), (c, act, acc, term, 4 * R.tol(T).max().item())


@pytest.mark.parametrize("s", R.STEM_GRID, ids=lambda s: '-'.join(str(v) for v in s))
def test_stem_cases_are_detectable(s):
    ref, T, term = R.stem_reference(s)
    assert term >= 0.25
    assert R.detectable(term, R.tol(T)), (s, term, 4 * R.tol(T).max().item())


def _chain_ratio(c, act):
    r = R.recipe(c)
    ns, ks = R.sample(c.N, 24), R.sample(c.K, 24 if c.taps == 1 else 8)
    X, dY = r.X[:, ks].float(), r.dY[:, ns]
    a = R.activate_fp32(X, r.scale[ks].float(), r.shift[ks].float()) if act else X
    ref, T, _ = R.reference(c, act, 0)
    ref, T = ref[ns][:, ks], T[ns][:, ks]
    if c.pool:
        m = a.view(c.imgs, c.S, c.S, -1)
        So = c.S // 2
        q = [m[:, dy:2 * So:2, dx:2 * So:2] for dy in (0, 1) for dx in (0, 1)]
        B = ((((q[0] + q[1]) + q[2]) + q[3]) * 0.25).reshape(c.M, -1)                        # fp32 sum of four, then the quarter
    elif c.taps == 9:
        B = torch.stack([R.shifted(a, c.imgs, c.S, t // 3, t % 3) for t in range(9)], 2).reshape(c.M, -1)   # [M][k][tap]
    else:
        B = a
    got = R.chain_fp32(dY, B).double().view(len(ns), len(ks), c.taps)
    return R.ratio(got, ref, T)


@pytest.mark.parametrize("c", R.GRID, ids=lambda c: '-'.join(str(v) for v in c))
def test_sequential_fp32_chain_stays_within_the_ratio_G_was_set_from(c, capsys):
    """One of the two figures behind wgrad_ref.G, kept runnable: a sequential fp32 multiply-add chain over the positions against
    the float64 reference, |err| / (2^-24 T), on evenly spread output channels and input channels of every case of GRID, with
    and without the activation."""
    ratio = max(_chain_ratio(c, 0), _chain_ratio(c, 1))
    with capsys.disabled():
        print(' fp32 chain ratio at %s: %.4f' % (tuple(c), ratio))
    assert ratio <= R.CHAIN_FP32_RATIO, ratio


@pytest.mark.parametrize("s", R.STEM_GRID, ids=lambda s: '-'.join(str(v) for v in s))
def test_sequential_fp32_chain_of_the_stem_stays_within_the_ratio(s, capsys):
    r = R.stem_recipe(s._replace(acc=0))
    os_ = R.sample(s.O, 8)
    cols = F.unfold(r.x, (s.KH, s.KH), padding=s.pad, stride=s.stride)                       # [imgs][3 KH KH][Ho Wo]
    ps = R.sample(cols.shape[1], 24)
    B = cols[:, ps].permute(0, 2, 1).reshape(-1, len(ps))
    ref, T, _ = R.stem_reference(s._replace(acc=0))
    ref, T = ref.reshape(s.O, -1)[os_][:, ps], T.reshape(s.O, -1)[os_][:, ps]
    ratio = R.ratio(R.chain_fp32(r.dS[:, os_], B), ref, T)
    with capsys.disabled():
        print(' fp32 chain ratio at %s: %.4f' % (tuple(s), ratio))
    assert ratio <= R.CHAIN_FP32_RATIO, ratio


# ------------------------------------------------------------------------------------------------- the dispatch, restated
def test_split_counts_are_those_of_the_source():
    assert [R.wgrad1_t_splits(M, 128, 132) for M in (224, 225, 256, 512, 513, 544, 545)] == [0, 8, 8, 16, 16, 16, 16]
    assert R.wgrad1_t_splits(256, 128, 128) == 0 and R.wgrad1_t_splits(256, 130, 132) == 0 and R.wgrad1_t_splits(256, 128, 130) == 0
    assert R.wgrad1_t_splits(*R.T1_CAP) == 24 and R.wgrad1_t_splits(100000, 128, 132) == 512
    assert R.wgrad_splits(*R.PF_EMPTY) == 128 and R.wgrad_splits(9 * 1024, 32, 1024) == 128
    assert R.wgrad_splits(1, 1, 1) == 1 and R.wgrad_splits(10 ** 6, 128, 128) == 512 and R.wgrad_splits(10 ** 6, 1024, 2048) == 8
    assert R.workspace_floats(*R.T1, 1) == 8 * 128 * 132 and R.workspace_floats(*R.PF, 1) == 4 * 128 * 128
    assert R.workspace_floats(128, 32, 128, 9) == 2 * 9 * 32 * 128
    # the generic 3x3 fits S = 114 into 160 KB and not 115
    assert R.MAX_S_PLAIN9 == 114 and R.lds_bytes(9, 114) <= R.LDS_LIMIT < R.lds_bytes(9, 115)
    assert R.form(9, 0, 115 * 115, 8, 8, 115, 8, 8).body is None and R.form(9, 0, 114 * 114, 8, 8, 114, 8, 8).body == 'plain9'


def test_grid_reaches_every_body():
    by = {}
    for c in R.GRID:
        for act in (0, 1):
            by.setdefault(R.form_of(c, act).body, []).append(c)
    assert set(by) == set(R.BODIES)
    t1 = by['t1']
    assert {c.K for c in t1} >= {132, 256, 260, 1028} and {c.N for c in t1} >= {128, 256, 512}
    assert {c.M for c in t1} >= {225, 256, 513, 544, 1000}
    pf = by['pf']
    assert {c.M for c in pf} >= {1, 63, 64, 65, 224, 8200} and {c.K for c in pf} >= {4, 8, 128, 132}
    assert any(c.K == 132 and c.M <= 224 for c in pf)
    p1 = by['plain1']
    assert {c.N for c in p1} >= set(R.PLAIN1_N) | {128} and {c.K for c in p1} >= set(R.PLAIN1_K) | {128, 132}
    for shape, body in ((R.T1, 't1'), (R.PF, 'pf')):
        assert R.form_of(R.one(*shape)).body == body
        off = [c for c in R.GRID if (c.M, c.N, c.K) == shape and c.taps == 1 and (c.xlay, c.ylay) != ('aligned', 'aligned')]
        assert {(c.xlay, c.ylay) for c in off} == set(R.MISLAYS)                             # each of the four, alone
        assert all(R.form_of(c, act).body == 'plain1' for c in off for act in (0, 1))
        ss = R.one(*shape, ss=1)
        assert ss in R.GRID and R.form_of(ss, 1).body == 'plain1' and R.form_of(ss, 0).body == body
    pool = by['pool']
    assert {c.S for c in pool} >= set(R.POOL_S) and {c.imgs for c in pool} >= {1, 3}
    assert {c.K for c in pool} >= {6, 130} and {c.N for c in pool} >= {5, 128}
    assert any(c.M > 64 for c in pool)                                                       # more than one tile
    t9 = by['t9']
    for n, S in R.T9_S:
        assert n >= 2 and n * S * S >= 3 * 32
        for K in (128, 256):
            assert R.nine(n, S, 32, K) in t9
    assert any(c.M % 64 == 32 for c in t9) and R.nine(*R.T9_EMPTY) in t9
    p9 = by['plain9']
    assert {c.S for c in p9} >= {1, 2, 3, 5, 64, R.MAX_S_PLAIN9} and {c.N for c in p9} >= {8, 33} and {c.K for c in p9} >= {12, 130}
    assert R.nine(1, 64, 32, 128) in p9 and R.nine(1, 114, 8, 8) in p9
    assert any(c.S == 4 and c.imgs % 2 == 1 and c.M % 32 != 0 and c.N == 32 and c.K == 128 for c in p9)
    assert any(c.xlay == 'shifted' and (c.S, c.N, c.K) == (8, 32, 128) for c in p9)


@pytest.mark.parametrize("shape,body,splits,tps,empty", [
    (R.T1_EMPTY[0], 't1', 16, 2, 7), (R.T1_EMPTY[1], 't1', 16, 2, 7), (R.T1_CAP, 't1', 24, 2, 8), (R.PF_EMPTY, 'pf', 128, 2, 63)])
def test_empty_split_cases_have_empty_splits(shape, body, splits, tps, empty):
    c = R.one(*shape)
    assert c in R.GRID
    f = R.form_of(c)
    assert (f.body, f.splits, f.tps, f.empty) == (body, splits, tps, empty)
    assert [s for s in range(f.splits) if s * f.tps >= f.tiles] == list(range(splits - empty, splits))


def test_empty_split_case_of_the_3x3():
    c = R.nine(*R.T9_EMPTY)
    f = R.form_of(c)
    assert c in R.GRID and (f.body, f.splits, f.tiles, f.tps, f.empty) == ('t9', 128, 288, 3, 32)
    # and the neighbours of the 1x1 cases are whole
    assert R.form_of(R.one(512, 128, 132)).empty == 0 and R.form_of(R.one(*R.T1)).empty == 0


@pytest.mark.parametrize("edge", range(len(R.EDGES)))
def test_every_edge_has_a_case_on_each_side(edge):
    lo, hi, want_lo, want_hi = R.EDGES[edge]
    for c, want in ((lo, want_lo), (hi, want_hi)):
        assert c in R.GRID, c
        f = R.form_of(c)
        assert (f.body, f.splits) == want, (c, f)


def test_stem_grid_reaches_every_body_and_edge():
    by = {}
    for s in R.STEM_GRID:
        by.setdefault(R.stem_form_of(s).body, []).append(s)
    assert set(by) == set(R.STEM_BODIES)
    fast = by['fast']
    assert {(s.H, s.W) for s in fast} >= {(16, 32), (16, 64), (32, 32)} and any(s.ldd == 96 for s in fast)
    f = R.stem_form_of(R.STEM_FAST_MANY)
    assert R.STEM_FAST_MANY in fast and (f.tiles, f.blocks, f.slabs) == (513, 512, 2048)
    assert R.stem_form_of(R.stem7(2, 16, 32)).blocks == 2 and R.stem_form_of(R.stem7(2, 16, 64)).blocks == 4
    p7 = by['plain7']
    assert {s.O for s in p7} >= {10, 33, 64} and any(s.O == 64 and s.ldd == 65 for s in p7)
    assert any(s.W == 30 for s in p7) and any(s.H == 20 for s in p7) and {s.pad for s in p7} >= {0, 2, 3}
    assert any(s.xmis for s in p7)
    f = R.stem_form_of(R.STEM_PLAIN_MANY)
    assert R.STEM_PLAIN_MANY in p7 and f.tiles == 514 and f.blocks == 512
    # each condition of the fast form, broken alone, on the smallest fast case
    base = R.stem7(2, 16, 32)
    for kw in (dict(O=33), dict(ldd=65), dict(W=30), dict(H=20), dict(pad=2), dict(xmis=1)):
        s = base._replace(**kw)
        if 'O' in kw:
            s = s._replace(ldd=kw['O'] + 8)
        assert s in p7, s
    p3 = by['plain3']
    assert {(s.H, s.W) for s in p3} >= {(9, 9), (16, 16), (17, 17), (8, 33)}
    assert {s.O for s in p3} >= {10, 64} and {s.pad for s in p3} >= {0, 1}
    for body in R.STEM_BODIES:
        assert any(s.acc for s in by[body]) and any(not s.acc for s in by[body])
    assert R.stem_form_of(R.stem3(2, 9, 9, 10, 0)).floats == 4 * 2 * 10 * 27
