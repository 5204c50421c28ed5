"""conv1_ref.py proven on the CPU: the float64 references against loops, F.conv2d / F.avg_pool2d and autograd on small shapes, the
restated dispatch against hand-worked values taken from the C source and against the properties the kernel tests rely on (every
body, every listed edge and every error code occurs), the detectability of every case of GRID, and the CPU half of the measurement
G comes from: a sequential fp32 multiply-add chain (the device half is in test_gpu_conv1_forms.py)."""
import pytest
import torch
import torch.nn.functional as F

import conv1_ref as R

SEEN = {}                                     # kind -> (ratio, case)


def ids(c):
    return '-'.join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("c", [R.conv(5, 3, 2), R.conv(5, 3, 2, 0, oact=1), R.conv(7, 4, 6, 1, oact=1), R.pconv(3, 7, 5, 10),
                               R.pconv(5, 2, 12, 22), R.pconv(2, 4, 3, 5, 0)], ids=ids)
def test_conv_reference_agrees_with_loops_and_torch(c):
    r, ref = R.recipe(c), R.reference(c)
    sc, sh = (r.scale, r.shift) if c.act else (None, None)
    osc, osh = (r.oscale, r.oshift) if c.oact else (None, None)
    want = R.naive_conv(r.X, r.W, sc, sh, c.pool, c.S, osc, osh)
    assert torch.allclose(ref.ref, want, rtol=0, atol=1e-12)
    assert bool((ref.T >= ref.ref.abs() - 1e-12).all())
    # torch's own operators, in the reference's order: BN + ReLU, 1x1 convolution, 2x2 average pooling
    x = r.X.double()
    a = torch.relu(x * r.scale.double() + r.shift.double()) if c.act else x
    if c.pool:
        n = R.images(c)
        m = a.view(n, c.S, c.S, c.K).permute(0, 3, 1, 2)
        y = F.avg_pool2d(F.conv2d(m, r.W.double().view(c.N, c.K, 1, 1)), 2, 2).permute(0, 2, 3, 1).reshape(c.M, c.N)
    else:
        y = F.conv2d(a.t().reshape(1, c.K, c.M, 1), r.W.double().view(c.N, c.K, 1, 1)).view(c.N, c.M).t()
    if c.oact:
        y = torch.relu(y * r.oscale.double() + r.oshift.double())
    assert torch.allclose(ref.ref, y, rtol=0, atol=1e-12)
    # the fp32 chain is the same operation
    got = R.chain_fp32(R.act_fp32(c), r.W)
    if c.oact:
        got = torch.relu(torch.addcmul(r.oshift, got, r.oscale))
    assert torch.allclose(got.double(), want, rtol=0, atol=1e-4)


def test_prologue_ranges():
    for c in (R.conv(300, 130, 36), R.pconv(3, 8, 20, 24)):
        r = R.recipe(c)
        pre = r.X.double() * r.scale.double() + r.shift.double()
        a, mag = R.activate(r.X, r.scale, r.shift)
        assert bool((pre.abs() >= 0.5).all()) and bool(((a == 0) | (a >= 0.5)).all()) and bool((mag >= pre.abs()).all())
        assert 0.25 < (r.scale < 0).float().mean().item() < 0.75, 'a fair share of negative scales'
    r = R.recipe(R.dgbn(128, 96))
    pre = r.X.double() * r.scale.double() + r.shift.double()
    assert bool((pre.abs() >= 0.375).all()) and bool((((r.X - r.mean) * r.invstd).abs() >= 0.38).all())
    assert 0.25 < (r.scale < 0).float().mean().item() < 0.75


@pytest.mark.parametrize("c", [R.dgbn(128, 32, 32), R.dgwg(32, 32), R.dgwg(64, 96)], ids=ids)
def test_adjoint_references_are_autograd(c):
    """norm1 -> relu1 -> conv1 in eval mode: z = gamma (x - mean) invstd + beta, scale = gamma invstd, shift = beta - mean scale."""
    r = R.recipe(c)
    sc, sh, mu, inv = (t.double() for t in (r.scale, r.shift, r.mean, r.invstd))
    gamma = (sc / inv).requires_grad_(True)
    beta = (sh + mu * sc).requires_grad_(True)
    x = r.X.double().requires_grad_(True)
    W1 = r.Wt.double().t().contiguous().requires_grad_(True)                   # conv1.weight [bottleneck][cin]
    z = gamma * ((x - mu) * inv) + beta
    assert torch.allclose(z, x * sc + sh, rtol=0, atol=1e-12)
    y = F.conv2d(torch.relu(z).t().reshape(1, -1, c.M, 1), W1.view(W1.shape[0], W1.shape[1], 1, 1)).view(W1.shape[0], c.M).t()
    y.backward(r.dY.double())
    o = R.adjoint(c)
    assert torch.allclose(o.dX - r.dX0.double(), x.grad, rtol=0, atol=1e-11)
    assert torch.allclose(o.dbeta, beta.grad, rtol=0, atol=1e-10) and torch.allclose(o.dgamma, gamma.grad, rtol=0, atol=1e-10)
    if c.op == 'dgwg':
        assert torch.allclose(o.dW, W1.grad, rtol=0, atol=1e-10)
    acc = R.adjoint(c, 1)
    assert torch.allclose(acc.dbeta - o.dbeta, r.dbeta0.double(), rtol=0, atol=1e-12)
    assert bool((acc.T_dgamma > o.T_dgamma).all()) and torch.equal(acc.dX, o.dX)
    assert bool((o.T_dX >= o.dX.abs() - 1e-12).all()) and bool((o.T_dbeta >= o.dbeta.abs() - 1e-9).all())


# ------------------------------------------------------------------------------------------------------- detectability
@pytest.mark.parametrize("c", R.GRID, ids=ids)
def test_every_case_is_detectable(c):
    """The smallest non-zero term is at least 4 x the largest tolerance; one dropped, doubled or misplaced term and one skipped
    chunk of 32 channels are flagged by the comparator of the kernel tests, a NaN is a miss."""
    if c.op == 'conv':
        ref = R.reference(c)
        t = R.tol(ref.T)
        assert R.detectable(ref.term, t), (ref.term, float(t.max()))
        assert not R.flagged(ref.ref, ref.ref, t) and R.flagged(ref.ref + float('nan'), ref.ref, t)
        if not c.oact:                                   # (behind the output ReLU a term shows where the ReLU is open)
            r = R.recipe(c)
            a = R.activate(r.X, r.scale, r.shift)[0] if c.act else r.X.double()
            if c.pool:
                a = R.pool4(a, R.images(c), c.S)
            m = c.M // 2
            while not a[m].any():                        # (the ReLU zeroed every channel of the row)
                m = (m + 1) % c.M
            k = int((a[m] != 0).nonzero()[0])
            one = torch.zeros_like(ref.ref)
            one[m] = a[m, k] * r.W[:, k].double()
            assert bool(((one[m].abs() > t[m]).all())), 'a dropped term'
            assert R.flagged(ref.ref - one, ref.ref, t) and R.flagged(ref.ref + one, ref.ref, t)
            kc = min(32, c.K)
            chunk = torch.zeros_like(ref.ref)
            chunk[m] = r.W[:, :kc].double() @ a[m, :kc]
            assert R.flagged(ref.ref - chunk, ref.ref, t), 'a skipped chunk of channels'
        return
    o = R.adjoint(c, 1)
    assert R.detectable(o.term, R.tol(o.T_dX)), (o.term, float(R.tol(o.T_dX).max()))
    if R.sums_detectable_case(c):
        for T in (o.T_dbeta, o.T_dgamma):
            assert R.detectable(o.sum_term, R.tol(T, R.G_SUMS)), (o.sum_term, float(R.tol(T, R.G_SUMS).max()))
    else:                                                # ... the loss of 32 rows of one column is still seen
        lost = o.g[:32].sum(0).abs()
        live = lost > 4
        assert live.any() and bool((lost[live] > 4 * R.tol(o.T_dbeta, R.G_SUMS)[live]).all())
    if c.op == 'dgwg' and c.M <= R.DW_DETECT_ROWS:
        assert R.detectable(o.dw_term, R.tol(o.T_dW)), (o.dw_term, float(R.tol(o.T_dW).max()))


def test_the_sum_detectability_limits_are_used_on_both_sides():
    adj = R.DGBN_GRID + R.DGWG_GRID
    assert {R.sums_detectable_case(c) for c in adj} == {True, False}
    assert {c.M <= R.DW_DETECT_ROWS for c in R.DGWG_GRID} == {True, False}


# ------------------------------------------------------------------------------------------------------- the dispatch
def test_small_splits_and_slab_plans_agree_with_the_c_source():
    s = R.small_splits
    # conv1x1_small_splits: M > 8192, K < 256, K % 32, N % 4 -> 0; K / 128, capped to 256 workgroups; below 32 workgroups and
    # K / 64 <= 16: K / 64; at most 16
    assert s(8192, 32, 256) == 2 and s(8193, 32, 256) == 0 and s(256, 128, 224) == 0 and s(256, 130, 256) == 0 and s(256, 128, 272) == 0
    assert s(256, 132, 256) == 4 and s(128, 128, 1024) == 16 and s(128, 128, 1088) == 8 and s(4224, 128, 1024) == 7
    assert s(4096, 128, 1024) == 8 and s(128, 128, 2176) == 16 and s(128, 128, 416) == 6 and s(512, 128, 992) == 15
    assert s(8192, 128, 256) == 2 and s(8192, 512, 512) == 0 and s(2048, 128, 512) == 4
    f = R.conv_form(128, 128, 416, 424, 136, ws=1)
    assert (f.body, f.splits, f.ksplit, f.nz, f.wgs, f.gy) == ('split', 6, 96, 5, 1, 1)
    f = R.conv_form(4224, 128, 1024, 1032, 136, ws=1)
    assert (f.splits, f.ksplit, f.nz, 1024 - (f.nz - 1) * f.ksplit) == (7, 160, 7, 64)              # a last split shorter than the others
    f = R.conv_form(128, 128, 2176, 2184, 136, ws=1)
    assert (f.splits, f.ksplit, f.nz) == (16, 160, 14)
    p = R.dgwg_plan
    # full_blocks / rest_cols / plan32: K = 32 q: q = 3 runs as a fourth wave of one more full block
    want = {32: (0, 1, False), 64: (0, 2, False), 96: (1, 0, True), 128: (1, 0, False), 160: (1, 1, False), 192: (1, 2, False),
            224: (2, 0, True), 288: (2, 1, False), 352: (3, 0, True)}
    for K, (full, rest, idle) in want.items():
        q = p(96, K)
        assert (q.full, q.rest, q.idle) == (full, rest, idle), K
    q = p(96, 160)                                       # 3 tiles: a slab each; cw = 256
    assert (q.slabs_full, q.per_full, q.slabs_rest, q.per_rest, q.floats) == (3, 1, 3, 1, 6 * 130 * 256)
    q = p(32 * 601, 128)                                 # 601 tiles on at most 512 slabs: 2 per slab, 301 slabs, the last of one
    assert (q.slabs_full, q.per_full, q.floats) == (301, 2, 301 * 130 * 128)
    q = p(32 * 1031, 64)                                 # rest 2: at most 1024 slabs
    assert (q.slabs_rest, q.per_rest, q.slabs_full) == (516, 2, 0)
    q = p(32 * 40, 352)                                  # three full blocks: at most 171 slabs
    assert (q.slabs_full, q.per_full) == (40, 1) and p(32 * 400, 352).slabs_full == 134 and p(32 * 400, 352).per_full == 3
    assert p(32, 32).floats == 130 * 128 and p(31, 32).floats == 0 and p(32, 31).floats == 0


def test_form_rules():
    f = R.conv_form
    assert f(128, 32, 32, 40, 37).body == 'ws_act' and f(128, 32, 32, 40, 37, 0).body == 'ws' and f(128, 32, 32, 40, 37, 1, 1, 4).body == 'ws_pool'
    assert f(128, 32, 32, 40, 37, 0, 1, 4).body == 'pool_vec' and f(128, 32, 32, 40, 37, 1, 1, 5).body == 'pool_vec'
    assert f(128, 32, 32, 41, 37).body == 'generic' and f(128, 32, 32, 40, 37, mis=('scale',)).body == 'generic'
    assert f(128, 32, 32, 40, 37, 0, mis=('scale',)).body == 'ws' and f(128, 32, 32, 40, 37, 1, 1, 4, mis=('W',)).body == 'pool'
    assert f(128, 32, 2048, 2056, 37).body == 'ws_act' and f(128, 32, 2080, 2088, 37).body == 'generic_vec'
    assert f(128, 32, 32, 65535 // 4 * 4, 37).body == 'ws_act' and f(128, 32, 32, 65536, 37).body == 'generic_vec'
    assert f(128, 32, 32, 40, 65535).body == 'ws_act' and f(128, 32, 32, 40, 65536).body == 'generic_vec'
    assert f((1 << 29) - 128, 32, 32, 40, 37).body == 'ws_act' and f(1 << 29, 32, 32, 40, 37).body == 'generic_vec'
    assert f(1 << 29, 32, 32, 40, 37).wgs == 1 << 22
    p = f(R.ROUNDS2_M, 160, 32, 40, 165)
    assert (p.wgs, p.tilesN, p.T, p.full, p.partial, p.jmap) == (512, 2, 514, 1, 2, True)
    p = f(R.ROUNDS_M, 32, 32, 40, 37)
    assert (p.wgs, p.tilesN, p.T, p.full, p.partial, p.jmap) == (512, 1, 513, 1, 1, False)
    assert f(1024, 352, 32, 40, 357).jmap and not f(256, 352, 32, 40, 357).jmap and f(1024, 160, 32, 40, 165).jmap
    assert not f(256, 160, 32, 40, 165).jmap
    assert f(0, 32, 32, 40, 37).wgs == 0 and f(0, 32, 32, 40, 37).err == R.OK
    # the split form wants everything aligned; the workspace argument alone decides nothing else
    assert f(128, 128, 416, 424, 136, ws=1).body == 'split' and f(128, 128, 416, 424, 136, ws=1, mis=('out',)).body == 'ws_act'
    assert f(128, 128, 416, 424, 136, 1, 0, 0, 1, ws=1, mis=('oscale',)).body == 'ws_act' and f(128, 128, 416, 424, 136, 1, 0, 0, 1, ws=1).body == 'split'
    d = R.dgbn_form
    assert d(128, 32, 128, 136, 39, 45).wgs == 1 and d(R.ROUNDS_M, 32, 32, 40, 39, 45).runs == (1, 2)
    p = d(R.ROUNDS2_M, 160, 32, 40, 167, 173)
    assert (p.wgs, p.tilesN, p.T, p.runs) == (512, 2, 514, (1, 2))
    assert R.dgbn_workspace(256, 96) == (8 + 256) * 96


def test_every_tile_is_taken_once():
    """The restated tile maps of the persistent forms cover every tile exactly once, jmap and partial round included."""
    for c in R.CONV_GRID:
        f = R.form_of(c)
        if f.body in ('ws', 'ws_act', 'ws_pool'):
            rounds = f.full + (1 if f.partial else 0)
            tiles = [R.ws_tile(f, b, r) for r in range(rounds) for b in range(f.wgs)]
            assert sorted(t for t in tiles if t is not None) == list(range(f.T)), ids(c)


def test_every_body_edge_and_error_code_occurs():
    forms = {c: R.form_of(c) for c in R.GRID}
    assert all(f.err == R.OK for f in forms.values())
    cf = {c: f for c, f in forms.items() if c.op == 'conv'}
    assert {f.body for f in cf.values()} == set(R.BODIES)
    for a, b, fa, fb in R.EDGES:
        assert a in forms and b in forms, (a, b)
        assert (forms[a].body, forms[b].body) == (fa, fb), (a, b, forms[a].body, forms[b].body)
    for c, (splits, nz) in R.SPLIT_EDGES.items():
        assert (forms[c].body, forms[c].splits, forms[c].nz) == ('split', splits, nz), c
    by = lambda body: [(c, f) for c, f in cf.items() if f.body == body]                      # noqa: E731
    gen = by('generic')
    assert {c.lay for c, _ in gen} >= {'ash', 'wsh', 'ssh', 'aodd'} and {c.K for c, _ in gen} >= {1, 3, 22, 31, 33, 37}
    assert {c.M for c, _ in gen} >= {1, 127, 129} and {c.N for c, _ in gen} >= {1, 127, 129}
    assert {c.act for c, _ in gen} == {0, 1} and any(c.oact for c, _ in gen)
    assert {c.S for c, _ in by('pool')} >= {7, 2} and {c.act for c, _ in by('pool')} == {0, 1}
    vec = by('generic_vec')
    assert any(c.M % 128 and c.N % 128 and c.K % 32 for c, _ in vec) and any(c.K > R.C1_KMAX for c, _ in vec)
    assert any(c.M > 256 and c.M % 128 and c.N > 128 and c.K % 32 == 0 for c, _ in vec), 'interior and edge tiles in one launch'
    assert {c.big for c, _ in vec} >= {'lda', 'ldc'} and any(c.oact for c, _ in vec)
    pv = by('pool_vec')
    assert any(not c.act and c.M % 128 == 0 for c, _ in pv) and any(c.S % 2 and c.M % 128 == 0 for c, _ in pv) and any(c.M % 128 for c, _ in pv)
    sp = by('split')
    assert any(f.nz < f.splits for _, f in sp) and any(c.K % f.ksplit for c, f in sp) and {c.act for c, _ in sp} == {0, 1}
    assert any(c.M % 128 for c, _ in sp) and any(c.N % 32 for c, _ in sp) and {f.splits for _, f in sp} >= {2, 4, 6, 7, 8, 16}
    assert {c.lay for c in cf if c.ws == 1} >= {'al', 'wmis', 'codd'} and any(c.ws == 2 for c in cf)
    for body in ('ws', 'ws_act'):
        fs = by(body)
        assert {c.K for c, _ in fs} >= {32, 64, 96} and {c.N for c, _ in fs} >= {32, 64, 96, 128, 160, 192, 352}, body
        assert any(f.T == 1 for _, f in fs) and {(f.tilesN, f.jmap) for _, f in fs} >= {(2, True), (2, False), (3, True), (3, False)}, body
        assert any(f.T > 512 and f.tilesN == 1 and f.partial for _, f in fs) and any(f.T > 512 and f.tilesN == 2 and f.partial and f.jmap for _, f in fs)
    assert any(c.K == 2048 for c, _ in by('ws_act')) and any(c.oact for c, _ in by('ws_act')) and any(c.oact for c, _ in by('ws'))
    assert any(f.full == 2 and not f.partial for _, f in by('ws_act'))
    wp = by('ws_pool')
    assert {c.S for c, _ in wp} >= {4, 8, 16, 64} and {f.tilesN for _, f in wp} >= {1, 2, 3} and any(f.T > 512 for _, f in wp)
    assert any(c.K == 2048 for c, _ in wp) and all(R.rows_in(c) == 4 * c.M for c, _ in wp)
    # the fused gradients
    assert {c.N for c in R.DGBN_GRID} >= {32, 96, 128, 160, 992} and any(c.M == 128 for c in R.DGBN_GRID)
    assert {(forms[c].tilesN, forms[c].runs) for c in R.DGBN_GRID if forms[c].T > 512} == {(1, (1, 2)), (2, (1, 2))}
    assert all(R.layout(c).ldx != R.layout(c).ldc for c in R.DGBN_GRID + R.DGWG_GRID)
    assert {c.K for c in R.DGWG_GRID} >= {32, 64, 96, 128, 160, 192, 224, 288} and any(c.M == 32 for c in R.DGWG_GRID)
    assert set().union(*(forms[c].shapes for c in R.DGWG_GRID)) == set(R.DGWG_SHAPES)
    plans = [R.dgwg_plan(c.M, c.K) for c in R.DGWG_GRID]
    assert any(p.slabs_full == 1 or p.slabs_rest == 1 for p in plans)
    assert any(p.per_full > 1 and (c.M // 32) % p.per_full for c, p in zip(R.DGWG_GRID, plans))
    assert any(p.per_rest > 1 and (c.M // 32) % p.per_rest for c, p in zip(R.DGWG_GRID, plans))
    # the refusals, through the restatement
    lo = R.layout(R.conv(128, 32, 32))
    for kw, code in R.CONV_REFUSALS:
        a = dict(M=128, N=32, K=32, lda=lo.lda, ldc=lo.ldc)
        a.update(kw)
        assert R.conv_form(**a).err == code, kw
    b = R.dgbn(128, 96)
    lo = R.layout(b)
    for kw, code in R.DGBN_REFUSALS + [(dict(null=(n,)), R.BAD_ARG) for n in R.DGBN_NULLS]:
        a = dict(M=b.M, N=b.N, K=b.K, lddy=lo.lda, ldx=lo.ldx, lddx=lo.ldc)
        a.update(kw)
        assert R.dgbn_form(**a).err == code, kw
    b = R.dgwg(96, 64)
    lo = R.layout(b)
    for kw, code in R.DGWG_REFUSALS + [(dict(null=(n,)), R.BAD_ARG) for n in R.DGWG_NULLS]:
        a = dict(M=b.M, K=b.K, lddb=lo.lda, ldx=lo.ldx, ldg=lo.ldc)
        a.update(kw)
        assert R.dgwg_form(**a).err == code, kw
    assert {code for _, code in R.DGBN_REFUSALS} == {code for _, code in R.DGWG_REFUSALS} == {R.BAD_ARG, R.UNSUPPORTED}
    # the layouts
    assert all(R.layout(c).lda > c.K for c in cf) and all(R.layout(c).ldc > c.N for c in cf)
    assert all(R.layout(c).ldc % 2 == 1 or c.ws == 1 or c.big == 'ldc' for c in cf)
    assert {R.layout(c).c_off for c in cf} == {1, 3, 4}


# ------------------------------------------------------------------------------------------------------- where G comes from
def _see(kind, ratio, c):
    if ratio > SEEN.get(kind, (-1.0, None))[0]:
        SEEN[kind] = (ratio, c)


@pytest.mark.parametrize("c", R.GRID, ids=ids)
def test_plain_fp32_chain_stays_within_the_ratio_G_was_set_from(c, capsys):
    """The CPU half of the measurement behind conv1_ref.G / G_SUMS: the reference operation as a sequential fp32 multiply-add chain
    (the prologue as one fp32 multiply-add and a max, the pooled mean as three additions and a multiplication, the column sums as a
    sequential fp32 sum over the rows) against the float64 reference, max |err| / (2^-24 T)."""
    r = R.recipe(c)
    rs = 0.0
    if c.op == 'conv':
        ref = R.reference(c)
        got = R.chain_fp32(R.act_fp32(c), r.W)
        if c.oact:
            got = torch.relu(torch.addcmul(r.oshift, got, r.oscale))
        ratio = R.ratio(got, ref.ref, ref.T)
    else:
        o = R.adjoint(c)
        mask = (torch.addcmul(r.shift, r.X, r.scale) > 0).float()
        g = R.chain_fp32(r.dY, r.Wt) * mask
        ratio = R.ratio(torch.addcmul(r.dX0, g, r.scale), o.dX, o.T_dX)
        if c.op == 'dgwg':
            a = torch.relu(torch.addcmul(r.shift, r.X, r.scale))
            ratio = max(ratio, R.ratio(R.chain_fp32_t(r.dY, a), o.dW, o.T_dW))
        rs = max(R.ratio(R.seq_sum(g), o.dbeta, o.T_dbeta), R.ratio(R.seq_sum(g * ((r.X - r.mean) * r.invstd)), o.dgamma, o.T_dgamma))
        _see('sums', rs, c)
        with capsys.disabled():
            print(' fp32 chain ratio of the column sums at %s: %.4f' % (ids(c), rs))
    _see('chain', ratio, c)
    with capsys.disabled():
        print(' fp32 chain ratio at %s: %.4f' % (ids(c), ratio))
    assert ratio <= R.G / 4 and rs <= R.G_SUMS / 4, (ratio, rs)


def test_report_the_cpu_ratios(capsys):
    """Prints the largest ratios the tests above saw and holds the recorded ones to G / 4 (empty when run alone)."""
    with capsys.disabled():
        print('\n G = %.3f, G_SUMS = %.3f' % (R.G, R.G_SUMS))
        for kind, (ratio, c) in sorted(SEEN.items()):
            print(' largest fp32 %-5s ratio %.4f at %s' % (kind, ratio, ids(c)))
    assert R.CHAIN_FP32_RATIO <= R.G / 4 and R.TORCH_FP32_RATIO <= R.G / 4
    assert R.CHAIN_FP32_SUM_RATIO <= R.G_SUMS / 4 and R.TORCH_FP32_SUM_RATIO <= R.G_SUMS / 4
    assert R.G >= R.G_FLOOR and R.G_SUMS >= R.G_FLOOR
