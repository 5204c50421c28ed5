"""conv3_ref.py proven on the CPU: the float64 references against loops and against autograd on tiny shapes, the restated
dispatch against the properties the kernel tests rely on (every body and every edge occurs in GRID), the comparator against
references with one deliberate fault at every GRID shape, and the two CPU halves of the measurement G comes from: a sequential
fp32 multiply-add chain and, for Winograd, an fp32 emulation of the F(2,3)-along-x algebra (the device half is in
test_gpu_conv3_forms.py).  The 8-wave cases are measured on their sampled images; the adjoint sums of the one 8-wave adjoint case
run over all 262144 rows and are measured on the device only."""
import pytest
import torch
import torch.nn.functional as F

import conv3_ref as R

SEEN = {}                                     # kind -> (ratio, case)


def ids(c):
    return '-'.join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("n,S,K,N", [(1, 1, 3, 2), (3, 1, 2, 3), (2, 2, 3, 4), (2, 3, 2, 2), (2, 4, 3, 5)])
def test_references_agree_with_loops(n, S, K, N):
    g = torch.Generator().manual_seed(S + 10 * n)
    a, W = R._signed(g, 0.5, 1.5, n * S * S, K).double(), R._signed(g, 0.5, 1.5, N, K, 3, 3).double()
    want = R.naive_conv(a, W, n, S)
    assert torch.allclose(R.conv2(a, W, n, S), want, rtol=0, atol=1e-13)
    assert torch.allclose(R.chain_fp32(a, W, n, S).double(), want, rtol=0, atol=1e-4)
    T = R.conv2(a.abs(), W.abs(), n, S)
    assert torch.equal(T, R.conv2(a.abs(), W.abs(), n, S)) and bool((T >= want.abs() - 1e-12).all())
    if S == 1:                                 # only the centre tap lies inside a 1 x 1 map
        assert torch.allclose(want, a @ W[:, :, 1, 1].t(), rtol=0, atol=1e-13)
    if S % 2 == 0:                             # the Winograd algebra is the same sum; its T bounds the direct one
        assert torch.allclose(R.wino_fp32(a, W, n, S).double(), want, rtol=0, atol=1e-4)
        Uw = R.winograd_weights(W)
        V = R.wino_pairs(a, n, S)
        m = sum(torch.einsum('iypxk,xnk->iypxn', V[:, dy:dy + S], Uw[dy]) for dy in range(3))
        y = torch.stack([m[:, :, :, 0] + m[:, :, :, 1] + m[:, :, :, 2], m[:, :, :, 1] - m[:, :, :, 2] - m[:, :, :, 3]], 3)
        assert torch.allclose(y.reshape(n * S * S, N), want, rtol=0, atol=1e-12)
        assert bool((R.wino_T(a, W, n, S) >= want.abs() - 1e-12).all())


def test_prologue_and_layout_formulas():
    g = torch.Generator().manual_seed(5)
    x, sc, sh = R._signed(g, 0.5, 1.5, 50, 7), R._signed(g, 1.5, 2.0, 7), R._signed(g, 0.125, 0.25, 7)
    a, mag = R.activate(x, sc, sh)
    pre = x.double() * sc.double() + sh.double()
    assert bool((pre.abs() >= 0.5).all()) and bool(((a == 0) | (a >= 0.5)).all()) and bool((mag >= pre.abs()).all())
    W = torch.arange(5 * 7 * 9, dtype=torch.float32).view(5, 7, 3, 3)
    wr, wb, wu = R.repack(W), R.repack_bwd(W), R.winograd_weights(W)
    for tap in range(9):
        assert torch.equal(wr[tap], W[:, :, tap // 3, tap % 3]) and torch.equal(wb[8 - tap], W[:, :, tap // 3, tap % 3].t())
    assert wu.shape == (3, 4, 5, 7) and torch.equal(wu[1, 0], W[:, :, 1, 0]) and torch.equal(wu[2, 3], W[:, :, 2, 2])
    assert torch.equal(wu[0, 1], 0.5 * ((W[:, :, 0, 0] + W[:, :, 0, 2]) + W[:, :, 0, 1]))
    assert torch.equal(wu[0, 2], 0.5 * ((W[:, :, 0, 0] + W[:, :, 0, 2]) - W[:, :, 0, 1]))
    # the data-gradient entry points take gnx_repack_conv3x3_bwd of conv2's weight = gnx_repack_conv3x3 of dgrad_weight
    assert torch.equal(R.repack(R.dgrad_weight(W)), R.repack_bwd(W))


def test_adjoint_reference_is_autograd():
    c = R.adj(2, 4)
    r = R.recipe(c)
    M = R.rows(c)
    x = torch.zeros(2, 128, 4, 4, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, r.W.double(), padding=1)                                   # conv2: 128 channels in, 32 out
    y.backward(r.X.double().view(2, 4, 4, 32).permute(0, 3, 1, 2))
    g = x.grad.permute(0, 2, 3, 1).reshape(M, 128)
    assert torch.allclose(R.reference(c).ref, g, rtol=0, atol=1e-12)
    # norm2 -> relu2 in eval mode: z = scale' xhat + beta with xhat = (x - mean) invstd, a = relu(z); dX = dz scale
    o = R.adjoint(c)
    mask = (r.act > 0).double()
    assert torch.allclose(o.dX, r.scale.double() * g * mask, rtol=0, atol=1e-12)
    assert torch.allclose(o.dbeta, (g * mask).sum(0), rtol=0, atol=1e-10)
    xhat = ((r.act.double() - r.shift.double()) / r.scale.double() - r.mean.double()) * r.invstd.double()
    assert torch.allclose(o.dgamma, (g * mask * xhat).sum(0), rtol=0, atol=1e-10)
    assert bool((xhat.abs()[r.act > 0] >= 0.28).all())
    acc = R.adjoint(c, 1)
    assert torch.allclose(acc.dbeta - o.dbeta, r.dbeta0.double(), rtol=0, atol=1e-12)
    assert bool((acc.T_dgamma > o.T_dgamma).all())


def test_half_ulp():
    x = torch.tensor([1.0, 1.5, 2.0, 100.0, 128.0, 2.0 ** -14, 2.0 ** -20], dtype=torch.float64)
    want = torch.tensor([2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -5, 2.0 ** -4, 2.0 ** -25, 2.0 ** -25], dtype=torch.float64)
    assert torch.equal(R.half_ulp16(x), want)
    h = torch.tensor([100.03], dtype=torch.float64)
    assert abs(h.half().double() - h).item() <= R.half_ulp16(h).item()


# ------------------------------------------------------------------------------------------------------- the dispatch
def test_every_body_and_edge_occurs_in_the_grid():
    forms = {c: R.form_of(c) for c in R.GRID}
    assert all(f.body is not None for f in forms.values())
    bodies = {f.body for f in forms.values()}
    assert bodies == set(R.BODIES) | {'wino', 'adj4', 'adj8', 'h4', 'h8'}
    for a, b, fa, fb in R.EDGES:
        assert a in forms and b in forms, (a, b)
        assert (forms[a].body, forms[b].body) == (fa, fb), (a, b, forms[a].body, forms[b].body)
    assert sum(1 for _, _, fa, fb in R.EDGES if fa != fb) == len(R.EDGES) - 1
    for body, counts in R.TILE_EDGES.items():
        have = {f.T for f in forms.values() if f.body == body}
        assert set(counts) <= have, (body, counts, sorted(have))
    for body in ('dma4', 'dmag4', 'wino', 'adj4', 'h4'):
        fs = [f for f in forms.values() if f.body == body]
        assert {f.xcd for f in fs} == {True, False}, body                      # G % 8 == 0 and not
        assert any(f.partial and f.full for f in fs) and any(f.one_strip for f in fs), body
        assert body != 'dma4' or any(f.rounds == 2 and not f.partial for f in fs)                  # two whole rounds
    for body in ('dma8', 'dmag8', 'adj8', 'h8'):
        assert all(f.bm == 256 and f.G == 256 and f.full >= 4 for f in forms.values() if f.body == body)
    assert any(f.body == 'dma8' and f.partial for f in forms.values())
    assert any(f.body == 'wino' and f.ragged for f in forms.values()) and any(f.body == 'wino' and f.T == 1 and f.ragged == 16
                                                                              for f in forms.values())
    # every map size of every persistent body
    for body, sizes in (('dma4', R.DMA_S), ('dmag4', R.DMA_S), ('wino', R.POW2_S), ('adj4', R.POW2_S), ('h4', R.POW2_S)):
        assert {c.S for c, f in forms.items() if f.body == body} >= set(sizes), body
    assert {c.K for c, f in forms.items() if f.body == 'dma4'} >= {64, 128, 192}
    assert {c.N for c, f in forms.items() if f.body == 'dmag4'} >= {64, 128, 192}
    assert {c.K for c, f in forms.items() if f.body == 'wino'} >= {32, 64, 96}
    assert {(c.K, f.T) for c, f in forms.items() if f.body == 'h4'} >= {(K, T) for K in (128, 256) for T in (1, 256, 257)}
    assert {c.K for c, f in forms.items() if f.body == 'generic'} >= {1, 3, 33} and {c.N for c in R.CONV_GRID} >= {1, 31, 33, 64}
    assert {c.big for c in R.GRID} == {0, 1} and {R.layout(c).c_off for c in R.GRID} == {1, 3}
    assert all(R.layout(c).ldc % 2 == 1 and R.layout(c).lda > c.K and R.layout(c).pad >= c.S + 17 for c in R.GRID)


def test_form_rules():
    f = R.form
    assert f(128, 32, 64, 8, 72, 37, 0).body == 'dma4' and f(128, 32, 32, 8, 40, 37, 0).body == 'pipe5'      # 32 | K is not enough
    assert f(128, 32, 64, 8, 72, 37, 0, a_mis=True).body == 'generic' and f(128, 32, 64, 8, 73, 37, 0).body == 'generic'
    assert f(128, 32, 64, 8, 72, 37, 1, ss_mis=True).body == 'generic' and f(128, 32, 64, 8, 72, 37, 0, w_mis=True).body == 'generic'
    assert f(1 << 21, 32, 64, 8, 1024, 37, 0).body == 'pipe5' and f((1 << 21) - 128, 32, 64, 8, 1024, 37, 0).body == 'dma4'
    assert f(R.MAX_S ** 2, 4, 8, R.MAX_S, 8, 4, 0).body == 'generic' and f((R.MAX_S + 1) ** 2, 4, 8, R.MAX_S + 1, 8, 4, 0).body is None
    assert R.MAX_S == 359
    p = f(128 * 600, 32, 64, 4, 72, 37, 0)
    assert (p.G, p.T, p.full, p.partial, p.rounds, p.xcd, p.head, p.tail) == (256, 600, 2, 88, 3, True, 1, 1)
    assert f(128 * 7, 32, 64, 4, 72, 37, 0).xcd is False and f(4096, 32, 64, 64, 72, 37, 1).body == 'pipe9'
    w = R.wino_form
    assert w(16, 32, 32, 4, 40, 37).T == 1 and w(16, 32, 32, 4, 40, 37).ragged == 16 and w(256, 32, 32, 4, 40, 37).ragged == 0
    for bad in (dict(N=64), dict(K=48), dict(lda=41), dict(a_mis=True), dict(w_mis=True), dict(S=7), dict(lda=1 << 27)):
        kw = dict(M=49 * 16 if bad.get('S') == 7 else 64, N=32, K=32, S=4, lda=40, ldc=37)
        kw.update(bad)
        assert w(**kw).body is None, bad
    a = R.adj_form
    assert a(128, 128, 32, 4, 40, 140, 133).body == 'adj4' and a(262144, 128, 32, 32, 40, 140, 133).body == 'adj8'
    assert a(262144, 128, 32, 64, 40, 140, 133).body == 'adj4'
    for bad in (dict(K=64), dict(N=64), dict(M=144), dict(lddy=41), dict(dy_mis=True)):
        kw = dict(M=128, N=128, K=32, S=4, lddy=40, lda=140, lddx=133)
        kw.update(bad)
        assert a(**kw).body is None, bad
    h = R.f16_form
    assert h(128, 32, 128, 4, 144, 37).resident and not h(128, 32, 256, 4, 272, 37).resident
    for bad in (dict(lda16=132), dict(K=64), dict(N=24), dict(S=7, M=6272)):
        kw = dict(M=128, N=32, K=128, S=4, lda16=144, ldc=37)
        kw.update(bad)
        assert h(**kw).body is None, bad


def test_sampled_images_cover_the_round_boundaries():
    for c in R.GRID:
        imgs = R.sampled_images(c)
        if imgs is None:
            assert R.rows(c) < R.WIDE_ROWS - 256
            continue
        f = R.form_of(c)
        tiles = set()
        ss = c.S * c.S
        for i in imgs:
            tiles |= set(range(i * ss // f.bm, ((i + 1) * ss - 1) // f.bm + 1))
        want = {0, 1, f.T - 2, f.T - 1} | {b + d for b in range(f.G, f.T, f.G) for d in (-1, 0)}
        assert want <= tiles and len(tiles) >= len(want) + 4 and len(imgs) * ss <= 24 * 4096, ids(c)


# ------------------------------------------------------------------------------------------------------- the comparator
def _operands(c):
    """(a [rows][K], W [N][K][3][3], per-element tolerance, ref, n images): the activated operand in float64 on the rows the
    reference covers, and the tolerance the kernel test applies to the case's output map."""
    r, ref = R.recipe(c), R.reference(c)
    X = r.X if ref.rows is None else r.X[ref.rows]
    a = R.activate(X, r.scale, r.shift)[0] if c.act else X.double()
    W = (R.dgrad_weight(r.W) if c.op == 'adj' else r.W).double()
    if c.op == 'adj':
        o = R.adjoint(c)
        return a, W, R.tol(o.T_dX), o.dX, ref.n, o.term
    t = R.tol(ref.T, R.g_of(c))
    if c.op == 'h16':
        t = t + R.half_ulp16(ref.ref.abs() + t)
    return a, W, t, ref.ref, ref.n, ref.term


@pytest.mark.parametrize("c", R.GRID, ids=ids)
def test_one_fault_is_flagged(c):
    """A reference with one tap dropped at one pixel, one tap doubled, one pixel taken from the neighbouring row or image (the
    wrap a missing border mask gives) or one chunk of 32 channels skipped is flagged by the comparator of the kernel tests."""
    a, W, t, ref, n, term = _operands(c)
    S, M = c.S, a.shape[0]
    if c.op != 'h16':
        assert R.detectable(term, t), 'the smallest non-zero term is below 4 tolerances'
    assert not R.flagged(ref, ref, t) and R.flagged(ref + float('nan'), ref, t)
    P = ((n // 2) * S + S // 2) * S                                            # x = 0 of a middle row of a middle image
    while not a[P].any():                                                      # (the ReLU zeroed every channel there)
        P += S
    if c.op == 'adj':
        r = R.recipe(c)
        rows_ = R.reference(c).rows
        act = r.act if rows_ is None else r.act[rows_]
        post = lambda d, p: r.scale.double() * d * (act[p] > 0)                # noqa: E731
    else:
        post = lambda d, p: d                                                  # noqa: E731

    def miss(p, delta):
        return bool((post(delta, p).abs() > t[p]).any())
    centre = W[:, :, 1, 1] @ a[P]
    assert miss(P, -centre), 'a dropped tap'
    assert miss(P, centre), 'a doubled tap'
    if M > 1:
        Q, kx = (P, 0) if P > 0 else (S - 1, 2)                                # tap (1, kx) of pixel Q lies outside the row
        nb = Q - 1 if kx == 0 else Q + 1
        while not a[nb].any():
            Q, nb = Q + S, nb + S
        assert miss(Q, W[:, :, 1, kx] @ a[nb]), 'a pixel of the neighbouring row or image'
    kc = min(32, c.K)
    y, x = (P // S) % S, P % S
    chunk = torch.zeros(W.shape[0], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            yy, xx = y + ky - 1, x + kx - 1
            if 0 <= yy < S and 0 <= xx < S:
                chunk += W[:, :kc, ky, kx] @ a[P + (ky - 1) * S + kx - 1, :kc]
    assert miss(P, -chunk), 'a skipped chunk of channels'


# ------------------------------------------------------------------------------------------------------- where G comes from
def _see(kind, ratio, c):
    if ratio > SEEN.get(kind, (-1.0, None))[0]:
        SEEN[kind] = (ratio, c)


def _seq_sum(v):
    acc = torch.zeros(v.shape[1], dtype=torch.float32)
    for m in range(v.shape[0]):
        acc = acc + v[m]
    return acc


@pytest.mark.parametrize("c", R.GRID, ids=ids)
def test_plain_fp32_chain_stays_within_the_ratio_G_was_set_from(c, capsys):
    """The CPU half of the measurement behind conv3_ref.G / G_WINO / G_SUMS: the reference operation as a sequential fp32
    multiply-add chain (the prologue as one fp32 multiply-add and a max; Winograd cases through the F(2,3)-along-x algebra in
    fp32) against the float64 reference, max |err| / (2^-24 T)."""
    r, ref = R.recipe(c), R.reference(c)
    X = r.X if ref.rows is None else r.X[ref.rows]
    a = torch.relu(torch.addcmul(r.shift, X, r.scale)) if c.act else X
    W = R.dgrad_weight(r.W) if c.op == 'adj' else r.W
    if c.op == 'wino':
        kind, bound = 'wino', R.G_WINO / 4
        ratio = R.ratio(R.wino_fp32(a, W, ref.n, c.S), ref.ref, ref.T)
    else:
        kind, bound = 'chain', R.G / 4
        g32 = R.chain_fp32(a, W, ref.n, c.S)
        ratio = R.ratio(g32, ref.ref, ref.T)
    _see(kind, ratio, c)
    with capsys.disabled():
        print(' fp32 %s ratio at %s: %.4f' % (kind, ids(c), ratio))
    if c.op == 'adj' and ref.rows is None:
        o = R.adjoint(c)
        d32 = g32 * (r.act > 0)
        xhat32 = ((r.act - r.shift) / r.scale - r.mean) * r.invstd
        rs = max(R.ratio(_seq_sum(d32), o.dbeta, o.T_dbeta), R.ratio(_seq_sum(d32 * xhat32), o.dgamma, o.T_dgamma))
        _see('sums', rs, c)
        with capsys.disabled():
            print(' fp32 chain ratio of the adjoint sums at %s: %.4f' % (ids(c), rs))
        assert rs <= R.G_SUMS / 4, rs
    assert ratio <= bound, ratio


def test_report_the_cpu_ratios(capsys):
    """Prints the largest ratios the tests above saw and holds the recorded ones to G / 4 (empty when run alone)."""
    with capsys.disabled():
        print('\n G = %.3f, G_WINO = %.3f, G_SUMS = %.3f' % (R.G, R.G_WINO, R.G_SUMS))
        for kind, (ratio, c) in sorted(SEEN.items()):
            print(' largest fp32 %-5s ratio %.4f at %s' % (kind, ratio, ids(c)))
    assert R.CHAIN_FP32_RATIO <= R.G / 4 and R.TORCH_FP32_RATIO <= R.G / 4 and R.WINO_FP32_RATIO <= R.G_WINO / 4
    assert R.CHAIN_FP32_SUM_RATIO <= R.G_SUMS / 4 and R.TORCH_FP32_SUM_RATIO <= R.G_SUMS / 4
    assert R.G >= R.G_FLOOR and R.G_WINO >= R.G_FLOOR and R.G_SUMS >= R.G_FLOOR
