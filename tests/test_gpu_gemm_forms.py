"""Every kernel form of csrc/gemm_f32.hip at its dispatch edges, through the C ABI, against the float64 reference tests/gemm_ref.py.

One call of gnx_gemm_f32 / gnx_gemm_f32_ws lands in one of four kernel bodies - wide (256 x 128 tiles, K split, slab reduce),
big (128 x 64), the 64 x 64 body with the tall K split over gridDim.z, the 64 x 64 body plain - and, within a body, in one of
four layout pairs and (64 x 64 body) four loader pairs, depending on M, N, K, both leading dimensions, both pointers' alignment
and whether a workspace was passed ("GEMM forms").  gemm_ref.GRID holds the smallest shapes at which each form and
each edge between two exists; gemm_ref.form restates the dispatch, and each case first compares it with gnx_gemm_f32_form (body,
workgroups, splits, loader pair), so that a case which silently lands in another body fails, and checks it against
gnx_gemm_f32_workspace.

A, B and C are windows of larger tensors filled with a sentinel of their own, with leading dimensions beyond the extent; bias
has a sentinel tail, the workspace is exactly gnx_gemm_f32_workspace floats plus a sentinel tail.  After a call C is within the
tolerance everywhere (a NaN or an infinity is a miss) and everything outside C's window, the workspace's tail and every input
are bit-unchanged; a second call gives the same bits.

Tolerance, per element: |err_mn| <= G 2^-24 T_mn, T = |A| |B|^T + |bias| + |C0|.  Every operand has a magnitude in [0.5, 1.5],
so every product term is at least 0.25, and each case asserts 0.25 >= 4 x its largest tolerance: one dropped, doubled or
misplaced K term fails.

G.  Two plain fp32 evaluations were measured against the float64 product over every shape of GRID, as max |err| / (2^-24 T):
    torch.matmul on the device (fp32)                   5.958   (2048 x 512 x 1280;  4.65 at 2048 x 257 x 512, 4.10 at 4992 x 500 x 2000)
    sequential fp32 multiply-add chain on the CPU       3.642   (64 x 65 x 64;  3.59 at 63 x 130 x 65, 2.97 at 2048 x 256 x 36)
G = max(8, 4 x 5.9579) = 23.83 (gemm_ref.G).  The kernels' own error had no part in it.  Both measurements stay runnable:
test_plain_fp32_matmul_stays_within_the_ratio_G_was_set_from here, the chain in test_gemm_ref_host.py; each prints its figures.
"""
import ctypes
import functools

import pytest
import torch

import bn_ref
import gemm_ref as R
from gridnext_amd import _lib as L
from gridnext_amd import functional as GF
from test_gpu_bn_forms import Emb, Vec, P

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WS_TAIL, WS_SENTINEL = 64, 555.25
WORST = {}                                   # (body, a_kmajor, b_kmajor, a_vec, b_vec) -> [worst |err| / tol, cases]


# ----------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=2)
def _parts(shape):
    r = R.recipe_of(shape)
    return R.product(r.A, r.B)


def reference(shape, bias, acc, rows=None):
    """(ref, tol) of one case, float64; `rows`: only those rows (the matmuls are then not cached)."""
    r = R.recipe_of(shape)
    if rows is None:
        ref, T = R.product(None, None, r.bias if bias else None, r.C0 if acc else None, parts=_parts(shape))
    else:
        ref, T = R.product(r.A[rows], r.B, r.bias if bias else None, r.C0[rows] if acc else None)
    t = R.tol(T)
    assert R.detectable(t), 'the smallest product term is below 4 tolerances at %s' % (shape,)
    return ref, t


class Operands:
    """A and B of a case on the device, as windows of sentinel-filled tensors in the case's layouts."""

    def __init__(self, c, r=None):
        r = R.recipe_of((c.M, c.N, c.K)) if r is None else r
        self.c = c
        lda, offa, sha = R.lay(c.alay, c.M if c.ak else c.K)
        ldb, offb, shb = R.lay(c.blay, c.N if c.bk else c.K)
        self.A = Emb(r.A.t() if c.ak else r.A, c.K if c.ak else c.M, c.M if c.ak else c.K, lda, offa, 1234.5, sha)
        self.B = Emb(r.B.t() if c.bk else r.B, c.K if c.bk else c.N, c.N if c.bk else c.K, ldb, offb, -4321.5, shb)
        self.bias = Vec(r.bias, c.N, 77.75) if c.bias else None
        self.C0 = r.C0.to(DEV) if c.acc else None
        assert (self.A.ptr % 16 != 0) == (c.alay == 'shifted') and (self.B.ptr % 16 != 0) == (c.blay == 'shifted')
        assert (lda % 4 != 0) == (c.alay == 'oddld') and (ldb % 4 != 0) == (c.blay == 'oddld')

    def inputs_unchanged(self):
        return self.A.unchanged() and self.B.unchanged() and (self.bias is None or self.bias.unchanged())


def workspace(M, N, K):
    nws = L.query('gnx_gemm_f32_workspace', M, N, K)
    assert nws == R.workspace_floats(M, N, K), 'gnx_gemm_f32_workspace(%d, %d, %d) = %d' % (M, N, K, nws)
    buf = torch.full((nws + WS_TAIL,), WS_SENTINEL, device=DEV)
    return buf, nws


def query(*args):
    """(code, workgroups, splits, a_vec, b_vec) of gnx_gemm_f32_form."""
    out = [ctypes.c_int(-7) for _ in range(4)]
    return (L.query('gnx_gemm_f32_form', *args, *[ctypes.addressof(v) for v in out]),) + tuple(v.value for v in out)


def form_said(c, M, args, wsp):
    """gnx_gemm_f32_form against gemm_ref.form for the call about to be made (wsp: the workspace pointer or None), so that a
    case cannot silently test another body, split count, grid or loader pair."""
    body, S, av, bv = R.form_of(c._replace(M=M, ws=int(wsp is not None)))
    want = (R.CODES[body], R.workgroups(M, c.N, c.K, body, S), S, int(av), int(bv))
    said = query(*args, wsp)
    assert said == want, 'case %s, %d rows: gnx_gemm_f32_form says %s, gemm_ref.form %s' % (c, M, said, want)


def gemm(o, M=None, ws='case'):
    """One call on the operands `o` (M: only the first M rows of the product); returns C's window on the host.  ws: 'case' -
    what the case says; None - gnx_gemm_f32_ws with a NULL workspace."""
    c = o.c
    M = c.M if M is None else M
    ldc = c.N + 7
    C = Emb(None if o.C0 is None else o.C0[:M], M, c.N, ldc, 3, -4242.5)
    args = [o.A.ptr, o.A.ld, c.ak, o.B.ptr, o.B.ld, c.bk, P(o.bias), C.ptr, ldc, M, c.N, c.K, c.acc]
    buf = None
    if ws is None:
        form_said(c, M, args, None)
        L.call('gnx_gemm_f32_ws', *args, None, L.stream())
    elif c.ws:
        buf, nws = workspace(M, c.N, c.K)
        form_said(c, M, args, buf.data_ptr())
        L.call('gnx_gemm_f32_ws', *args, buf.data_ptr(), L.stream())
    else:
        form_said(c, M, args, None)
        L.call('gnx_gemm_f32', *args, L.stream())
    torch.cuda.synchronize()
    what = 'case %s' % (c,)
    assert o.inputs_unchanged(), what + ': an input was written'
    assert C.outside_unchanged(), what + ': C written outside its window'
    if buf is not None:
        assert bool((buf[nws:] == WS_SENTINEL).all()), what + ': wrote past the workspace'
        body, S, _, _ = R.form_of(c._replace(M=M))
        if S > 1:
            assert nws == S * M * c.N, what + ': form() says %d splits, the workspace is %d floats' % (S, nws)
        else:
            assert bool((buf == WS_SENTINEL).all()), what + ': an unsplit form wrote its workspace'
    return C.get()


def ratio_of(what, got, ref, t):
    """The largest |err| / tolerance; a miss (a NaN or an infinity in `got` included) raises."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    miss = ~(err <= t)
    if miss.any():
        ratio = torch.where(miss, torch.nan_to_num(err / t, nan=float('inf')), torch.zeros_like(err))
        i = int(ratio.argmax())
        raise AssertionError("%s: %d of %d elements miss; worst |err| %.4e = %.3g x tolerance %.4e at %s (got %.9g, want %.9g)" % (
            what, int(miss.sum()), miss.numel(), err.flatten()[i].item(), ratio.max().item(), t.flatten()[i].item(),
            divmod(i, err.shape[1]), got.flatten()[i].item(), ref.flatten()[i].item()))
    return (err / t).max().item()


def note(c, ratio):
    body, _, av, bv = R.form_of(c)
    w = WORST.setdefault((body, c.ak, c.bk, av, bv), [0.0, 0])
    w[0], w[1] = max(w[0], ratio), w[1] + 1


def run_case(c, o=None):
    """The case against float64, its sentinels, and a second call for the same bits.  Returns C."""
    o = Operands(c) if o is None else o
    ref, t = reference((c.M, c.N, c.K), c.bias, c.acc)
    got = gemm(o)
    note(c, ratio_of('case %s, form %s' % (c, R.form_of(c)), got, ref, t))
    assert torch.equal(got, gemm(o)), 'case %s: a second call gives other bits' % (c,)
    return got


# --------------------------------------------------------------------------------------------------- 1. the whole grid
def _cases_of(shape):
    return [c for c in R.GRID if (c.M, c.N, c.K) == shape]


@pytest.mark.parametrize("M,N,K", [s for s in R.SHAPES if s not in R.HUGE and s not in (R.PLAIN_VEC, R.TALL_VEC)])
def test_grid(M, N, K):
    failed = []                                                # every case of the shape runs: a failure names all that miss
    for c in _cases_of((M, N, K)):
        try:
            run_case(c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)


@pytest.mark.parametrize("shape", [R.PLAIN_VEC, R.TALL_VEC])
def test_scalar_and_vector_loaders_give_the_same_bits(shape):
    """The 64 x 64 body's loaders only fetch: the same values through 16-B buffer loads, through the scalar loader because the
    pointer is one float off, and through the scalar loader because the leading dimension is 1 mod 4, on either operand, feed the
    same MFMA chain.  All nine layout combinations of a layout pair must agree bit for bit (and each is checked against
    float64)."""
    failed, first = [], {}
    for c in _cases_of(shape):
        try:
            got = run_case(c)
            want = first.setdefault((c.ak, c.bk), got)
            assert torch.equal(got, want), 'case %s: bits differ from the aligned run' % (c,)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)
    assert len(first) == 4


def test_slab_workspace_cap():
    """gemm_tall_splits falls back to one split where s M N would pass 2^26 floats.  Both sides of that edge on one gigabyte of
    A: M = 174 762 (three splits, all of the 2^26-float workspace but 128 floats) and M = 174 763 (none).  float64 covers the
    first 64 rows, the last 64 and 64 seeded random ones."""
    below, above = [c for c in R.GRID if (c.M, c.N, c.K) in R.HUGE]
    assert (below.M, below.N, below.K) == R.CAP_BELOW and R.form_of(below)[:2] == ('tall', 3) and R.form_of(above)[:2] == ('plain', 1)
    o = Operands(above)
    for c in (above, below):
        o.c = c
        g = torch.Generator().manual_seed(c.M)
        rows = torch.cat([torch.arange(64), torch.arange(c.M - 64, c.M), torch.randint(64, c.M - 64, (64,), generator=g)])
        ref, t = reference((c.M, c.N, c.K), c.bias, c.acc, rows=rows)
        got = gemm(o)
        assert bool(torch.isfinite(got).all())
        note(c, ratio_of('case %s' % (c,), got[rows], ref, t))


# ------------------------------------------------------------------------- 2. bit-identities the source claims or implies
@pytest.mark.parametrize("ak", [0, 1])
@pytest.mark.parametrize("ws", [0, 1])
def test_a_rows_bits_do_not_depend_on_the_row_count(ak, ws):
    """The comment above gemm_tall_splits: for N <= 128 the split is a function of (N, K) only, "so that a row's result does not
    depend on how many rows the call has".  The composed 2000 -> 100 layer over 4992 spots against the same operands with
    4991, 130 and 1 rows (K-major A: those row counts are off 4, so the subset goes through the scalar loader as well)."""
    c = R.Case(4992, 100, 2000, ak, 0, 'aligned', 'aligned', 1, 0, ws)
    assert R.form_of(c)[:2] == (('tall', 3) if ws else ('plain', 1))
    o = Operands(c)
    full = gemm(o)
    ref, t = reference((c.M, c.N, c.K), c.bias, c.acc)
    note(c, ratio_of('case %s' % (c,), full, ref, t))
    for m in (4991, 130, 1):
        assert R.form_of(c._replace(M=m))[:2] == R.form_of(c)[:2]
        sub = gemm(o, M=m)
        assert torch.equal(sub, full[:m]), '%d rows of %d: the bits of a row depend on the row count' % (m, c.M)


@pytest.mark.parametrize("shape", [R.WIDE, R.EMPTY_SPLIT, R.BIG, R.TALL, R.PLAIN_VEC])
def test_null_workspace_is_the_entry_point_without_one(shape):
    for i, (ak, bk) in enumerate(R.PAIRS):
        bias, acc = R.FLAGS[i]
        c = R.Case(*shape, ak, bk, 'aligned', 'aligned', bias, acc, 0)
        o = Operands(c)
        ref, t = reference(shape, bias, acc)
        plain, null = gemm(o), gemm(o, ws=None)
        ratio_of('case %s' % (c,), plain, ref, t)
        assert torch.equal(plain, null), 'case %s: gnx_gemm_f32_ws(NULL) differs from gnx_gemm_f32' % (c,)


# --------------------------------------------------------------------------------------------------- 3. argument errors
def test_argument_errors_launch_nothing():
    M, N, K = 12, 8, 16
    r = R.recipe(M, N, K)
    A, At = Emb(r.A, M, K, K + 4, 0, 1234.5), Emb(r.A.t(), K, M, M + 4, 0, 1234.5)
    B, Bt = Emb(r.B, N, K, K + 4, 0, -4321.5), Emb(r.B.t(), K, N, N + 4, 0, -4321.5)
    bias, C = Vec(r.bias, N, 77.75), Emb(r.C0, M, N, N + 4, 0, -4242.5)
    ws = torch.full((WS_TAIL,), WS_SENTINEL, device=DEV)
    st = L.stream()

    def args(**kw):
        p = dict(A=A.ptr, lda=A.ld, ak=0, B=B.ptr, ldb=B.ld, bk=0, bias=bias.ptr, C=C.ptr, ldc=C.ld, M=M, N=N, K=K, acc=1)
        p.update(kw)
        return [p[k] for k in ('A', 'lda', 'ak', 'B', 'ldb', 'bk', 'bias', 'C', 'ldc', 'M', 'N', 'K', 'acc')]
    bad = [dict(A=None), dict(B=None), dict(C=None), dict(K=0), dict(K=-1), dict(M=-1), dict(N=-1), dict(ldc=N - 1),
           # a leading dimension below the operand's contiguous extent: K for a row-major operand, M resp. N for a K-major one
           dict(lda=K - 1), dict(ldb=K - 1), dict(lda=0), dict(ldb=0),
           dict(A=At.ptr, ak=1, lda=M - 1), dict(B=Bt.ptr, bk=1, ldb=N - 1), dict(lda=K - 1, N=0), dict(ldb=K - 1, M=0)]
    for kw in bad:
        for name, tail in (('gnx_gemm_f32', [st]), ('gnx_gemm_f32_ws', [ws.data_ptr(), st]), ('gnx_gemm_f32_ws', [None, st])):
            assert query(*args(**kw), tail[0] if len(tail) == 2 else None) == (R.BAD_ARG, 0, 0, 0, 0), kw
            with pytest.raises(RuntimeError, match='bad argument'):
                L.call(name, *args(**kw), *tail)
    # the extent itself is legal (K-major operands: M resp. N - smaller than K here), and an empty product is GNX_OK
    fine = [dict(M=0), dict(N=0), dict(M=0, N=0), dict(M=0, A=At.ptr, ak=1, lda=0)]
    for kw in fine:
        assert query(*args(**kw), ws.data_ptr())[:2] == (R.CODES['plain'], 0), kw               # nothing to launch
        L.call('gnx_gemm_f32', *args(**kw), st)
        L.call('gnx_gemm_f32_ws', *args(**kw), ws.data_ptr(), st)
    torch.cuda.synchronize()
    for v in (A, At, B, Bt, bias, C):
        assert v.unchanged()
    assert bool((ws == WS_SENTINEL).all())
    ref, T = R.product(r.A, r.B, r.bias, r.C0)
    for kw in (dict(A=At.ptr, ak=1, lda=At.ld, B=Bt.ptr, bk=1, ldb=Bt.ld), dict()):
        Ck = Emb(r.C0, M, N, N, 0, -4242.5)                   # ldc == N, and below: lda == M, ldb == N, the smallest legal
        L.call('gnx_gemm_f32', *args(C=Ck.ptr, ldc=N, **kw), st)
        torch.cuda.synchronize()
        ratio_of('smallest legal leading dimensions', Ck.get(), ref, R.tol(T))
        assert Ck.outside_unchanged()
    Am, Bm = Emb(r.A.t(), K, M, M, 0, 1234.5), Emb(r.B.t(), K, N, N, 0, -4321.5)
    Ck = Emb(r.C0, M, N, N, 0, -4242.5)
    L.call('gnx_gemm_f32', *args(A=Am.ptr, ak=1, lda=M, B=Bm.ptr, bk=1, ldb=N, C=Ck.ptr, ldc=N), st)
    torch.cuda.synchronize()
    ratio_of('lda == M, ldb == N', Ck.get(), ref, R.tol(T))
    assert Ck.outside_unchanged() and Am.unchanged() and Bm.unchanged()


# ------------------------------------------------------------------------------------------- 4. GF.linear, once per route
def _linear_check(x, w, b, dy, y):
    """y of GF.linear against float64 with the per-element gate (x [M][K], w [N][K], float64); returns dx's reference and gate."""
    ref, T = R.product(x, w, b)
    assert R.detectable(R.tol(T))
    ratio_of('linear y', y.detach().cpu(), ref, R.tol(T))
    ref, T = R.product(dy, w.t())                              # dx[M][K] = dy[M][N] w[N][K]
    return ref, R.tol(T)


def test_linear_rows_with_a_shifted_noncontiguous_x():
    M, N, K = 300, 36, 72
    r, d = R.recipe(M, N, K, seed=7), R.recipe(M, N, 1, seed=8)
    big = torch.full((M, K + 8), 1234.5, device=DEV)
    big[:, 1:1 + K] = r.A.float().to(DEV)
    x = big[:, 1:1 + K].requires_grad_(True)
    assert not x.is_contiguous() and x.data_ptr() % 16 == 4
    w, b = r.B.float().to(DEV).requires_grad_(True), r.bias.float().to(DEV).requires_grad_(True)
    dy = d.C0
    y = GF.linear(x, w, b)
    y.backward(dy.float().to(DEV))
    torch.cuda.synchronize()
    ref, t = _linear_check(r.A, r.B, r.bias, dy, y)
    ratio_of('linear dx', x.grad.cpu(), ref, t)
    ref, T = R.product(dy.t(), r.A.t())                        # dW[N][K] = dy^T[N][M] x[M][K]
    ratio_of('linear dW', w.grad.cpu(), ref, R.tol(T))
    ratio_of('linear db', b.grad.cpu()[None], dy.sum(0)[None], bn_ref.K * R.U * dy.abs().sum(0)[None])
    assert bool((big[:, 0] == 1234.5).all()) and bool((big[:, 1 + K:] == 1234.5).all())


def test_linear_kmajor_grid_off_four():
    """A K-major count grid [B][K][S] with S = 131: the rows of A are not 16-B apart, so both arrays - and the second one's
    `accumulate` call of dW - run the scalar loaders."""
    Bn, S, N, K = 2, 131, 20, 72
    M = Bn * S
    r, d = R.recipe(M, N, K, seed=9), R.recipe(M, N, 1, seed=10)
    xg = r.A.float().view(Bn, S, K).transpose(1, 2).contiguous().to(DEV).requires_grad_(True)          # [B][K][S]
    w, b = r.B.float().to(DEV).requires_grad_(True), r.bias.float().to(DEV).requires_grad_(True)
    dy = d.C0
    y = GF.linear(xg, w, b, kmajor=True)
    assert y.shape == (M, N)
    y.backward(dy.float().to(DEV))
    torch.cuda.synchronize()
    ref, t = _linear_check(r.A, r.B, r.bias, dy, y)
    ratio_of('linear dx', xg.grad.transpose(1, 2).reshape(M, K).cpu(), ref, t)
    ref, T = R.product(dy.t(), r.A.t())
    ratio_of('linear dW', w.grad.cpu(), ref, R.tol(T))
    ratio_of('linear db', b.grad.cpu()[None], dy.sum(0)[None], bn_ref.K * R.U * dy.abs().sum(0)[None])


def test_linear_backward_takes_an_expanded_gradient():
    """y.sum().backward() hands Linear(K, 1) a gradient [M][1] of stride 0: a leading dimension below the extent, which the
    entry points refuse - the rows are made contiguous first."""
    M, K = 70, 12
    r = R.recipe(M, 1, K, seed=11)
    x = r.A.float().to(DEV).requires_grad_(True)
    w, b = r.B.float().to(DEV).requires_grad_(True), r.bias.float().to(DEV).requires_grad_(True)
    GF.linear(x, w, b).sum().backward()
    torch.cuda.synchronize()
    one = torch.ones(M, 1, dtype=torch.float64)
    ref, T = R.product(one, r.B.t())
    ratio_of('dx', x.grad.cpu(), ref, R.tol(T))
    ref, T = R.product(one.t(), r.A.t())
    ratio_of('dW', w.grad.cpu(), ref, R.tol(T))
    assert abs(b.grad.item() - M) <= 1e-4


# ------------------------------------------------------------------------------------------------- where G comes from
@pytest.mark.parametrize("M,N,K", R.SHAPES)
def test_plain_fp32_matmul_stays_within_the_ratio_G_was_set_from(M, N, K, capsys):
    """The device half of the measurement behind gemm_ref.G, kept runnable: torch.matmul in fp32 on the device against the
    float64 product, max |err| / (2^-24 T), over every shape of GRID (the two shapes at the workspace cap: on 192 rows).  A torch
    whose GEMM rounds differently fails here with the figure to set TORCH_FP32_RATIO (and with it G) from."""
    shape = (M, N, K)
    r = R.recipe_of(shape)
    if shape in R.HUGE:
        rows = R.sample(M, 192)
        A = r.A[rows]
        ref, T = R.product(A, r.B)
    else:
        A = r.A
        ref, T = _parts(shape)
    got = torch.matmul(A.float().to(DEV), r.B.float().to(DEV).t()).cpu().double()
    ratio = ((got - ref).abs() / (R.U * T)).max().item()
    with capsys.disabled():
        print(' torch fp32 matmul ratio at %d x %d x %d: %.4f' % (M, N, K, ratio))
    assert ratio <= R.TORCH_FP32_RATIO, ratio


def test_report_worst_ratio_per_form(capsys):
    """Prints what the tests above saw: per kernel form the largest |err| / tolerance and the number of cases (empty when this
    test runs alone)."""
    with capsys.disabled():
        print('\n G = %.3f (torch fp32 matmul %.4f, fp32 chain %.4f)' % (R.G, R.TORCH_FP32_RATIO, R.CHAIN_FP32_RATIO))
        for (body, ak, bk, av, bv), (worst, n) in sorted(WORST.items()):
            print(' %-5s a_kmajor %d b_kmajor %d a_vec %d b_vec %d: worst |err| / tolerance %.4f over %d cases' % (
                body, ak, bk, av, bv, worst, n))
    assert all(w <= 1.0 for w, _ in WORST.values())
