"""Every 3x3-convolution form of csrc/conv3x3.hip at its dispatch edges, through the C ABI, against the float64 references of
tests/conv3_ref.py.

One call of gnx_conv3x3_bnrelu lands in one of nine kernel bodies - generic, the register-pipelined form with 5 / 6 / 7 / 9 strip
rows per thread, the persistent LDS-DMA form with 4 or 8 waves (dma4 / dma8) and the same in its data-gradient shape (dmag4 /
dmag8) - depending on M, N, K, S, the prologue, both leading dimensions and the alignment of A, Wr, scale and shift (DESIGN.md,
"conv2 forms").  gnx_conv3x3_winograd, gnx_conv3x3_dgrad_bnrelu_bwd and gnx_conv3x3_f16_dma / _h run persistent kernels of their
own shapes.  conv3_ref.GRID holds the smallest shapes at which each body and each edge between two exists; conv3_ref.form /
wino_form / adj_form / f16_form restate the dispatch, and each case first compares them with the gnx_*_form queries, so that a case
which silently lands in another body fails.

A (dY), the stored activation and the output are windows of larger sentinel-filled tensors with S + 17 sentinel rows above and
below, leading dimensions beyond the extent (a small excess or 1024), the output at a column offset of 1 or 3 floats with an
odd leading dimension; weights and per-channel vectors sit in sentinel frames; the adjoint's workspace is exactly the queried
number of floats plus a sentinel tail.  After a call the whole window is within the tolerance (a NaN or an infinity is a miss),
everything outside it and every input are bit-unchanged, and a second call gives the same bits (dbeta and dgamma included: their
reduction order is fixed).  The 8-wave cases (262144 rows) are compared on whole sampled images - the first and last two tiles,
both sides of every round boundary, 8 others - and held finite and bounded everywhere.

Tolerance, per element: |err| <= G 2^-24 T, T the sum of the term magnitudes (as Winograd forms them for gnx_conv3x3_winograd).
Every term is exactly 0 or at least 0.25, and each case asserts smallest non-zero term >= 4 x its largest tolerance: one
dropped, doubled or misplaced tap fails (conv3_ref's docstring has the two exceptions: the adjoint sums over many rows, the fp16
output - which is also held bit-equal to the rounded fp32 output).

G.  Plain fp32 evaluations of the reference operation were measured against float64 over every case of GRID as max |err| / (2^-24 T):
    fp32 F.conv2d on the device                         4.177   (64 maps of 64 x 64, K 64, N 32;  3.84 at one map of 48 x 48, K 8;  3.50 at
                                                                 one map of 79 x 79;  2.81 at the adjoint's data gradient, one map of 64 x 64)
    sequential fp32 multiply-add chain on the CPU       4.557   (adjoint, 9 maps of 64 x 64;  4.545 at fp16 operands, 2048 maps of 4 x 4,
                                                                 K 128;  4.530 at 256 maps of 32 x 32, K 32, N 64)
    fp32 F(2,3)-along-x emulation on the CPU            2.393   (4112 maps of 4 x 4, K 32;  2.00 at 2 maps of 64 x 64, K 64)
    adjoint sums: device conv2d + fp32 column sums      0.102   (8 maps of 4 x 4);  CPU chain + sequential sum over the rows 0.207 (2 maps of 8 x 8)
G = max(8, 4 x the largest), separately: direct forms 18.227 (conv3_ref.G), Winograd 9.570 (G_WINO), the adjoint sums 8 (G_SUMS, the
floor).  The kernels' own error had no part in it.  The measurements stay runnable: test_plain_fp32_conv2d_stays_within_the_ratio_G_was_set_from
here, the CPU ones in test_conv3_ref_host.py; each prints its figures.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv3_ref as R
from gridnext_amd import _lib as L
from test_gpu_bn_forms import Emb, Vec, P

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
H = torch.float16
OUT_SENTINEL, WS_SENTINEL, WS_TAIL = -4.0e30, 555.25, 64
BOUND = 1.0e6                                 # far above any result (at most 9 x 256 x 1.5 x 1.5 x 2.25), far below OUT_SENTINEL
WORST = {}                                    # body -> [worst |err| / tol, runs]
RAN = set()
UNSUPPORTED, BAD_ARG = L.ERR_UNSUPPORTED, -1
ALL_BODIES = set(R.BODIES) | {'wino', 'adj4', 'adj8', 'h4', 'h8'}


def ids(c):
    return '-'.join(str(v) for v in c)


# ----------------------------------------------------------------------------------------------------------- operands
class Win(Emb):
    """A window [pad : pad + M, off : off + C] of a [pad + M + pad][ld] tensor, everything else sentinel.  The window's first
    element lies `shift` elements off 16 B when `aligned` (the storage starts as many elements in as that takes)."""

    def __init__(self, val, M, C, ld, off, pad, sentinel, shift=0, dtype=torch.float32, aligned=True):
        per16 = 16 // torch.empty(0, dtype=dtype).element_size()
        self.M, self.C, self.ld, self.off, self.pad, self.rows = M, C, ld, off, pad, M + 2 * pad
        self.shift = shift + ((-(pad * ld + off)) % per16 if aligned else 0)
        self.flat = torch.full((self.rows * ld + 2 * per16,), float(sentinel), device=DEV, dtype=dtype)
        self.win = self._window(self.flat)
        if val is not None:
            self.win.copy_(val.to(DEV))
        self.before = self.flat.clone()
        self.ptr = self.win.data_ptr()
        assert self.flat.data_ptr() % 16 == 0 and (not aligned or self.ptr % 16 == shift * self.flat.element_size())

    def _window(self, flat):
        return flat[self.shift:self.shift + self.rows * self.ld].view(self.rows, self.ld)[self.pad:self.pad + self.M,
                                                                                         self.off:self.off + self.C]

    def outside_unchanged(self):
        a = self.flat.clone()
        self._window(a).copy_(self._window(self.before))
        return torch.equal(a, self.before)


class Flat:
    """`n` elements between two sentinel frames, `shift` elements off 16 B; val None: sentinel throughout."""

    def __init__(self, val, n, sentinel, shift=0, dtype=torch.float32, frame=64):
        self.n, self.lo = n, frame + shift
        self.buf = torch.full((n + 2 * frame + 8,), float(sentinel), device=DEV, dtype=dtype)
        if val is not None:
            self.buf[self.lo:self.lo + n] = val.reshape(-1).to(DEV)
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + self.buf.element_size() * self.lo
        assert self.ptr % 16 == shift * self.buf.element_size()

    def get(self):
        return self.buf[self.lo:self.lo + self.n].cpu()

    def unchanged(self):
        return torch.equal(self.buf, self.before)

    def outside_unchanged(self):
        return (torch.equal(self.buf[:self.lo], self.before[:self.lo])
                and torch.equal(self.buf[self.lo + self.n:], self.before[self.lo + self.n:]))


def chan(val, sentinel, shift=0):
    return Flat(val, val.numel(), sentinel, shift, frame=16)


def note(body, ratio):
    w = WORST.setdefault(body, [0.0, 0])
    w[0], w[1] = max(w[0], ratio), w[1] + 1


def ratio_of(what, got, ref, t):
    """The largest |err| / tolerance; a miss (a NaN or an infinity in `got` included) raises."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    miss = ~(err <= t)
    if miss.any():
        ratio = torch.where(miss, torch.nan_to_num(err / t, nan=float('inf')), torch.zeros_like(err))
        i = int(ratio.argmax())
        at = divmod(i, err.shape[-1]) if err.dim() == 2 else (i,)
        raise AssertionError("%s: %d of %d elements miss; worst |err| %.4e = %.3g x tolerance %.4e at %s (got %.9g, want %.9g)" % (
            what, int(miss.sum()), miss.numel(), err.flatten()[i].item(), ratio.max().item(), t.flatten()[i].item(), at,
            got.flatten()[i].item(), ref.flatten()[i].item()))
    live = t > 0
    return (err[live] / t[live]).max().item() if live.any() else 0.0


def window_rows(out, rows):
    """The window of `out` on the host; only `rows` of it when given - the rest is then held finite and bounded on the device."""
    if rows is None:
        return out.get()
    assert bool((out.win.float().abs() < BOUND).all()), 'a NaN, an infinity or an unwritten element in the window'
    return out.win[rows.to(DEV)].cpu()


def describe(c, f):
    s = 'case %s (%s, %d x %d workgroups, %d tiles' % (ids(c), f.body, f.G, f.gy, f.T)
    if hasattr(f, 'full'):
        s += ': %d full rounds + %d, xcd order %s' % (f.full, f.partial, f.xcd)
    return s + ')'


def query(name, *args):
    """(code, workgroups) of a gnx_*_form query."""
    w = ctypes.c_int(-7)
    rc = L.query(name, *args, ctypes.addressof(w))
    return rc, w.value


# ----------------------------------------------------------------------------------------------------------- gnx_conv3x3_bnrelu
class ConvOps:
    def __init__(self, c):
        lo, r, M = R.layout(c), R.recipe(c), R.rows(c)
        self.c, self.lo, self.M = c, lo, M
        self.A = Win(r.X, M, c.K, lo.lda, lo.a_off, lo.pad, 1234.5, lo.a_shift)
        self.Wr = Flat(R.repack(r.W), 9 * c.N * c.K, -77.5, lo.w_shift)
        self.scale = chan(r.scale, 88.25, lo.ss_shift) if c.act else None
        self.shift = chan(r.shift, -99.75, lo.ss_shift) if c.act else None
        assert (self.A.ptr % 16 != 0) == (c.lay == 'ash') and (lo.lda % 4 != 0) == (c.lay == 'aodd') and lo.lda > c.K
        assert (self.Wr.ptr % 16 != 0) == (c.lay == 'wsh') and lo.ldc % 2 == 1 and lo.ldc > c.N

    def out(self):
        return Win(None, self.M, self.c.N, self.lo.ldc, self.lo.c_off, self.lo.pad, OUT_SENTINEL, aligned=False)

    def args(self, out, **kw):
        c = self.c
        p = dict(A=self.A.ptr, lda=self.lo.lda, Wr=self.Wr.ptr, out=out.ptr, ldc=self.lo.ldc, M=self.M, N=c.N, K=c.K, S=c.S,
                 scale=P(self.scale), shift=P(self.shift))
        p.update(kw)
        return [p[k] for k in ('A', 'lda', 'Wr', 'out', 'ldc', 'M', 'N', 'K', 'S', 'scale', 'shift')]

    def inputs_unchanged(self):
        return all(o is None or o.unchanged() for o in (self.A, self.Wr, self.scale, self.shift))


def run_conv(c):
    o = ConvOps(c)
    f = R.form_of(c)
    what = describe(c, f)
    out = o.out()
    code, wgs = query('gnx_conv3x3_form', *o.args(out))
    assert (code, wgs) == (R.CODES[f.body], f.G), '%s: gnx_conv3x3_form says code %d, %d workgroups' % (what, code, wgs)
    L.call('gnx_conv3x3_bnrelu', *o.args(out), L.stream())
    torch.cuda.synchronize()
    assert o.inputs_unchanged(), what + ': an input was written'
    assert out.outside_unchanged(), what + ': wrote outside the window'
    ref = R.reference(c)
    t = R.tol(ref.T)
    assert R.detectable(ref.term, t), what + ': the smallest non-zero term is below 4 tolerances'
    note(f.body, ratio_of(what, window_rows(out, ref.rows), ref.ref, t))
    again = o.out()
    L.call('gnx_conv3x3_bnrelu', *o.args(again), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(again.flat, out.flat), what + ': a second call gives other bits'
    RAN.add(c)


SMALL_CONV = [c for c in R.CONV_GRID if not R.is_huge(c)]
HUGE_CONV = [c for c in R.CONV_GRID if R.is_huge(c)]


@pytest.mark.parametrize("c", SMALL_CONV, ids=ids)
def test_conv_grid(c):
    run_conv(c)


def test_conv_grid_at_262144_rows():
    """The 8-wave forms and the 4-wave cases beside them: every case of 64 MB in one test."""
    assert {R.form_of(c).body for c in HUGE_CONV} == {'dma8', 'dma4', 'dmag8'}
    failed = []
    for c in HUGE_CONV:
        try:
            run_conv(c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)


def test_conv_refusals_write_nothing():
    c = R.conv(2, 8, 8, 32, 1)
    o = ConvOps(c)
    big = R.conv(1, R.MAX_S + 1, 4, 4)
    runs = [(dict(lda=c.K - 1), BAD_ARG), (dict(ldc=c.N - 1), BAD_ARG), (dict(scale=None), BAD_ARG), (dict(shift=None), BAD_ARG),
            (dict(M=R.rows(c) - 1), BAD_ARG), (dict(A=None), BAD_ARG), (dict(Wr=None), BAD_ARG), (dict(K=0), BAD_ARG),
            (dict(S=big.S, M=R.rows(big)), UNSUPPORTED)]
    assert R.form_of(big).body is None and R.form_of(R.conv(1, R.MAX_S, 4, 4)).body == 'generic'
    for kw, code in runs:
        out = o.out()
        assert query('gnx_conv3x3_form', *o.args(out, **kw)) == (code, 0), kw
        assert L.query('gnx_conv3x3_bnrelu', *o.args(out, **kw), L.stream()) == code, kw
        torch.cuda.synchronize()
        assert out.unchanged() and o.inputs_unchanged(), kw
    out = o.out()
    assert query('gnx_conv3x3_form', *o.args(out, M=0)) == (R.CODES['generic'], 0)
    assert L.query('gnx_conv3x3_bnrelu', *o.args(out, M=0), L.stream()) == 0
    torch.cuda.synchronize()
    assert out.unchanged()


# ----------------------------------------------------------------------------------------------------------- gnx_conv3x3_winograd
class WinoOps:
    def __init__(self, c):
        lo, r, M = R.layout(c), R.recipe(c), R.rows(c)
        self.c, self.lo, self.M = c, lo, M
        self.A = Win(r.X, M, c.K, lo.lda, lo.a_off, lo.pad, 1234.5)
        self.Wu = Flat(R.winograd_weights(r.W), 12 * c.N * c.K, -77.5)

    def out(self):
        return Win(None, self.M, self.c.N, self.lo.ldc, self.lo.c_off, self.lo.pad, OUT_SENTINEL, aligned=False)

    def args(self, out, **kw):
        c = self.c
        p = dict(A=self.A.ptr, lda=self.lo.lda, Wu=self.Wu.ptr, out=out.ptr, ldc=self.lo.ldc, M=self.M, N=c.N, K=c.K, S=c.S)
        p.update(kw)
        return [p[k] for k in ('A', 'lda', 'Wu', 'out', 'ldc', 'M', 'N', 'K', 'S')]


@pytest.mark.parametrize("c", R.WINO_GRID, ids=ids)
def test_winograd_grid(c):
    o = WinoOps(c)
    f = R.form_of(c)
    what = describe(c, f) + ' ragged %d' % f.ragged
    out = o.out()
    assert query('gnx_conv3x3_winograd_form', *o.args(out)) == (R.CODES['wino'], f.G), what
    L.call('gnx_conv3x3_winograd', *o.args(out), L.stream())
    torch.cuda.synchronize()
    assert o.A.unchanged() and o.Wu.unchanged(), what + ': an input was written'
    assert out.outside_unchanged(), what + ': wrote outside the window'
    ref = R.reference(c)
    t = R.tol(ref.T, R.G_WINO)
    assert R.detectable(ref.term, t), what + ': the smallest non-zero term is below 4 tolerances'
    note('wino', ratio_of(what, out.get(), ref.ref, t))
    again = o.out()
    L.call('gnx_conv3x3_winograd', *o.args(again), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(again.flat, out.flat), what + ': a second call gives other bits'
    RAN.add(c)


def test_winograd_refusals_write_nothing():
    c = R.wino(2, 8, 32, big=1)
    o = WinoOps(c)
    c7 = R.wino(3, 7, 32)
    runs = [dict(N=64), dict(N=31), dict(K=48), dict(K=16), dict(lda=o.lo.lda + 1), dict(A=o.A.ptr + 4), dict(Wu=o.Wu.ptr + 4),
            dict(S=7, M=R.rows(c7)), dict(lda=(1 << 31) // R.rows(c) + 4), dict(ldc=(1 << 31) // R.rows(c) + 4)]
    for kw in runs:
        out = o.out()
        assert query('gnx_conv3x3_winograd_form', *o.args(out, **kw)) == (UNSUPPORTED, 0), kw
        assert L.query('gnx_conv3x3_winograd', *o.args(out, **kw), L.stream()) == UNSUPPORTED, kw
        torch.cuda.synchronize()
        assert out.unchanged() and o.A.unchanged() and o.Wu.unchanged(), kw
    out = o.out()
    assert L.query('gnx_conv3x3_winograd', *o.args(out, M=R.rows(c) + 1), L.stream()) == BAD_ARG
    assert query('gnx_conv3x3_winograd_form', *o.args(out, M=0, S=7)) == (R.CODES['wino'], 0)
    assert L.query('gnx_conv3x3_winograd', *o.args(out, M=0, S=7), L.stream()) == 0
    torch.cuda.synchronize()
    assert out.unchanged()


RELAYOUTS = {'gnx_repack_conv3x3': (R.repack, 9), 'gnx_repack_conv3x3_bwd': (R.repack_bwd, 9),
             'gnx_winograd_conv3x3_weights': (R.winograd_weights, 12)}


@pytest.mark.parametrize("N,K", [(5, 7), (32, 96), (33, 130)])
@pytest.mark.parametrize("name", sorted(RELAYOUTS))
def test_weight_transforms_equal_their_formulas_bit_for_bit(name, N, K):
    """Against the same formula evaluated in float32 on the host; (5, 7): less than one block, (33, 130): no multiple of 256."""
    formula, per = RELAYOUTS[name]
    g = torch.Generator().manual_seed(N * K)
    W = R._signed(g, 0.5, 1.5, N, K, 3, 3)
    src, dst = Flat(W, W.numel(), 1234.5), Flat(None, per * N * K, OUT_SENTINEL)
    L.call(name, src.ptr, dst.ptr, N, K, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(dst.get(), formula(W).reshape(-1)) and dst.outside_unchanged() and src.unchanged()


# ----------------------------------------------------------------------------------------------------------- the fused adjoint
ADJ_FLAGS = ((0, 1, 1), (1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 0, 0))            # (accumulate, dgamma wanted, dbeta wanted)


class AdjOps:
    def __init__(self, c):
        lo, r, M = R.layout(c), R.recipe(c), R.rows(c)
        self.c, self.lo, self.M, self.r = c, lo, M, r
        self.dY = Win(r.X, M, c.K, lo.lda, lo.a_off, lo.pad, 1234.5)
        self.Wb = Flat(R.repack_bwd(r.W), 9 * c.N * c.K, -77.5)
        self.act = Win(r.act, M, c.N, lo.ld_act, lo.act_off, lo.pad, -4321.5)
        self.vecs = [chan(v, 88.25 + i) for i, v in enumerate((r.scale, r.shift, r.mean, r.invstd))]
        self.nws = L.query('gnx_conv3x3_dgrad_bn_workspace', M, c.N)
        assert lo.lda > c.K and lo.ld_act > c.N and lo.ldc > c.N

    def out(self):
        return Win(None, self.M, self.c.N, self.lo.ldc, self.lo.c_off, self.lo.pad, OUT_SENTINEL, aligned=False)

    def space(self):
        ws = torch.full((self.nws + WS_TAIL,), float('nan'), device=DEV)
        ws[self.nws:] = WS_SENTINEL
        return ws

    def sums(self, acc, want_g, want_b):
        mk = lambda v0, want: Vec(v0 if acc else None, self.c.N, 31.5) if want else None      # noqa: E731
        return mk(self.r.dgamma0, want_g), mk(self.r.dbeta0, want_b)

    def args(self, dX, dg, db, acc, ws, **kw):
        c = self.c
        p = dict(dY=self.dY.ptr, lddy=self.lo.lda, Wb=self.Wb.ptr, act=self.act.ptr, lda=self.lo.ld_act, dX=dX.ptr, lddx=self.lo.ldc,
                 M=self.M, N=c.N, K=c.K, S=c.S, ws=None if ws is None else ws.data_ptr())
        p.update(kw)
        v = [x.ptr for x in self.vecs]
        return [p[k] for k in ('dY', 'lddy', 'Wb', 'act', 'lda', 'dX', 'lddx', 'M', 'N', 'K', 'S')] + v + [P(dg), P(db), acc, p['ws']]

    def form_args(self, dX, ws, **kw):
        a = self.args(dX, None, None, 0, ws, **kw)
        return a[:15] + [a[18]]

    def inputs_unchanged(self):
        return all(o.unchanged() for o in [self.dY, self.Wb, self.act] + self.vecs)


def run_adj(c):
    o = AdjOps(c)
    f = R.form_of(c)
    what = describe(c, f)
    assert o.nws >= f.G * f.waves * 2 * c.N
    first = None
    for acc, want_g, want_b in ADJ_FLAGS:
        w = '%s accumulate %d dgamma %d dbeta %d' % (what, acc, want_g, want_b)
        ref = R.adjoint(c, acc)
        for rep in range(2):
            dX, ws = o.out(), o.space()
            dg, db = o.sums(acc, want_g, want_b)
            assert query('gnx_conv3x3_dgrad_bnrelu_bwd_form', *o.form_args(dX, ws)) == (f.waves, f.G), w
            L.call('gnx_conv3x3_dgrad_bnrelu_bwd', *o.args(dX, dg, db, acc, ws), L.stream())
            torch.cuda.synchronize()
            assert o.inputs_unchanged(), w + ': an input was written'
            assert dX.outside_unchanged(), w + ': wrote outside dX'
            assert bool((ws[o.nws:] == WS_SENTINEL).all()), w + ': wrote past the workspace'
            assert all(v is None or v.tail_unchanged() for v in (dg, db)), w + ': wrote past dgamma / dbeta'
            got = (dX.flat.clone(), None if dg is None else dg.get(), None if db is None else db.get())
            if rep == 0:
                t = R.tol(ref.T_dX)
                assert R.detectable(ref.term, t), w + ': the smallest non-zero term of dX is below 4 tolerances'
                note(f.body, ratio_of(w + ' dX', window_rows(dX, ref.rows), ref.dX, t))
                for name, v, want, T in (('dgamma', dg, ref.dgamma, ref.T_dgamma), ('dbeta', db, ref.dbeta, ref.T_dbeta)):
                    if v is not None:
                        ts = R.tol(T, R.G_SUMS)
                        if o.M <= R.ADJ_SUMS_DETECT_ROWS:
                            assert R.detectable(ref.sum_term, ts), w + ': the smallest term of %s is below 4 tolerances' % name
                        note(f.body + ' sums', ratio_of(w + ' ' + name, v.get(), want, ts))
                if first is None:
                    first = got[0]
                assert torch.equal(got[0], first), w + ': dX differs from the first run of the case'
                one = got
            else:
                assert torch.equal(got[0], one[0]) and all(a is None or torch.equal(a, b) for a, b in zip(got[1:], one[1:])), \
                    w + ': a second call gives other bits'
    RAN.add(c)


@pytest.mark.parametrize("c", [c for c in R.ADJ_GRID if not R.is_huge(c)], ids=ids)
def test_fused_adjoint_grid(c):
    run_adj(c)


def test_fused_adjoint_at_262144_rows():
    huge = [c for c in R.ADJ_GRID if R.is_huge(c)]
    assert [R.form_of(c).body for c in huge] == ['adj8']
    run_adj(huge[0])


def test_fused_adjoint_refusals_write_nothing():
    c = R.adj(9, 4, big=1)
    o = AdjOps(c)
    runs = [(dict(K=64), UNSUPPORTED), (dict(K=16), UNSUPPORTED), (dict(N=64), UNSUPPORTED), (dict(M=128 + 16), UNSUPPORTED),
            (dict(lddy=o.lo.lda + 1), UNSUPPORTED), (dict(dY=o.dY.ptr + 4), UNSUPPORTED), (dict(Wb=o.Wb.ptr + 4), UNSUPPORTED),
            (dict(S=7, M=128 * 49), UNSUPPORTED), (dict(lddx=127, M=128), BAD_ARG), (dict(lda=127, M=128), BAD_ARG),
            (dict(no_ws=1, M=128), BAD_ARG), (dict(M=128 + 1), BAD_ARG)]
    for kw, code in runs:
        dX, ws = o.out(), o.space()
        dg, db = o.sums(0, 1, 1)
        kw = dict(kw)
        kw.setdefault('M', 128)
        passed = None if kw.pop('no_ws', 0) else ws                           # a NULL workspace
        assert query('gnx_conv3x3_dgrad_bnrelu_bwd_form', *o.form_args(dX, passed, **kw)) == (code, 0), kw
        assert L.query('gnx_conv3x3_dgrad_bnrelu_bwd', *o.args(dX, dg, db, 0, passed, **kw), L.stream()) == code, kw
        torch.cuda.synchronize()
        assert dX.unchanged() and dg.unchanged() and db.unchanged() and o.inputs_unchanged(), kw
        assert bool(torch.isnan(ws[:o.nws]).all()) and bool((ws[o.nws:] == WS_SENTINEL).all()), kw


# ----------------------------------------------------------------------------------------------------------- fp16 operands
class HalfOps:
    def __init__(self, c):
        lo, r, M = R.layout(c), R.recipe(c), R.rows(c)
        self.c, self.lo, self.M = c, lo, M
        self.A = Win(r.X.half(), M, c.K, lo.lda, lo.a_off, lo.pad, 1234.0, dtype=H)
        self.Wr = Flat(R.repack(r.W).half(), 9 * c.N * c.K, -77.5, dtype=H)
        assert lo.lda % 8 == 0 and lo.lda > c.K and self.A.ptr % 16 == 0 and self.Wr.ptr % 16 == 0
        assert torch.equal(r.X.half().float(), r.X) and torch.equal(r.W.half().float(), r.W)       # the recipe is fp16-exact

    def out(self, half):
        return Win(None, self.M, self.c.N, self.lo.ldc, self.lo.c_off, self.lo.pad, -60000.0 if half else OUT_SENTINEL,
                   dtype=H if half else torch.float32, aligned=False)

    def args(self, out, **kw):
        c = self.c
        p = dict(A=self.A.ptr, lda=self.lo.lda, Wr=self.Wr.ptr, out=out.ptr, ldc=self.lo.ldc, M=self.M, N=c.N, K=c.K, S=c.S)
        p.update(kw)
        return [p[k] for k in ('A', 'lda', 'Wr', 'out', 'ldc', 'M', 'N', 'K', 'S')]


def run_f16(c):
    o = HalfOps(c)
    f = R.form_of(c)
    what = describe(c, f) + (' resident weights' if f.resident else '')
    ref = R.reference(c)
    t = R.tol(ref.T)
    assert R.detectable(ref.term, t), what + ': the smallest non-zero term is below 4 tolerances'
    o32 = o.out(False)
    assert query('gnx_conv3x3_f16_dma_form', *o.args(o32)) == (f.waves, f.G), what
    L.call('gnx_conv3x3_f16_dma', *o.args(o32), L.stream())
    torch.cuda.synchronize()
    assert o.A.unchanged() and o.Wr.unchanged(), what + ': an input was written'
    assert o32.outside_unchanged(), what + ': wrote outside the window'
    note(f.body, ratio_of(what, window_rows(o32, ref.rows), ref.ref, t))
    outs = [(o32, 'gnx_conv3x3_f16_dma', False)]
    if c.op == 'h16':
        o16 = o.out(True)
        assert query('gnx_conv3x3_f16_dma_form', *o.args(o16)) == (f.waves, f.G), what
        L.call('gnx_conv3x3_f16_dma_h', *o.args(o16), L.stream())
        torch.cuda.synchronize()
        assert o.A.unchanged() and o.Wr.unchanged() and o16.outside_unchanged(), what + ': fp16 output: wrote outside the window'
        note(f.body + ' fp16 out', ratio_of(what + ' fp16 out', window_rows(o16, ref.rows), ref.ref,
                                            t + R.half_ulp16(ref.ref.abs() + t)))
        assert torch.equal(o16.win, o32.win.half()), what + ': the fp16 output is not the fp32 output rounded once'
        outs.append((o16, 'gnx_conv3x3_f16_dma_h', True))
    for first, name, half in outs:
        again = o.out(half)
        L.call(name, *o.args(again), L.stream())
        torch.cuda.synchronize()
        assert torch.equal(again.flat, first.flat), what + ': a second call of %s gives other bits' % name
    RAN.add(c)


@pytest.mark.parametrize("c", [c for c in R.F16_GRID if not R.is_huge(c)], ids=ids)
def test_f16_grid(c):
    run_f16(c)


def test_f16_grid_at_262144_rows():
    huge = [c for c in R.F16_GRID if R.is_huge(c)]
    assert {R.form_of(c).body for c in huge} == {'h8'} and {c.op for c in huge} == {'h32', 'h16'}
    failed = []
    for c in huge:
        try:
            run_f16(c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)


def test_f16_refusals_write_nothing():
    c = R.f16(8, 4, 128)
    o = HalfOps(c)
    runs = [dict(lda=o.lo.lda + 4), dict(K=64), dict(N=24), dict(M=128 + 16), dict(A=o.A.ptr + 8), dict(Wr=o.Wr.ptr + 8),
            dict(S=7, M=128 * 49)]
    for name, half in (('gnx_conv3x3_f16_dma', False), ('gnx_conv3x3_f16_dma_h', True)):
        for kw in runs:
            out = o.out(half)
            assert query('gnx_conv3x3_f16_dma_form', *o.args(out, **kw)) == (UNSUPPORTED, 0), kw
            assert L.query(name, *o.args(out, **kw), L.stream()) == UNSUPPORTED, (name, kw)
            torch.cuda.synchronize()
            assert out.unchanged() and o.A.unchanged() and o.Wr.unchanged(), (name, kw)


# ------------------------------------------------------------------------------------------------- where G comes from
DIRECT = [c for c in R.GRID if c.op != 'wino']
DEVICE_SEEN = {}


def _see(kind, ratio, c):
    if ratio > DEVICE_SEEN.get(kind, (-1.0, None))[0]:
        DEVICE_SEEN[kind] = (ratio, c)


def _device_conv(a, W, n, S):
    m = a.view(n, S, S, -1).permute(0, 3, 1, 2)
    return F.conv2d(m, W, padding=1).permute(0, 2, 3, 1).reshape(n * S * S, -1)


@pytest.mark.parametrize("c", DIRECT, ids=ids)
def test_plain_fp32_conv2d_stays_within_the_ratio_G_was_set_from(c, capsys):
    """The device half of the measurement behind conv3_ref.G and G_SUMS, kept runnable: the reference operation as fp32
    F.conv2d on the device (the prologue as one fp32 multiply-add and a max; the adjoint's mask, xhat and column sums in fp32)
    against the float64 reference, max |err| / (2^-24 T), held to G / 4.  A torch whose convolution rounds worse than that fails
    here with the figure to set TORCH_FP32_RATIO (and with it G) from."""
    r, ref = R.recipe(c), R.reference(c)
    X = (r.X if ref.rows is None else r.X[ref.rows]).to(DEV)
    a = torch.relu(torch.addcmul(r.shift.to(DEV), X, r.scale.to(DEV))) if c.act else X
    W = (R.dgrad_weight(r.W) if c.op == 'adj' else r.W).to(DEV)
    ratio = R.ratio(_device_conv(a, W, ref.n, c.S).cpu(), ref.ref, ref.T)
    _see('conv2d', ratio, c)
    with capsys.disabled():
        print(' torch fp32 conv2d ratio at %s: %.4f' % (ids(c), ratio))
    rs = 0.0
    if c.op == 'adj':
        o = R.adjoint(c)
        act, sc, sh, mu, inv = (v.to(DEV) for v in (r.act, r.scale, r.shift, r.mean, r.invstd))
        d = _device_conv(r.X.to(DEV), W, c.n, c.S) * (act > 0)
        xhat = ((act - sh) / sc - mu) * inv
        rs = max(R.ratio(d.sum(0).cpu(), o.dbeta, o.T_dbeta), R.ratio((d * xhat).sum(0).cpu(), o.dgamma, o.T_dgamma))
        _see('sums', rs, c)
        with capsys.disabled():
            print(' torch fp32 ratio of the adjoint sums at %s: %.4f' % (ids(c), rs))
    assert ratio <= R.G / 4 and rs <= R.G_SUMS / 4, (ratio, rs)


def test_report_worst_ratio_per_body(capsys):
    """Prints what the tests above saw: per kernel body the number of runs and the largest |err| / tolerance; after a run of
    the whole grid, every form the queries can return must have been reached."""
    with capsys.disabled():
        print('\n G = %.3f, G_WINO = %.3f, G_SUMS = %.3f (torch fp32 %.4f at %s; chain %.4f at %s; Winograd emulation %.4f at %s; '
              'sums: torch %.4f, chain %.4f)' % (R.G, R.G_WINO, R.G_SUMS, R.TORCH_FP32_RATIO, R.TORCH_FP32_AT, R.CHAIN_FP32_RATIO,
                                                 R.CHAIN_FP32_AT, R.WINO_FP32_RATIO, R.WINO_FP32_AT, R.TORCH_FP32_SUM_RATIO,
                                                 R.CHAIN_FP32_SUM_RATIO))
        for kind, (ratio, c) in sorted(DEVICE_SEEN.items()):
            print(' largest torch fp32 %s ratio %.4f at %s' % (kind, ratio, ids(c)))
        for body, (worst, n) in sorted(WORST.items()):
            print(' %-16s %4d runs, worst |err| / tolerance %.4f' % (body, n, worst))
    assert all(w <= 1.0 for w, _ in WORST.values())
    assert R.TORCH_FP32_RATIO <= R.G / 4 and R.TORCH_FP32_SUM_RATIO <= R.G_SUMS / 4
    if RAN >= set(R.GRID):
        assert ALL_BODIES <= set(WORST), 'never reached: %s' % sorted(ALL_BODIES - set(WORST))
