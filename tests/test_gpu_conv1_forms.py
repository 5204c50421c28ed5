"""Every fp32 1x1-convolution form of csrc/conv1x1.hip and csrc/dgrad_wgrad_f32.hip at its dispatch edges, through the C ABI,
against the float64 references of tests/conv1_ref.py.

One call of conv1x1_launch (gnx_conv1x1_bnrelu, gnx_conv1x1_bnrelu_ws, gnx_conv1x1_bnrelu_act) lands in one of eight bodies -
conv1x1_kernel<pool, fast> in four combinations (generic, generic_vec, pool, pool_vec), the K-split launch with its reduction
(split), the persistent wave-specialised kernel without and with the prologue and with pooling producers (ws, ws_act, ws_pool) -
depending on M, N, K, both leading dimensions, the alignment of six pointers, S_in and the workspace ("conv1 forms").
gnx_conv1x1_dgrad_bnrelu_bwd runs the persistent kernel in its fused data-gradient shape, gnx_conv1x1_dgrad_wgrad_bnrelu_bwd a
launch over full 128-channel blocks and one over the 1 or 2 columns that are left (3 run as a full block with an idle wave).
conv1_ref.GRID holds the smallest shapes at which each body and each edge between two exists; conv1_ref.conv_form / dgbn_form /
dgwg_plan restate the dispatch, and each case first compares them with gnx_conv1x1_form, gnx_conv1x1_dgrad_bnrelu_bwd_form and
the workspace queries, so that a case which silently lands in another body fails.

Every operand is a window of a larger sentinel-filled tensor with sentinel rows above and below and a leading dimension beyond the
extent; the output lies at a column offset of 1 or 3 floats with an odd leading dimension (the split form takes an aligned one
only); weights and per-channel vectors sit in sentinel frames; a workspace is exactly the queried number of floats plus a sentinel
tail.  After a call the whole window is within the tolerance (a NaN or an infinity is a miss), everything outside it - the columns
of the in-place dX past N included - and every input are bit-unchanged, the workspace tail and the split slabs that are planned
but not launched keep the sentinel, and a second call gives the same bits (dgamma, dbeta and dW included: their reduction orders
are fixed).  Every refused call returns its code and writes nothing.

Tolerance, per element: |err| <= G 2^-24 T, T the sum of the term magnitudes (conv1_ref's docstring).  Every term is exactly 0 or
at least 0.25 (a quarter of that when pooled, half of it behind the output activation), and each case asserts smallest non-zero
term >= 4 x its largest tolerance: one dropped, doubled or misplaced term fails (the column sums over many rows are the exception
conv1_ref's docstring states).

G.  Plain fp32 evaluations of the reference operation were measured against float64 over every case of GRID as max |err| / (2^-24 T):
    products: fp32 torch on the device                  4.672   (65664 rows, N 32, K 32, no prologue;  4.24 at the one-pass gradient, 19232 rows, K 128;
                                                                 4.20 at the fused data gradient, 32896 rows, N 160, K 32)
    products: sequential fp32 chain on the CPU          4.396   (32896 rows, N 160, K 32, no prologue;  3.995 at dW of the one-pass gradient, 32992 rows, K 64)
    column sums: device product + fp32 column sums      0.344   (one-pass gradient, 32 rows, K 288;  0.284 at 32 rows, K 224)
    column sums: CPU chain + sequential sum             0.324   (one-pass gradient, 32 rows, K 288;  0.312 at the fused data gradient, 32896 rows, N 160, K 32)
G = max(8, 4 x the largest), separately: products 18.688 (conv1_ref.G), column sums 8, the floor (G_SUMS).  The kernels' own error had no
part in it.  The measurements stay runnable: test_plain_fp32_torch_stays_within_the_ratio_G_was_set_from here, the CPU one in
test_conv1_ref_host.py; each prints its figures.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv1_ref as R
from gridnext_amd import _lib as L
from test_gpu_bn_forms import Vec, P
from test_gpu_conv3_forms import Win, Flat, chan, ratio_of

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
OUT_SENTINEL, WS_SENTINEL, WS_TAIL = -4.0e30, 555.25, 64
WORST = {}                                    # body -> [worst |err| / tol, runs]
RAN = set()
ALL_BODIES = set(R.BODIES) | {'dgbn'} | set(R.DGWG_SHAPES)


def ids(c):
    return '-'.join(str(v) for v in c)


def note(body, ratio):
    w = WORST.setdefault(body, [0.0, 0])
    w[0], w[1] = max(w[0], ratio), w[1] + 1


def sel(ptr, name, kw):
    """An operand's pointer under the overrides of a refusal: NULL, or one float off 16 B."""
    if name in kw.get('null', ()):
        return None
    return ptr + 4 if ptr is not None and name in kw.get('mis', ()) else ptr


class Space:
    """A workspace of exactly `n` floats `shift` floats off 16 B, sentinel throughout, with a sentinel tail."""

    def __init__(self, n, shift=0):
        self.n, self.shift = n, shift
        self.buf = torch.full((n + WS_TAIL + 8,), WS_SENTINEL, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * shift
        assert self.buf.data_ptr() % 16 == 0

    def untouched_from(self, written):
        """Everything but the first `written` floats of the workspace keeps the sentinel."""
        b = self.buf
        return bool((b[:self.shift] == WS_SENTINEL).all()) and bool((b[self.shift + written:] == WS_SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------- conv1x1_launch
class ConvOps:
    def __init__(self, c):
        lo, r = R.layout(c), R.recipe(c)
        self.c, self.lo = c, lo
        self.A = Win(r.X, R.rows_in(c), c.K, lo.lda, lo.a_off, lo.pad, 1234.5, lo.a_shift)
        self.W = Flat(r.W, c.N * c.K, -77.5, lo.w_shift)
        self.scale = chan(r.scale, 88.25, lo.ss_shift) if c.act else None
        self.shift = chan(r.shift, -99.75, lo.ss_shift) if c.act else None
        self.oscale = chan(r.oscale, 66.25) if c.oact else None
        self.oshift = chan(r.oshift, -55.75) if c.oact else None
        self.nws = L.query('gnx_conv1x1_workspace', c.M, c.N, c.K)
        assert self.nws == (lambda s: s * c.M * c.N if s > 1 else 0)(R.small_splits(c.M, c.N, c.K))
        assert (self.A.ptr % 16 != 0) == (c.lay == 'ash') and (lo.lda % 4 != 0) == (c.lay == 'aodd') and lo.lda > c.K
        assert (self.W.ptr % 16 != 0) == (c.lay == 'wsh') and lo.ldc > c.N

    def out(self):
        o = Win(None, self.c.M, self.c.N, self.lo.ldc, self.lo.c_off, self.lo.pad, OUT_SENTINEL, aligned=self.lo.out_aligned)
        assert not self.lo.out_aligned or o.ptr % 16 == 0
        return o

    def space(self):
        return Space(self.nws, self.lo.ws_shift) if self.c.ws == 1 else None

    def _p(self, out, kw):
        c = self.c
        p = dict(A=self.A.ptr, lda=self.lo.lda, W=self.W.ptr, out=out.ptr, ldc=self.lo.ldc, M=c.M, N=c.N, K=c.K, pool=c.pool, S=c.S,
                 scale=P(self.scale), shift=P(self.shift), oscale=P(self.oscale), oshift=P(self.oshift))
        p.update({k: v for k, v in kw.items() if k in p})
        for name in ('A', 'W', 'out', 'scale', 'shift', 'oscale', 'oshift'):
            p[name] = sel(p[name], name, kw)
        return p

    def call_args(self, out, ws, **kw):
        """(entry point, its arguments) as the case (or the refusal's overrides) asks."""
        p = self._p(out, kw)
        head = [p[k] for k in ('A', 'lda', 'W', 'out', 'ldc', 'M', 'N', 'K', 'scale', 'shift')]
        if self.c.oact or kw.get('oact'):
            return 'gnx_conv1x1_bnrelu_act', head + [p['oscale'], p['oshift'], L.stream()]
        if self.c.ws:
            return 'gnx_conv1x1_bnrelu_ws', head + [P(ws), L.stream()]
        return 'gnx_conv1x1_bnrelu', head + [p['pool'], p['S'], L.stream()]

    def form(self, out, ws, **kw):
        """(code, workgroups, nz) of gnx_conv1x1_form for the same call."""
        p = self._p(out, kw)
        wg, nz = ctypes.c_int(-7), ctypes.c_int(-7)
        rc = L.query('gnx_conv1x1_form', *[p[k] for k in ('A', 'lda', 'W', 'out', 'ldc', 'M', 'N', 'K', 'scale', 'shift', 'pool', 'S',
                                                         'oscale', 'oshift')], P(ws), ctypes.addressof(wg), ctypes.addressof(nz))
        return rc, wg.value, nz.value

    def inputs_unchanged(self):
        return all(o is None or o.unchanged() for o in (self.A, self.W, self.scale, self.shift, self.oscale, self.oshift))


def describe(c, f):
    s = 'case %s (%s, %d x %d workgroups' % (ids(c), f.body, f.wgs, f.gy)
    if f.body == 'split':
        s += ', %d splits planned, %d launched' % (f.splits, f.nz)
    if f.T:
        s += ', %d tiles, %d column tiles: %d full rounds + %d, xcd map %s' % (f.T, f.tilesN, f.full, f.partial, f.jmap)
    return s + ')'


def run_conv(c):
    o = ConvOps(c)
    f = R.form_of(c)
    what = describe(c, f)
    out, ws = o.out(), o.space()
    got = o.form(out, ws)
    assert got == (f.code, f.wgs, f.nz), '%s: gnx_conv1x1_form says code %d, %d workgroups, %d splits' % ((what,) + got)
    assert L.query('gnx_conv1x1_form', o.A.ptr, o.lo.lda, o.W.ptr, out.ptr, o.lo.ldc, c.M, c.N, c.K, P(o.scale), P(o.shift), c.pool, c.S,
                   P(o.oscale), P(o.oshift), P(ws), None, None) == f.code, what + ': NULL out-pointers'
    name, args = o.call_args(out, ws)
    L.call(name, *args)
    torch.cuda.synchronize()
    assert o.inputs_unchanged(), what + ': an input was written'
    assert out.outside_unchanged(), what + ': wrote outside the window'
    if ws is not None:
        assert ws.untouched_from(f.nz * c.M * c.N), what + ': wrote past the launched slabs of the workspace'
    ref = R.reference(c)
    t = R.tol(ref.T)
    assert R.detectable(ref.term, t), what + ': the smallest non-zero term is below 4 tolerances'
    note(f.body, ratio_of(what, out.get(), ref.ref, t))
    again, ws2 = o.out(), o.space()
    name, args = o.call_args(again, ws2)
    L.call(name, *args)
    torch.cuda.synchronize()
    assert torch.equal(again.flat, out.flat), what + ': a second call gives other bits'
    RAN.add(c)


@pytest.mark.parametrize("c", R.CONV_GRID, ids=ids)
def test_conv_grid(c):
    run_conv(c)


def test_conv_form_beyond_32_bit_row_offsets_by_query_only():
    """4 M >= 2^31: the persistent kernel's int row offsets decline; nothing of that size is allocated or launched."""
    c = R.conv(128, 32, 32)
    o = ConvOps(c)
    out = o.out()
    for M in ((1 << 29) - 128, 1 << 29):
        f = R.conv_form(M, c.N, c.K, o.lo.lda, o.lo.ldc)
        assert o.form(out, None, M=M) == (f.code, f.wgs, 0), M
    assert R.conv_form(1 << 29, c.N, c.K, o.lo.lda, o.lo.ldc).body == 'generic_vec'


def test_conv_refusals_write_nothing():
    c = R.conv(128, 32, 32, 1, oact=1)                   # (the output vectors are passed where a refusal asks for the _act entry)
    o = ConvOps(c)
    o.c = R.conv(128, 32, 32)
    for kw, code in R.CONV_REFUSALS:
        out = o.out()
        fkw = dict(kw)
        if not kw.get('oact'):
            fkw['null'] = tuple(kw.get('null', ())) + ('oscale', 'oshift')
        assert o.form(out, None, **fkw) == (code, 0, 0), kw
        name, args = o.call_args(out, None, **kw)
        assert L.query(name, *args) == code, kw
        torch.cuda.synchronize()
        assert out.unchanged() and o.inputs_unchanged(), kw
    out = o.out()
    assert o.form(out, None, M=0, null=('oscale', 'oshift')) == (R.CODES['generic'], 0, 0)
    name, args = o.call_args(out, None, M=0)
    assert L.query(name, *args) == 0
    torch.cuda.synchronize()
    assert out.unchanged()


# ----------------------------------------------------------------------------------------------------------- the fused gradients
ADJ_FLAGS = ((0, 1, 1), (1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 0, 0))            # (accumulate, dgamma wanted, dbeta wanted)


class AdjOps:
    """The operands of a dgbn / dgwg case.  C = the channels in, B = the bottleneck's channels."""

    def __init__(self, c):
        lo, r = R.layout(c), R.recipe(c)
        self.c, self.lo, self.r = c, lo, r
        self.C, self.B = (c.N, c.K) if c.op == 'dgbn' else (c.K, 128)
        al = c.op == 'dgwg'
        self.dY = Win(r.dY, c.M, self.B, lo.lda, lo.a_off, lo.pad, 1234.5)
        self.Wt = Flat(r.Wt, self.C * self.B, -77.5)
        self.X = Win(r.X, c.M, self.C, lo.ldx, lo.x_off, lo.pad, -4321.5, aligned=al)
        self.vecs = [chan(v, 88.25 + i) for i, v in enumerate((r.scale, r.shift, r.mean, r.invstd))]
        if c.op == 'dgbn':
            self.nws = L.query('gnx_conv1x1_dgrad_bn_workspace', c.M, c.N)
            assert self.nws == R.dgbn_workspace(c.M, c.N)
        else:
            self.nws = L.query('gnx_conv1x1_dgrad_wgrad_workspace', c.M, c.K)
            assert self.nws == R.dgwg_plan(c.M, c.K).floats, 'the restated slab plan differs from the workspace query'
        assert lo.lda > self.B and lo.ldx > self.C and lo.ldc > self.C and lo.ldx != lo.ldc

    def dX(self):
        return Win(self.r.dX0, self.c.M, self.C, self.lo.ldc, self.lo.c_off, self.lo.pad, OUT_SENTINEL, aligned=self.c.op == 'dgwg')

    def sums(self, acc, want_g, want_b):
        mk = lambda v0, want: Vec(v0 if acc else None, self.C, 31.5) if want else None      # noqa: E731
        return mk(self.r.dgamma0, want_g), mk(self.r.dbeta0, want_b)

    def dW(self, acc):
        return Flat(self.r.dW0 if acc else None, 128 * self.C, 47.25)

    def args(self, dX, dg, db, acc, ws, dW=None, **kw):
        c = self.c
        p = dict(dY=self.dY.ptr, lddy=self.lo.lda, Wt=self.Wt.ptr, X=self.X.ptr, ldx=self.lo.ldx, dX=dX.ptr, lddx=self.lo.ldc, M=c.M,
                 N=c.N, K=c.K, ws=P(ws), dW=P(dW))
        p.update(dict(zip(('scale', 'shift', 'mean', 'invstd'), (v.ptr for v in self.vecs))))
        alias = dict(dB='dY', W1t='Wt', G='dX', lddb='lddy', ldg='lddx')
        kw = {k: (tuple(alias.get(n, n) for n in v) if k in ('null', 'mis') else v) for k, v in kw.items()}
        p.update({alias.get(k, k): v for k, v in kw.items() if alias.get(k, k) in p})
        for name in ('dY', 'Wt', 'X', 'dX', 'scale', 'shift', 'mean', 'invstd', 'ws', 'dW'):
            p[name] = sel(p[name], name, kw)
        v = [p[k] for k in ('scale', 'shift', 'mean', 'invstd')]
        if c.op == 'dgbn':
            return [p[k] for k in ('dY', 'lddy', 'Wt', 'X', 'ldx', 'dX', 'lddx', 'M', 'N', 'K')] + v + [P(dg), P(db), acc, p['ws']]
        return [p[k] for k in ('dY', 'lddy', 'Wt', 'X', 'ldx', 'dX', 'lddx', 'M', 'K')] + v + [P(dg), P(db), p['dW'], p['ws'], acc]

    def form(self, *a, **kw):
        w = ctypes.c_int(-7)
        rc = L.query('gnx_conv1x1_dgrad_bnrelu_bwd_form', *self.args(*a, **kw), ctypes.addressof(w))
        return rc, w.value

    def inputs_unchanged(self):
        return all(o.unchanged() for o in [self.dY, self.Wt, self.X] + self.vecs)


def run_adj(c):
    o = AdjOps(c)
    f = R.form_of(c)
    dg_case = c.op == 'dgbn'
    entry = 'gnx_conv1x1_dgrad_bnrelu_bwd' if dg_case else 'gnx_conv1x1_dgrad_wgrad_bnrelu_bwd'
    bodies = ['dgbn'] if dg_case else sorted(f.shapes)
    if dg_case:
        what = 'case %s (%d workgroups, %d tiles, %d column tiles, runs of %d .. %d)' % (ids(c), f.wgs, f.T, f.tilesN, f.runs[0], f.runs[1])
    else:
        p = R.dgwg_plan(c.M, c.K)
        what = 'case %s (%s: %d slabs of %d tiles, rest %d slabs of %d)' % (ids(c), ', '.join(bodies), p.slabs_full, p.per_full,
                                                                           p.slabs_rest, p.per_rest)
    first = None
    for acc, want_g, want_b in ADJ_FLAGS:
        w = '%s accumulate %d dgamma %d dbeta %d' % (what, acc, want_g, want_b)
        ref = R.adjoint(c, acc)
        for rep in range(2):
            dX, ws = o.dX(), Space(o.nws)
            dg, db = o.sums(acc, want_g, want_b)
            dW = None if dg_case else o.dW(acc)
            if dg_case:
                assert o.form(dX, dg, db, acc, ws) == (4, f.wgs), w
            L.call(entry, *o.args(dX, dg, db, acc, ws, dW), L.stream())
            torch.cuda.synchronize()
            assert o.inputs_unchanged(), w + ': an input was written'
            assert dX.outside_unchanged(), w + ': wrote outside dX (the columns past the channels in included)'
            assert ws.untouched_from(o.nws), w + ': wrote past the workspace'
            assert all(v is None or v.tail_unchanged() for v in (dg, db)), w + ': wrote past dgamma / dbeta'
            assert dW is None or dW.outside_unchanged(), w + ': wrote outside dW'
            got = (dX.flat.clone(), None if dg is None else dg.get(), None if db is None else db.get(), None if dW is None else dW.get())
            if rep == 0:
                t = R.tol(ref.T_dX)
                assert R.detectable(ref.term, t), w + ': the smallest non-zero term of dX is below 4 tolerances'
                worst = ratio_of(w + ' dX', dX.get(), ref.dX, t)
                for b in bodies:
                    note(b, worst)
                for name, v, want, T in (('dgamma', dg, ref.dgamma, ref.T_dgamma), ('dbeta', db, ref.dbeta, ref.T_dbeta)):
                    if v is not None:
                        ts = R.tol(T, R.G_SUMS)
                        if R.sums_detectable_case(c):
                            assert R.detectable(ref.sum_term, ts), w + ': the smallest term of %s is below 4 tolerances' % name
                        note(c.op + ' sums', ratio_of(w + ' ' + name, v.get(), want, ts))
                if dW is not None:
                    tw = R.tol(ref.T_dW)
                    if c.M <= R.DW_DETECT_ROWS:
                        assert R.detectable(ref.dw_term, tw), w + ': the smallest term of dW is below 4 tolerances'
                    note('dgwg dW', ratio_of(w + ' dW', dW.get().view(128, o.C), ref.dW, tw))
                if first is None:
                    first = got[0]
                assert torch.equal(got[0], first), w + ': dX differs from the first run of the case'
                one = got
            else:
                assert all(a is None or torch.equal(a, b) for a, b in zip(got, one)), w + ': a second call gives other bits'
    RAN.add(c)


@pytest.mark.parametrize("c", R.DGBN_GRID + R.DGWG_GRID, ids=ids)
def test_fused_gradient_grid(c):
    run_adj(c)


def _refused(o, entry, runs, with_form):
    for kw, code in runs:
        dX, ws = o.dX(), Space(o.nws)
        dg, db = o.sums(0, 1, 1)
        dW = None if o.c.op == 'dgbn' else o.dW(0)
        if with_form:
            assert o.form(dX, dg, db, 0, ws, **kw) == (code, 0), kw
        assert L.query(entry, *o.args(dX, dg, db, 0, ws, dW, **kw), L.stream()) == code, kw
        torch.cuda.synchronize()
        assert dX.unchanged() and dg.unchanged() and db.unchanged() and o.inputs_unchanged() and ws.untouched_from(0), kw
        assert dW is None or dW.unchanged(), kw


def test_fused_data_gradient_refusals_write_nothing():
    o = AdjOps(R.dgbn(128, 96))
    _refused(o, 'gnx_conv1x1_dgrad_bnrelu_bwd', R.DGBN_REFUSALS + [(dict(null=(n,)), R.BAD_ARG) for n in R.DGBN_NULLS], True)
    dX, ws = o.dX(), Space(o.nws)
    assert o.form(dX, None, None, 0, ws, M=0) == (4, 0)
    assert L.query('gnx_conv1x1_dgrad_bnrelu_bwd', *o.args(dX, None, None, 0, ws, M=0), L.stream()) == 0
    torch.cuda.synchronize()
    assert dX.unchanged() and ws.untouched_from(0)


def test_one_pass_gradient_refusals_write_nothing():
    o = AdjOps(R.dgwg(96, 64))
    _refused(o, 'gnx_conv1x1_dgrad_wgrad_bnrelu_bwd', R.DGWG_REFUSALS + [(dict(null=(n,)), R.BAD_ARG) for n in R.DGWG_NULLS], False)


# ------------------------------------------------------------------------------------------------- where G comes from
DEVICE_SEEN = {}


def _see(kind, ratio, c):
    if ratio > DEVICE_SEEN.get(kind, (-1.0, None))[0]:
        DEVICE_SEEN[kind] = (ratio, c)


@pytest.mark.parametrize("c", R.GRID, ids=ids)
def test_plain_fp32_torch_stays_within_the_ratio_G_was_set_from(c, capsys):
    """The device half of the measurement behind conv1_ref.G and G_SUMS, kept runnable: the reference operation in fp32 torch on
    the device (the prologue as one fp32 multiply-add and a max; a matmul, or F.conv2d + F.avg_pool2d for the pooled cases; the
    adjoints' mask, xhat and column sums in fp32) against the float64 reference, max |err| / (2^-24 T), held to G / 4.  A torch
    whose product rounds worse than that fails here with the figure to set TORCH_FP32_RATIO (and with it G) from."""
    r = R.recipe(c)
    d = lambda v: v.to(DEV)                                                    # noqa: E731
    rs = 0.0
    if c.op == 'conv':
        ref = R.reference(c)
        a = torch.relu(torch.addcmul(d(r.shift), d(r.X), d(r.scale))) if c.act else d(r.X)
        if c.pool:
            m = a.view(R.images(c), c.S, c.S, c.K).permute(0, 3, 1, 2)
            y = F.avg_pool2d(F.conv2d(m, d(r.W).view(c.N, c.K, 1, 1)), 2, 2).permute(0, 2, 3, 1).reshape(c.M, c.N)
        else:
            y = a @ d(r.W).t()
        if c.oact:
            y = torch.relu(torch.addcmul(d(r.oshift), y, d(r.oscale)))
        ratio = R.ratio(y.cpu(), ref.ref, ref.T)
    else:
        o = R.adjoint(c)
        X, sc = d(r.X), d(r.scale)
        pre = torch.addcmul(d(r.shift), X, sc)
        g = (d(r.dY) @ d(r.Wt).t()) * (pre > 0)
        ratio = R.ratio(torch.addcmul(d(r.dX0), g, sc).cpu(), o.dX, o.T_dX)
        if c.op == 'dgwg':
            ratio = max(ratio, R.ratio((d(r.dY).t() @ torch.relu(pre)).cpu(), o.dW, o.T_dW))
        xhat = (X - d(r.mean)) * d(r.invstd)
        rs = max(R.ratio(g.sum(0).cpu(), o.dbeta, o.T_dbeta), R.ratio((g * xhat).sum(0).cpu(), o.dgamma, o.T_dgamma))
        _see('sums', rs, c)
        with capsys.disabled():
            print(' torch fp32 ratio of the column sums at %s: %.4f' % (ids(c), rs))
    _see('products', ratio, c)
    with capsys.disabled():
        print(' torch fp32 ratio at %s: %.4f' % (ids(c), ratio))
    assert ratio <= R.G / 4 and rs <= R.G_SUMS / 4, (ratio, rs)


def test_report_worst_ratio_per_body(capsys):
    """Prints what the tests above saw: per kernel body the number of runs and the largest |err| / tolerance; after a run of
    the whole grid, every body must have been reached."""
    with capsys.disabled():
        print('\n G = %.3f, G_SUMS = %.3f (products: torch fp32 %.4f at %s; chain %.4f at %s; sums: torch %.4f at %s; chain %.4f at %s)' % (
            R.G, R.G_SUMS, R.TORCH_FP32_RATIO, R.TORCH_FP32_AT, R.CHAIN_FP32_RATIO, R.CHAIN_FP32_AT, R.TORCH_FP32_SUM_RATIO,
            R.TORCH_FP32_SUM_AT, R.CHAIN_FP32_SUM_RATIO, R.CHAIN_FP32_SUM_AT))
        for kind, (ratio, c) in sorted(DEVICE_SEEN.items()):
            print(' largest torch fp32 %s ratio %.4f at %s' % (kind, ratio, ids(c)))
        for body, (worst, n) in sorted(WORST.items()):
            print(' %-16s %4d runs, worst |err| / tolerance %.4f' % (body, n, worst))
    assert all(w <= 1.0 for w, _ in WORST.values())
    assert R.TORCH_FP32_RATIO <= R.G / 4 and R.TORCH_FP32_SUM_RATIO <= R.G_SUMS / 4
    if RAN >= set(R.GRID):
        assert ALL_BODIES <= set(WORST), 'never reached: %s' % sorted(ALL_BODIES - set(WORST))
