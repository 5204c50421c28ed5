"""Every fp32 weight-gradient form of csrc/densenet_bwd.hip at its dispatch edges, through the C ABI, against the float64
references of tests/wgrad_ref.py.

One call of gnx_wgrad_bnrelu lands in one of six kernel bodies - t1 (128 x 256 transposed images), t9 (three shifted dY copies,
S in 4 / 8 / 16 / 32), pf (register-prefetched 1x1), plain1, pool (the transition: 2x2 mean first), plain9 - depending on taps,
pool, M, N, K, S, both leading dimensions and the alignment of X, dY, scale and shift ("Weight-gradient forms").
Every body writes per-split slabs that wgrad_reduce_kernel sums, and a split that owns no tile still owes its zero slab.
gnx_wgrad_bnrelu_batch runs the t1 / t9 bodies from a flat block id and must equal the single calls bit for bit; gnx_conv0_wgrad
has three bodies of its own (fast, plain 7x7, 3x3) and a grid-stride loop over tiles.  wgrad_ref.GRID / STEM_GRID hold the smallest
shapes at which each body and each edge between two exists; wgrad_ref.form / stem_form restate the dispatch, and each case first
compares them with gnx_wgrad_bnrelu_form / gnx_conv0_wgrad_form (body, workgroups, splits, both vec flags, the error of a refused
shape), so that a case which silently lands in another body fails, then checks them against gnx_wgrad_workspace /
gnx_conv0_wgrad_workspace and against which slabs were written.  The batch cases also assert that wgrad_ref.batch_takes agrees
with the per-item queries.

X and dY are windows of larger tensors filled with a sentinel of their own, with leading dimensions beyond the extent (the dY
columns at a non-zero column offset); scale and shift have sentinel tails, dW sits in a sentinel frame, the workspace is exactly
the queried number of floats, NaN-filled, plus a finite sentinel tail.  After a call dW is within the tolerance everywhere (a
NaN or an infinity is a miss), everything outside dW, the workspace's tail and every input are bit-unchanged, the first splits *
taps * N * K workspace floats hold no NaN and the rest still does; a second call gives the same bits.

Tolerance, per element: |err| <= G 2^-24 T, T the sum of the term magnitudes.  Every term is exactly 0 or bounded away from 0
(wgrad_ref's docstring) and each case asserts smallest non-zero term >= 4 x its largest tolerance: one dropped, doubled or
misplaced position or tap fails.

G.  Two plain fp32 evaluations were measured against the float64 references over every case of GRID and STEM_GRID, with and
without the activation, as max |err| / (2^-24 T):
    fp32 torch.matmul on the device (one per tap)       4.339   (taps 1, 130 x 260 x 132 (M x N x K);  4.17 at taps 9, one 64 x 64 map, N 32,
                                                                 K 128;  3.94 at 256 x 256 x 132, 3.87 at 1000 x 512 x 1028)
    sequential fp32 multiply-add chain on the CPU       2.969   (taps 9, 6 maps of 4 x 4, N 32, K 256;  2.77 at 2 maps of 8 x 8, K 256;
                                                                 2.48 at taps 1, 225 x 128 x 132;  stem 1.12 at 513 maps of 16 x 32)
G = max(8, 4 x 4.3391) = 17.36 (wgrad_ref.G).  The kernels' own error had no part in it.  Both measurements stay runnable:
test_plain_fp32_matmul_stays_within_the_ratio_G_was_set_from here, the chain in test_wgrad_ref_host.py; each prints its figures.
"""
import ctypes
import struct
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as R
from gridnext_amd import _lib as L
from test_gpu_bn_forms import Emb, Vec, P

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WS_TAIL, WS_SENTINEL = 64, 555.25
FRAME, DW_SENTINEL = 64, -4242.5
NAN = float('nan')
WORST = {}                                   # body -> [worst |err| / tol, runs]
BAD_ARG, UNSUPPORTED = 'bad argument', 'unsupported shape'
ERR = {BAD_ARG: R.ERR_BAD_ARG, UNSUPPORTED: R.ERR_UNSUPPORTED}


def ids(c):
    return '-'.join(str(v) for v in c)


# ----------------------------------------------------------------------------------------------------------- operands
class Chan(Vec):
    """A per-channel vector 16 floats into a sentinel-filled buffer (+ `shift` floats: off 16 B), sentinel on both sides."""

    def __init__(self, val, C, sentinel, shift=0):
        self.C = C
        self.buf = torch.full((C + 32,), sentinel, device=DEV)
        self.buf[16 + shift:16 + shift + C] = val.float().to(DEV)
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 4 * (16 + shift)


class Framed:
    """`n` floats between two sentinel frames; val None: sentinel throughout (an output that must be written whole)."""

    def __init__(self, val, n, sentinel=DW_SENTINEL, shift=0):
        self.n, self.lo = n, FRAME + shift
        self.buf = torch.full((n + 2 * FRAME + 4,), sentinel, device=DEV)
        if val is not None:
            self.buf[self.lo:self.lo + n] = val.reshape(-1).float().to(DEV)
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 4 * self.lo

    def get(self):
        return self.buf[self.lo:self.lo + self.n].cpu()

    def unchanged(self):
        return torch.equal(self.buf, self.before)

    def outside_unchanged(self):
        return (torch.equal(self.buf[:self.lo], self.before[:self.lo])
                and torch.equal(self.buf[self.lo + self.n:], self.before[self.lo + self.n:]))


class Workspace:
    """Exactly `n` floats of NaN and a finite sentinel tail."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + WS_TAIL,), NAN, device=DEV)
        self.buf[n:] = WS_SENTINEL
        self.ptr = self.buf.data_ptr()

    def tail_unchanged(self):
        return bool((self.buf[self.n:] == WS_SENTINEL).all())

    def written_exactly(self, m):
        """The first m floats hold no NaN, the rest is still NaN."""
        return not bool(torch.isnan(self.buf[:m]).any()) and bool(torch.isnan(self.buf[m:self.n]).all())

    def untouched(self):
        return self.written_exactly(0) and self.tail_unchanged()


class Operands:
    """X, dY, scale and shift of a case on the device, in the case's layouts."""

    def __init__(self, c):
        r = R.recipe(c)
        self.c = c
        ldx, offx, shx = R.lay(c.xlay, c.K)
        ldy, offy, shy = R.lay(c.ylay, c.N)
        self.X = Emb(r.X, R.x_rows(c), c.K, ldx, offx, 1234.5, shx)
        self.dY = Emb(r.dY, c.M, c.N, ldy, offy, -4321.5, shy)
        self.scale, self.shift = Chan(r.scale, c.K, 77.75, c.ss), Chan(r.shift, c.K, -88.25, c.ss)
        assert (self.X.ptr % 16 != 0) == (c.xlay == 'shifted') and (self.dY.ptr % 16 != 0) == (c.ylay == 'shifted')
        assert (ldx % 4 != 0) == (c.xlay == 'oddld') and (ldy % 4 != 0) == (c.ylay == 'oddld') and ldx > c.K and ldy > c.N
        assert (self.scale.ptr % 16 != 0) == bool(c.ss) and (self.shift.ptr % 16 != 0) == bool(c.ss)

    def inputs_unchanged(self):
        return self.X.unchanged() and self.dY.unchanged() and self.scale.unchanged() and self.shift.unchanged()

    def args(self, act, dW, space, acc, **kw):
        c = self.c
        p = dict(dY=self.dY.ptr, lddy=self.dY.ld, X=self.X.ptr, ldx=self.X.ld, scale=P(self.scale if act else None),
                 shift=P(self.shift if act else None), dW=dW.ptr, ws=space.ptr, M=c.M, N=c.N, K=c.K, S=c.S, taps=c.taps,
                 pool=c.pool, acc=acc)
        p.update(kw)
        return [p[k] for k in ('dY', 'lddy', 'X', 'ldx', 'scale', 'shift', 'dW', 'ws', 'M', 'N', 'K', 'S', 'taps', 'pool', 'acc')]


def query_workspace(c):
    nws = L.query('gnx_wgrad_workspace', c.M, c.N, c.K, c.taps)
    assert nws == R.workspace_floats(c.M, c.N, c.K, c.taps), 'gnx_wgrad_workspace%s = %d' % ((c.M, c.N, c.K, c.taps), nws)
    return nws


def query(*args):
    """(code, workgroups, splits, vec_x, vec_dy) of gnx_wgrad_bnrelu_form."""
    out = [ctypes.c_int(-7) for _ in range(4)]
    return (L.query('gnx_wgrad_bnrelu_form', *args, *[ctypes.addressof(v) for v in out]),) + tuple(v.value for v in out)


def new_dw(c, acc):
    return Framed(R.recipe(c).dW0 if acc else None, c.N * c.K * c.taps)


def wgrad(o, act, acc):
    """One call of gnx_wgrad_bnrelu on the operands `o`; returns dW [N][K][taps] on the host."""
    c = o.c
    f = R.form_of(c, act)
    dW, ws = new_dw(c, acc), Workspace(query_workspace(c))
    what = 'case %s act %d acc %d (%s, %d splits)' % (ids(c), act, acc, f.body, f.splits)
    said = query(*o.args(act, dW, ws, acc))
    assert said == R.answer(f), what + ': gnx_wgrad_bnrelu_form says %s, wgrad_ref.form %s' % (said, R.answer(f))
    L.call('gnx_wgrad_bnrelu', *o.args(act, dW, ws, acc), L.stream())
    torch.cuda.synchronize()
    assert o.inputs_unchanged(), what + ': an input was written'
    assert dW.outside_unchanged(), what + ': wrote outside dW'
    assert ws.tail_unchanged(), what + ': wrote past the workspace'
    assert ws.written_exactly(f.splits * c.taps * c.N * c.K), what + ': not exactly the slabs of %d splits were written' % f.splits
    return dW.get().view(c.N, c.K, c.taps)


def _unravel(i, shape):
    idx = []
    for n in reversed(shape):
        i, r = divmod(i, n)
        idx.append(r)
    return tuple(reversed(idx))


def ratio_of(what, got, ref, t):
    """The largest |err| / tolerance; a miss (a NaN or an infinity in `got` included) raises.  An element without a term has a
    tolerance of 0: it must be exactly 0."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    miss = ~(err <= t)
    if miss.any():
        ratio = torch.where(miss, torch.nan_to_num(err / t, nan=float('inf')), torch.zeros_like(err))
        i = int(ratio.argmax())
        raise AssertionError("%s: %d of %d elements miss; worst |err| %.4e = %.3g x tolerance %.4e at %s (got %.9g, want %.9g)" % (
            what, int(miss.sum()), miss.numel(), err.flatten()[i].item(), ratio.max().item(), t.flatten()[i].item(),
            _unravel(i, err.shape), got.flatten()[i].item(), ref.flatten()[i].item()))
    live = t > 0
    return (err[live] / t[live]).max().item() if live.any() else 0.0


def note(body, ratio):
    w = WORST.setdefault(body, [0.0, 0])
    w[0], w[1] = max(w[0], ratio), w[1] + 1


def check_against_float64(c, act, acc, got):
    ref, T, term = R.reference(c, act, acc)
    t = R.tol(T)
    assert R.detectable(term, t), 'case %s: the smallest non-zero term is below 4 tolerances' % ids(c)
    f = R.form_of(c, act)
    r = ratio_of('case %s act %d acc %d (%s, %d splits of %d tiles, %d empty)' % (ids(c), act, acc, f.body, f.splits, f.tps,
                                                                                  f.empty), got, ref, t)
    note(f.body, r)


# --------------------------------------------------------------------------------------------------- 1. the whole grid
@pytest.mark.parametrize("c", R.GRID, ids=ids)
def test_grid(c):
    o = Operands(c)
    failed = []                                                # every run of the case: a failure names all that miss
    for act, acc in R.FLAGS:
        try:
            got = wgrad(o, act, acc)
            check_against_float64(c, act, acc, got)
            assert torch.equal(got, wgrad(o, act, acc)), 'case %s act %d acc %d: a second call gives other bits' % (ids(c), act, acc)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)


# --------------------------------------------------------------------------------------------------- 2. refusals
def test_refusals_write_nothing():
    c = R.nine(2, 4, 8, 12)
    o = Operands(c)
    p1 = R.pooled(2, 4, 8, 12)
    op = Operands(p1)
    big = R.nine(1, R.MAX_S_PLAIN9 + 1, 8, 8)
    ob = Operands(big)
    assert R.form_of(big).body is None and R.form_of(R.nine(1, R.MAX_S_PLAIN9, 8, 8)).body == 'plain9'
    runs = [
        (o, dict(lddy=c.N - 1), BAD_ARG), (o, dict(ldx=c.K - 1), BAD_ARG), (o, dict(taps=3), BAD_ARG),
        (o, dict(taps=9, pool=1), BAD_ARG), (o, dict(M=c.M - 1), BAD_ARG),                      # M % S^2 != 0 at taps = 9
        (op, dict(S=1), BAD_ARG), (o, dict(shift=None), BAD_ARG), (o, dict(scale=None), BAD_ARG), (o, dict(M=0), BAD_ARG),
        (o, dict(ws=None), BAD_ARG), (o, dict(taps=1, M=0), BAD_ARG), (op, dict(ws=None), BAD_ARG),
        (ob, dict(), UNSUPPORTED),
    ]
    for ops, kw, code in runs:
        k = ops.c
        for act in ((1,) if 'scale' in kw or 'shift' in kw else (0, 1)):
            dW, ws = Framed(None, k.N * k.K * k.taps), Workspace(query_workspace(k))
            assert query(*ops.args(act, dW, ws, 0, **kw)) == (ERR[code], 0, 0, 0, 0), (kw, code)
            with pytest.raises(RuntimeError, match=code):
                L.call('gnx_wgrad_bnrelu', *ops.args(act, dW, ws, 0, **kw), L.stream())
            torch.cuda.synchronize()
            assert dW.unchanged() and ws.untouched() and ops.inputs_unchanged(), (kw, code)
    # the extents themselves are legal: lddy == N, ldx == K
    r = R.recipe(c)
    X, dY = Emb(r.X, c.M, c.K, c.K, 0, 1234.5), Emb(r.dY, c.M, c.N, c.N, 0, -4321.5)
    dW, ws = Framed(None, c.N * c.K * 9), Workspace(query_workspace(c))
    L.call('gnx_wgrad_bnrelu', *o.args(1, dW, ws, 0, X=X.ptr, ldx=c.K, dY=dY.ptr, lddy=c.N), L.stream())
    torch.cuda.synchronize()
    check_against_float64(c, 1, 0, dW.get().view(c.N, c.K, 9))
    assert X.unchanged() and dY.unchanged() and dW.outside_unchanged() and ws.tail_unchanged()


# --------------------------------------------------------------------------------------------------- 3. the batch
Item = L.struct('gnx_wgrad_item')      # fields in the header's order: dY lddy X ldx scale shift dW workspace M N K S accumulate


def batch_item(o, act, acc):
    c = o.c
    dW, ws = new_dw(c, acc), Workspace(query_workspace(c))
    it = Item(o.dY.ptr, o.dY.ld, o.X.ptr, o.X.ld, P(o.scale if act else None), P(o.shift if act else None), dW.ptr, ws.ptr,
              c.M, c.N, c.K, c.S, acc)
    return it, dW, ws


def batch_taken(taps, made):
    """Whether gnx_wgrad_bnrelu_batch takes these (operands, activation, item) triples: wgrad_ref.batch_takes on the restated
    forms, which must agree with what gnx_wgrad_bnrelu_form says of each item as a single call (pool = 0)."""
    forms, codes = [], []
    for o, act, it in made:
        f = R.form_of(o.c, act)
        said = query(it.dY, it.lddy, it.X, it.ldx, it.scale, it.shift, it.dW, it.workspace, it.M, it.N, it.K, it.S, taps, 0,
                     it.accumulate)
        assert said == R.answer(f), 'item %s act %d: gnx_wgrad_bnrelu_form says %s, wgrad_ref.form %s' % (ids(o.c), act, said, R.answer(f))
        forms.append(NS(body=f.body, S=it.S))
        codes.append(said[0])
    takes = R.batch_takes(taps, forms)
    assert takes == (all(k == R.CODES['t1' if taps == 1 else 't9'] for k in codes) and (taps == 1 or len({it.S for _, _, it in made}) == 1))
    return takes


def run_batch(cases, taps):
    """The batch against the single calls, item by item: equal bits, each item's own workspace written as the single call writes
    it; items mixed with and without activation, each with its own `accumulate`.  Every single call against float64."""
    ops = {}
    flags = [(((i + 1) // 2) % 2, i % 2) for i in range(len(cases))]
    items = []
    for c, (act, acc) in zip(cases, flags):
        o = ops.setdefault(c, Operands(c))
        items.append((o, act, acc) + batch_item(o, act, acc))
    assert {a for _, a, _, _, _, _ in items} == {0, 1} or len(cases) == 1
    arr = (Item * len(items))(*[it for _, _, _, it, _, _ in items])
    assert batch_taken(taps, [(o, act, it) for o, act, _, it, _, _ in items])
    L.call('gnx_wgrad_bnrelu_batch', ctypes.addressof(arr), len(items), taps, L.stream())
    torch.cuda.synchronize()
    for i, (o, act, acc, _, dW, ws) in enumerate(items):
        c, f = o.c, R.form_of(o.c, act)
        what = 'item %d of %d, case %s act %d acc %d' % (i, len(items), ids(c), act, acc)
        assert f.body == ('t1' if taps == 1 else 't9')
        assert o.inputs_unchanged() and dW.outside_unchanged() and ws.tail_unchanged(), what
        assert ws.written_exactly(f.splits * taps * c.N * c.K), what
        single = wgrad(o, act, acc)
        check_against_float64(c, act, acc, single)
        assert torch.equal(dW.get().view(c.N, c.K, taps), single), what + ': the batch differs from the single call'


# one and two k blocks, N = 128 and 256, 8 and 16 splits, a ragged last tile, empty splits
BATCH1 = [R.one(*R.T1), R.one(256, 128, 260), R.one(256, 256, 132), R.one(*R.T1_EMPTY[0]), R.one(225, 128, 256), R.one(320, 256, 260)]


def _batch1(n):
    if n == 1:
        return [R.one(*R.T1_EMPTY[0])]
    if n == 2:
        return [R.one(256, 256, 260), R.one(*R.T1_EMPTY[0])]
    return [BATCH1[i % len(BATCH1)]._replace(M=BATCH1[i % len(BATCH1)].M + 32 * (i // len(BATCH1))) for i in range(n)]


@pytest.mark.parametrize("n", [1, 2, 24, 25])
def test_batch_1x1_equals_the_single_calls(n):
    """n = 25: the second launch of one item."""
    cases = _batch1(n)
    assert len(set(cases)) == n and any(R.form_of(c).empty for c in cases) and n in (1, 2, R.WG_BATCH, R.WG_BATCH + 1)
    if n > 2:
        assert {R.form_of(c).splits for c in cases} >= {8, 16} and {c.N for c in cases} == {128, 256}
        assert {-(-c.K // 256) for c in cases} == {1, 2}
    run_batch(cases, 1)


@pytest.mark.parametrize("S,imgs", [(4, (6, 8, 16)), (8, (2, 3, 4)), (16, (2, 2, 3)), (32, (2, 2, 3))])
def test_batch_3x3_equals_the_single_calls(S, imgs):
    cases = [R.nine(n, S, 32, K) for n, K in zip(imgs, (128, 256, 128))]
    run_batch(cases, 9)


def test_batch_refusals_write_nothing():
    good1, good9 = R.one(*R.T1), R.nine(2, 8, 32, 128)
    refused = [
        (1, [R.one(*R.PF)]), (1, [good1, R.one(*R.PF)]), (1, [good1, R.one(*R.T1, xlay='shifted')]), (1, [R.one(*R.T1, ylay='oddld'), good1]),
        (1, [good1, R.one(256, 130, 132)]),
        (9, [good9, R.nine(2, 16, 32, 128)]), (9, [R.nine(1, 64, 32, 128)]), (9, [R.nine(8, 4, 32, 128), R.nine(7, 4, 32, 128)]),
        (9, [good9, R.nine(2, 8, 33, 128)]), (9, [R.nine(2, 8, 32, 128, ylay='shifted'), good9]),
    ]
    for taps, cases in refused:
        made = [(Operands(c),) for c in cases]
        made = [(o,) + batch_item(o, i % 2, 0) for i, (o,) in enumerate(made)]
        arr = (Item * len(made))(*[it for _, it, _, _ in made])
        assert not batch_taken(taps, [(o, i % 2, it) for i, (o, it, _, _) in enumerate(made)]), (taps, cases)
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            L.call('gnx_wgrad_bnrelu_batch', ctypes.addressof(arr), len(made), taps, L.stream())
        torch.cuda.synchronize()
        for o, _, dW, ws in made:
            assert dW.unchanged() and ws.untouched() and o.inputs_unchanged(), (taps, cases)
    o = Operands(good1)
    it, dW, ws = batch_item(o, 1, 0)
    arr = (Item * 1)(it)
    L.call('gnx_wgrad_bnrelu_batch', ctypes.addressof(arr), 0, 1, L.stream())                 # n = 0: GNX_OK
    for n, taps in ((-1, 1), (1, 3)):
        with pytest.raises(RuntimeError, match=BAD_ARG):
            L.call('gnx_wgrad_bnrelu_batch', ctypes.addressof(arr), n, taps, L.stream())
    with pytest.raises(RuntimeError, match=BAD_ARG):
        L.call('gnx_wgrad_bnrelu_batch', None, 1, 1, L.stream())
    torch.cuda.synchronize()
    assert dW.unchanged() and ws.untouched() and o.inputs_unchanged()


# --------------------------------------------------------------------------------------------------- 4. the stem
class StemOperands:
    def __init__(self, s):
        r = R.stem_recipe(s._replace(acc=0))
        Ho, Wo = R.stem_out(s)
        self.s = s
        self.x = Framed(r.x, r.x.numel(), 1234.5, shift=s.xmis)
        self.dS = Emb(r.dS, s.imgs * Ho * Wo, s.O, s.ldd, 4 if s.ldd - s.O >= 4 else 0, -4321.5)
        assert (self.x.ptr % 16 != 0) == bool(s.xmis) and self.dS.ptr % 16 == 0

    def args(self, dW, space, **kw):
        s = self.s
        p = dict(x=self.x.ptr, dS=self.dS.ptr, ldd=s.ldd, dW=dW.ptr, ws=space.ptr, imgs=s.imgs, H=s.H, W=s.W, O=s.O, KH=s.KH, KW=s.KH,
                 stride=s.stride, pad=s.pad, acc=s.acc)
        p.update(kw)
        return [p[k] for k in ('x', 'dS', 'ldd', 'dW', 'ws', 'imgs', 'H', 'W', 'O', 'KH', 'KW', 'stride', 'pad', 'acc')]


def stem_query(*args):
    """(code, workgroups) of gnx_conv0_wgrad_form."""
    w = ctypes.c_int(-7)
    return L.query('gnx_conv0_wgrad_form', *args, ctypes.addressof(w)), w.value


def stem_wgrad(o):
    s = o.s
    f = R.stem_form_of(s)
    nws = L.query('gnx_conv0_wgrad_workspace', s.imgs, s.H, s.W, s.O, s.KH, s.KH, s.stride, s.pad)
    assert nws == f.floats, 'gnx_conv0_wgrad_workspace of %s = %d, stem_form says %d slabs' % (ids(s), nws, f.slabs)
    dW = Framed(R.stem_recipe(s._replace(acc=0)).dW0 if s.acc else None, s.O * 3 * s.KH * s.KH)
    ws = Workspace(nws)
    what = 'stem %s (%s, %d blocks)' % (ids(s), f.body, f.blocks)
    assert stem_query(*o.args(dW, ws)) == (R.CODES[f.body], f.blocks), what + ': gnx_conv0_wgrad_form says otherwise'
    L.call('gnx_conv0_wgrad', *o.args(dW, ws), L.stream())
    torch.cuda.synchronize()
    assert o.x.unchanged() and o.dS.unchanged(), what + ': an input was written'
    assert dW.outside_unchanged() and ws.tail_unchanged(), what + ': wrote outside dW or past the workspace'
    assert ws.written_exactly(nws), what + ': a slab was not written whole'
    return dW.get().view(s.O, 3, s.KH, s.KH)


@pytest.mark.parametrize("s", R.STEM_GRID, ids=ids)
def test_stem_grid(s):
    o = StemOperands(s)
    got = stem_wgrad(o)
    rs = s._replace(acc=0)
    ref, T, term = R.stem_reference(rs)
    if s.acc:
        d = R.stem_recipe(rs).dW0
        ref, T = ref + d, T + d.abs()
    t = R.tol(T)
    assert R.detectable(term, t), 'stem %s: the smallest term is below 4 tolerances' % ids(s)
    f = R.stem_form_of(s)
    note('stem ' + f.body, ratio_of('stem %s (%s, %d tiles on %d blocks)' % (ids(s), f.body, f.tiles, f.blocks), got, ref, t))
    assert torch.equal(got, stem_wgrad(o)), 'stem %s: a second call gives other bits' % ids(s)


def test_stem_refusals_write_nothing():
    s = R.stem7(2, 16, 32, O=10)
    o = StemOperands(s)
    wide = StemOperands(R.stem7(2, 16, 32, O=65))
    runs = [(wide, dict(), BAD_ARG), (o, dict(ldd=s.O - 1), BAD_ARG), (o, dict(KH=5, KW=5), UNSUPPORTED), (o, dict(ws=None), BAD_ARG),
            (o, dict(imgs=0), BAD_ARG), (o, dict(stride=1), UNSUPPORTED)]
    for ops, kw, code in runs:
        k = ops.s
        dW, ws = Framed(None, k.O * 3 * 49), Workspace(4 * 2 * k.O * 3 * 49)
        assert stem_query(*ops.args(dW, ws, **kw)) == (ERR[code], 0), (kw, code)
        with pytest.raises(RuntimeError, match=code):
            L.call('gnx_conv0_wgrad', *ops.args(dW, ws, **kw), L.stream())
        torch.cuda.synchronize()
        assert dW.unchanged() and ws.untouched() and ops.x.unchanged() and ops.dS.unchanged(), (kw, code)


# --------------------------------------------------------------------------------------------------- 5. the re-layouts
RELAYOUT_SHAPES = [(1, 1), (5, 7), (32, 128), (128, 992)]
SINGLES = {0: 'gnx_repack_conv3x3', 1: 'gnx_repack_conv3x3_bwd', 2: 'gnx_transpose_weight'}


def relayout_weight(N, K, kind, seed=0):
    """Distinct float32 values (exact integers) in the source layout [N][K][taps]."""
    n = N * K * (1 if kind == 2 else 9)
    return (torch.arange(n, dtype=torch.float32) + 1 + 7 * seed).view(N, K, -1)


def relayout_formula(w, kind):
    """The index formulas of include/gridnext_hip.h: 0: [tap][n][k], 1: [8 - tap][k][n], 2: [k][n]."""
    if kind == 0:
        return w.permute(2, 0, 1).contiguous()
    if kind == 1:
        return w.flip(2).permute(2, 1, 0).contiguous()
    return w[:, :, 0].t().contiguous()


@pytest.mark.parametrize("N,K", RELAYOUT_SHAPES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_single_relayouts_equal_the_index_formulas(N, K, kind):
    w = relayout_weight(N, K, kind)
    src, dst = Framed(w, w.numel(), 1234.5), Framed(None, w.numel())
    L.call(SINGLES[kind], src.ptr, dst.ptr, N, K, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(dst.get(), relayout_formula(w, kind).reshape(-1)) and dst.outside_unchanged() and src.unchanged()
    for kw in (dict(N=0), dict(K=0), dict(src=None), dict(dst=None)):
        p = dict(src=src.ptr, dst=dst.ptr, N=N, K=K)
        p.update(kw)
        before = dst.buf.clone()
        with pytest.raises(RuntimeError, match=BAD_ARG):
            L.call(SINGLES[kind], p['src'], p['dst'], p['N'], p['K'], L.stream())
        torch.cuda.synchronize()
        assert torch.equal(dst.buf, before)


def device_table(entries, shift=0):
    rows = b''.join(struct.pack('<QQii', s.ptr, d.ptr, N, K) for s, d, N, K in entries)
    t = torch.frombuffer(bytearray(b'\0' * shift + rows + b'\0' * 8), dtype=torch.uint8).to(DEV)
    assert t.data_ptr() % 8 == 0
    return t, t.data_ptr() + shift


@pytest.mark.parametrize("n", [1, 60])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_batched_relayout_equals_the_single_calls(kind, n):
    """One launch over a device table against the single calls and the index formulas; an entry of more than 16 x 256 elements
    runs the grid-stride loop more than once."""
    mixed = [(128, 992), (5, 7), (32, 128), (1, 1), (3, 130), (33, 12), (130, 33)]
    shapes = [mixed[i % len(mixed)] for i in range(n)]
    assert any(N * K * (1 if kind == 2 else 9) > 16 * 256 for N, K in shapes)
    ws = [relayout_weight(N, K, kind, seed=i) for i, (N, K) in enumerate(shapes)]
    srcs = [Framed(w, w.numel(), 1234.5) for w in ws]
    dsts = [Framed(None, w.numel()) for w in ws]
    table, tptr = device_table([(s, d, N, K) for s, d, (N, K) in zip(srcs, dsts, shapes)])
    L.call('gnx_relayout_weights_batch', tptr, n, kind, L.stream())
    torch.cuda.synchronize()
    for i, (w, s, d, (N, K)) in enumerate(zip(ws, srcs, dsts, shapes)):
        one = Framed(None, w.numel())
        L.call(SINGLES[kind], s.ptr, one.ptr, N, K, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(d.get(), relayout_formula(w, kind).reshape(-1)), (i, N, K)
        assert torch.equal(d.buf, one.buf) and d.outside_unchanged() and s.unchanged(), (i, N, K)


def test_batched_relayout_refusals_write_nothing():
    w = relayout_weight(5, 7, 2)
    src, dst = Framed(w, w.numel(), 1234.5), Framed(None, w.numel())
    table, tptr = device_table([(src, dst, 5, 7)])
    off, optr = device_table([(src, dst, 5, 7)], shift=4)
    assert optr % 8 == 4
    L.call('gnx_relayout_weights_batch', tptr, 0, 2, L.stream())                                # n = 0: GNX_OK
    for args in ((tptr, 1, 3), (tptr, 1, -1), (optr, 1, 2), (None, 1, 2), (tptr, -1, 2)):
        with pytest.raises(RuntimeError, match=BAD_ARG):
            L.call('gnx_relayout_weights_batch', *args, L.stream())
    torch.cuda.synchronize()
    assert dst.unchanged() and src.unchanged()


# ------------------------------------------------------------------------------------------------- where G comes from
def _device_ratio(c, act):
    r = R.recipe(c)
    X, dY = r.X.float().to(DEV), r.dY.float().to(DEV)
    a = R.activate_fp32(X, r.scale.float().to(DEV), r.shift.float().to(DEV)) if act else X
    if c.pool:
        So = c.S // 2
        m = a.view(c.imgs, c.S, c.S, -1)
        q = [m[:, dy:2 * So:2, dx:2 * So:2] for dy in (0, 1) for dx in (0, 1)]
        got = torch.matmul(dY.t(), ((((q[0] + q[1]) + q[2]) + q[3]) * 0.25).reshape(c.M, -1))[:, :, None]
    elif c.taps == 9:
        got = torch.stack([torch.matmul(dY.t(), R.shifted(a, c.imgs, c.S, t // 3, t % 3)) for t in range(9)], 2)
    else:
        got = torch.matmul(dY.t(), a)[:, :, None]
    ref, T, _ = R.reference(c, act, 0)
    return R.ratio(got.cpu(), ref, T)


@pytest.mark.parametrize("c", R.GRID, ids=ids)
def test_plain_fp32_matmul_stays_within_the_ratio_G_was_set_from(c, capsys):
    """The device half of the measurement behind wgrad_ref.G, kept runnable: the same contraction as fp32 torch.matmul on the
    device (the activation and the 2x2 mean in fp32, one matmul per tap on the shifted operand) against the float64 reference,
    max |err| / (2^-24 T), with and without the activation.  A torch whose GEMM rounds differently fails here with the figure
    to set TORCH_FP32_RATIO (and with it G) from."""
    ratio = max(_device_ratio(c, 0), _device_ratio(c, 1))
    with capsys.disabled():
        print(' torch fp32 ratio at %s: %.4f' % (ids(c), ratio))
    assert ratio <= R.TORCH_FP32_RATIO, ratio


@pytest.mark.parametrize("s", R.STEM_GRID, ids=ids)
def test_plain_fp32_matmul_of_the_stem_stays_within_the_ratio(s, capsys):
    rs = s._replace(acc=0)
    r = R.stem_recipe(rs)
    cols = F.unfold(r.x.float().to(DEV), (s.KH, s.KH), padding=s.pad, stride=s.stride)        # [imgs][3 KH KH][Ho Wo]
    B = cols.permute(0, 2, 1).reshape(-1, cols.shape[1])
    got = torch.matmul(r.dS.float().to(DEV).t(), B)
    ref, T, _ = R.stem_reference(rs)
    ratio = R.ratio(got.cpu().view_as(ref), ref, T)
    with capsys.disabled():
        print(' torch fp32 ratio at stem %s: %.4f' % (ids(s), ratio))
    assert ratio <= R.TORCH_FP32_RATIO, ratio


def test_report_worst_ratio_per_body(capsys):
    """Prints what the tests above saw: per kernel body the largest |err| / tolerance and the number of runs (empty when this
    test runs alone)."""
    with capsys.disabled():
        print('\n G = %.3f (torch fp32 %.4f at %s, fp32 chain %.4f at %s)' % (R.G, R.TORCH_FP32_RATIO, R.TORCH_FP32_AT,
                                                                           R.CHAIN_FP32_RATIO, R.CHAIN_FP32_AT))
        for body, (worst, n) in sorted(WORST.items()):
            print(' %-11s worst |err| / tolerance %.4f over %d runs' % (body, worst, n))
    assert all(w <= 1.0 for w, _ in WORST.values())
