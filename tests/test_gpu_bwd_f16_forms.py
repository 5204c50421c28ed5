"""Every kernel form of the fp16 gradient path (csrc/dense_bwd_f16.hip, and the two conv1x1_h16 tile forms of
csrc/densenet_f16.hip) at its dispatch edges, through the C ABI, against the float64 references of tests/bwd_f16_ref.py.

Eleven kernels behind the entry points of dense_bwd_f16.hip: which body runs and on what slab plan depends on M, S, N, K, on
whether a weight gradient is asked for, and on the layouts ("fp16 backward forms").  bwd_f16_ref.GRID holds the
smallest shapes at which each body and each edge exists; bwd_f16_ref.form_* restate the dispatch, and every case first compares
them with the library's gnx_*_form query (body, workgroups, slabs, tiles per slab; slots and thread map for the elementwise
adjoints), so that a case which silently lands in another body fails, then with the gnx_*_workspace query.

Every operand is a window of a larger sentinel-filled allocation: row-major matrices have leading dimensions beyond their
extent and start at a column offset, channel-blocked buffers have rows_total > M (dP, X and G each their own), every
allocation of a matrix begins 16 sentinel elements before it and ends 8 after it, per-channel inputs carry sentinel tails, fp32
outputs (dW, dgamma, dbeta) sit between two sentinel frames, fp16 outputs start as NaN inside a finite sentinel frame.  The workspace
is exactly the queried number of floats, NaN-filled, plus a finite tail; the flag starts at 0.  After a call every output element
is within its tolerance (a NaN or an infinity is a miss), everything outside the outputs and every input is bit-unchanged,
exactly the planned slabs hold no NaN, the flag is still 0, and a second call gives the same bits.  Every case runs with
accumulate = 0 onto NaN and with accumulate = 1 onto a non-zero prior.  A long case whose BatchNorm sums need a thinned ReLU mask
(bwd_f16_ref.thinned) runs a second time with half of the mask live and without those sums: dB, G and the weight gradients are
then compared on a dense mask at the same shape and slab plan.  The flag tests place ONE infinity, in the first and in the last
valid row, in columns that are not lane 0 of a reduce block.

Tolerances and G: bwd_f16_ref's docstring.  The device half of the measurement behind G stays runnable here
(test_plain_fp32_matmul_stays_within_the_ratio_G_was_set_from), the chain half in test_bwd_f16_ref_host.py.
"""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

import bwd_f16_ref as R
from gridnext_amd import _lib as L
from test_gpu_bn_forms import Vec, P
from test_gpu_wgrad_forms import Framed, Workspace, ratio_of

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
H = torch.float16
NAN = float('nan')
WORST = {}                                   # body -> [worst |err| / tol, runs]
SEEN = set()                                 # every code a form query answered for a call that then ran
BAD_ARG, UNSUPPORTED = 'bad argument', 'unsupported shape'
ERR = {BAD_ARG: R.ERR_BAD_ARG, UNSUPPORTED: R.ERR_UNSUPPORTED}
ESIZE = {torch.float16: 2, torch.float32: 4}


# ----------------------------------------------------------------------------------------------------------- operands
class Buf:
    """[M][C] values inside a sentinel-filled allocation that begins LEAD elements (a multiple of 16 B) before the matrix and ends
    8 after it.  'rows': the window [0:M, off:off+C] of an [M + 3][C + extra] matrix; 'blocked': rows [0, M) of every block of
    [C / 32][M + pad][32].  val None: NaN inside the window (an output)."""
    LEAD = 16

    def __init__(self, val, M, C, lay, sentinel, extra=24, off=8, pad=5, dtype=H):
        self.M, self.C, self.lay = M, C, lay
        if lay == 'rows':
            off = off if extra else 0
            self.ld, self.bs, self.rows_total = C + extra, 32, M + 3
            n = self.rows_total * self.ld
        else:
            assert C % 32 == 0
            off = 0
            self.ld, self.rows_total = 32, M + pad
            self.bs = self.rows_total * 32
            n = (C // 32) * self.bs
        self.n, self.off = n, off
        self.flat = torch.full((self.LEAD + n + 8,), float(sentinel), device=DEV, dtype=dtype)
        v = torch.full((M, C), NAN, dtype=dtype) if val is None else val.to(dtype)
        self._window(self.flat).copy_(self._shape(v.to(DEV)))
        self.before = self.flat.clone()
        self.ptr = self.flat.data_ptr() + ESIZE[dtype] * (self.LEAD + off)
        assert self.ptr % 16 == 0

    def _shape(self, v):
        return v if self.lay == 'rows' else v.view(self.M, self.C // 32, 32).permute(1, 0, 2)

    def _window(self, flat):
        if self.lay == 'rows':
            return flat[self.LEAD:self.LEAD + self.n].view(self.rows_total, self.ld)[:self.M, self.off:self.off + self.C]
        return flat[self.LEAD:self.LEAD + self.n].view(self.C // 32, self.rows_total, 32)[:, :self.M]

    def get(self):
        w = self._window(self.flat)
        return (w if self.lay == 'rows' else w.permute(1, 0, 2).reshape(self.M, self.C)).cpu()

    def unchanged(self):
        return torch.equal(self.flat.view(torch.uint8), self.before.view(torch.uint8))

    def outside_unchanged(self):
        a, b = self.flat.clone(), self.before.clone()
        self._window(a).zero_()
        self._window(b).zero_()
        return torch.equal(a, b)


class Plain:
    """A contiguous operand without a layout of its own (packed weights), with a copy to compare with."""

    def __init__(self, val, dtype=H):
        self.t = val.to(dtype).contiguous().to(DEV)
        self.before = self.t.clone()
        self.ptr = self.t.data_ptr()

    def unchanged(self):
        return torch.equal(self.t, self.before)


class Flag:
    def __init__(self):
        self.t = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.t[1:] = 0x5A5A5A5A
        self.ptr = self.t.data_ptr()

    def value(self):
        v = self.t.cpu()
        assert bool((v[1:] == 0x5A5A5A5A).all()), 'wrote past the flag'
        return int(v[0])


def ls_tensor(s):
    return torch.tensor([s, 1.0 / s], device=DEV, dtype=torch.float32)


def vec(val, C, prior=None, acc=0):
    """A per-channel fp32 input (sentinel tail), or an output between two sentinel frames: the prior under accumulate, NaN
    otherwise."""
    if val is not None:
        return Vec(val.float(), C, 77.75)
    return framed(prior, C, acc)


def framed(prior, n, acc):
    return Framed(prior if acc else torch.full((n,), NAN), n)


def bn_vecs(bn, C):
    return [vec(getattr(bn, k), C) for k in ('scale', 'shift', 'mean', 'invstd')]


# -------------------------------------------------------------------------------------------------------- one call
class Call:
    """One call of an entry point: its arguments by the header's parameter names, what it reads, what it writes."""

    def __init__(self, entry, form, nout, restate, p, inputs, outs, ws, ws_ok, ls, flag):
        self.entry, self.form, self.nout, self.restate = entry, form, nout, restate
        self.p, self.inputs, self.outs, self.ws, self.ws_ok, self.ls, self.flag = p, inputs, outs, ws, ws_ok, ls, flag

    def args(self, name, drop):
        return [self.p[k] for k in L.PARAMS[name][:len(L.PARAMS[name]) - drop]]

    def query(self, **kw):
        outs = [ctypes.c_int(-7) for _ in range(self.nout)]
        saved = dict(self.p)
        self.p.update(kw)
        try:
            rc = L.query(self.form, *self.args(self.form, self.nout), *[ctypes.addressof(o) for o in outs])
        finally:
            self.p = saved
        return (rc,) + tuple(o.value for o in outs)

    def expected(self, **kw):
        f = self.restate(NS(**dict(self.p, **kw)))
        if self.nout == 1:
            return f.code, f.workgroups
        if self.nout == 2:
            return f.code, f.workgroups, f.per
        if 'slots' in L.PARAMS[self.form]:
            return f.code, f.slots, f.workgroups, f.blocked
        return f.code, f.workgroups, f.slabs, f.per

    def launch(self, **kw):
        p = dict(self.p, **kw)
        L.call(self.entry, *[p[k] for k in L.PARAMS[self.entry][:-1]], L.stream())
        torch.cuda.synchronize()

    def untouched(self):
        return (all(i.unchanged() for i in self.inputs) and all(same_bytes(b) for b, _ in self.outs.values())
                and (self.ws is None or self.ws.untouched()))


def same_bytes(o):
    """Bit-unchanged, NaNs included."""
    t = o.flat if hasattr(o, 'flat') else o.buf
    return torch.equal(t.view(torch.uint8), o.before.view(torch.uint8))


def note(body, ratio):
    w = WORST.setdefault(body, [0.0, 0])
    w[0], w[1] = max(w[0], ratio), w[1] + 1


def run(call, what, expect_flag=0, compare=True):
    """Steps 1 to 3 of a case: the form, the call inside its frames, the assertions.  Returns {output: host tensor}."""
    said, want = call.query(), call.expected()
    assert said == want, '%s: %s says %s, bwd_f16_ref %s' % (what, call.form, said, want)
    assert said[0] >= 0, what
    body = R.NAMES[said[0]]
    call.launch()
    SEEN.add(said[0])
    assert all(i.unchanged() for i in call.inputs), what + ': an input was written'
    got = {}
    for name, (buf, o) in call.outs.items():
        assert buf.outside_unchanged() if hasattr(buf, 'outside_unchanged') else buf.tail_unchanged(), what + ': wrote outside ' + name
        got[name] = buf.get().double().reshape(o.ref.shape)
    if call.ws is not None:
        assert call.ws.tail_unchanged(), what + ': wrote past the workspace'
        assert call.ws_ok(call.ws.buf[:call.ws.n]), what + ': not exactly the planned slabs were written'
    if call.flag is not None:
        assert call.flag.value() == expect_flag, what + ': the flag reads %d' % call.flag.value()
    if compare:
        for name, (buf, o) in call.outs.items():
            note(body, ratio_of('%s, %s (%s)' % (what, name, body), got[name], o.ref, R.tol(o)))
    return got


def full_case(build, what, variants=((0, 1.0), (1, 1.0))):
    """Steps 1 to 5: accumulate = 0 onto NaN, the same call again (equal bits), accumulate = 1 onto a prior."""
    failed = []
    for acc, s in variants:
        w = '%s acc %d s %g' % (what, acc, s)
        try:
            got = run(build(acc, s), w)
            again = run(build(acc, s), w + ' (second call)', compare=False)
            for k in got:
                assert torch.equal(got[k], again[k]), w + ': a second call gives other bits in ' + k
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)


def no_nan(t):
    return not bool(torch.isnan(t).any())


def all_nan(t):
    return bool(torch.isnan(t).all())


def first_floats(n):
    return lambda ws: no_nan(ws[:n]) and all_nan(ws[n:])


def refuse(call, kw, code, what):
    assert call.query(**kw) == (ERR[code],) + (0,) * call.nout, (what, kw, call.query(**kw))
    assert call.expected(**kw)[0] == ERR[code], (what, kw)
    with pytest.raises(RuntimeError, match=code):
        call.launch(**kw)
    assert call.untouched(), (what, kw, 'something was written')


# ---------------------------------------------------------------------------------------------------- the builders
def build_wgrad1(c, pro, acc=0, s=1.0, dY=None, flag=True):
    r = R.recipe_wgrad1(c)
    dYb = Buf(r.dY if dY is None else dY, c.M, c.N, 'rows', -4321.0)
    X = Buf(r.X, c.M, c.K, 'rows', 1234.0)
    sc, sh = (vec(r.bn.scale, c.K), vec(r.bn.shift, c.K)) if pro else (None, None)
    o = R.reference_wgrad1(c, pro, s)['dW']
    dW = framed(r.dW0, c.N * c.K, acc)
    nws = L.query('gnx_wgrad1x1_f16_workspace', c.M, c.N, c.K)
    assert nws == R.ws_wgrad1(c.M, c.N, c.K)
    ws, ls, fl = Workspace(nws), ls_tensor(s), Flag() if flag else None
    p = dict(dY16=dYb.ptr, lddy=dYb.ld, X16=X.ptr, ldx=X.ld, scale=P(sc), shift=P(sh), dW=dW.ptr, workspace=ws.ptr, M=c.M, N=c.N, K=c.K,
             ls=ls.data_ptr(), accumulate=acc, flag=P(fl))
    return Call('gnx_wgrad1x1_f16', 'gnx_wgrad1x1_f16_form', 3, R.form_wgrad1, p, [dYb, X] + ([sc, sh] if pro else []),
                dict(dW=(dW, R.with_prior(o, r.dW0) if acc else o)), ws, first_floats(nws), ls, fl)


def conv2_operands(c, lay, dY=None, dense=False):
    r = R.recipe_conv2(c.imgs, c.S, dense)
    dYb = Buf(r.dY if dY is None else dY, r.M, 32, lay, -4321.0, pad=9)
    A = Buf(r.A, r.M, 128, lay, 1234.0)
    return r, dYb, A


def _w2b(r):
    return Plain(r.W2.permute(2, 3, 1, 0).reshape(9, 128, 32))


def build_wgrad3(c, lay, acc=0, s=1.0, dY=None, flag=True, dense=False):
    r, dYb, A = conv2_operands(c, lay, dY, dense)
    o = R.reference_conv2(c.imgs, c.S, s, dense)['dW']
    dW = framed(r.dW0, 36864, acc)
    nws = L.query('gnx_wgrad3x3_f16_workspace', r.M)
    assert nws == R.ws_wgrad3(r.M)
    ws, ls, fl = Workspace(nws), ls_tensor(s), Flag() if flag else None
    p = dict(dY16=dYb.ptr, lddy=dYb.ld, A16=A.ptr, lda=A.ld, bsa=A.bs, dW=dW.ptr, workspace=ws.ptr, M=r.M, S=c.S, ls=ls.data_ptr(),
             accumulate=acc, flag=P(fl))
    return Call('gnx_wgrad3x3_f16_lb', 'gnx_wgrad3x3_f16_form', 3, R.form_wgrad3, p, [dYb, A],
                dict(dW=(dW, R.with_prior(o, r.dW0) if acc else o)), ws, first_floats(nws), ls, fl)


def _bn2_outs(r, ref, want, acc):
    outs, ptrs = {}, {}
    for key, name, prior in (('g', 'dgamma', r.dg0), ('b', 'dbeta', r.db0)):
        if key in want:
            v = vec(None, 128, prior, acc)
            outs[name] = (v, R.with_prior(ref[name], prior) if acc else ref[name])
        ptrs[name] = P(outs[name][0]) if key in want else None
    return outs, ptrs


def build_dgrad3(c, lay, acc=0, s=1.0, dY=None, flag=True, dense=False):
    """dense: the half-live mask of a thinned case, without the BatchNorm sums."""
    r, dYb, A = conv2_operands(c, lay, dY, dense)
    ref = R.reference_conv2(c.imgs, c.S, s, dense)
    W = _w2b(r)
    dB = Buf(None, r.M, 128, 'rows', -999.0, extra=0)
    sc2, g2, b2 = vec(r.scale2, 128), vec(r.gamma2, 128), vec(r.beta2, 128)
    outs, ptrs = _bn2_outs(r, ref, '' if dense else c.want, acc)
    outs['dB'] = (dB, ref['dB'])
    nws = L.query('gnx_conv3x3_dgrad_bnrelu_bwd_f16_workspace', r.M)
    assert nws == R.ws_dgrad3(r.M)
    ws, ls, fl = Workspace(nws), ls_tensor(s), Flag() if flag else None
    p = dict(dY16=dYb.ptr, lddy=dYb.ld, W2b16=W.ptr, A16=A.ptr, lda=A.ld, bsa=A.bs, dB16=dB.ptr, M=r.M, S=c.S, scale2=sc2.ptr,
             gamma2=g2.ptr, beta2=b2.ptr, dgamma=ptrs['dgamma'], dbeta=ptrs['dbeta'], workspace=ws.ptr, ls=ls.data_ptr(),
             accumulate=acc, flag=P(fl))
    return Call('gnx_conv3x3_dgrad_bnrelu_bwd_f16_lb', 'gnx_conv3x3_dgrad_bnrelu_bwd_f16_form', 3, R.form_dgrad3, p,
                [dYb, A, W, sc2, g2, b2], outs, ws, first_floats(nws), ls, fl)


def build_conv3(c, acc=0, s=1.0, dY=None, flag=True, want='gb', dense=False):
    r, dYb, A = conv2_operands(c, c.lay, dY, dense)
    ref = R.reference_conv2(c.imgs, c.S, s, dense)
    want = '' if dense else want
    W = _w2b(r)
    dB = Buf(None, r.M, 128, 'rows', -999.0, extra=0)
    sc2, g2, b2 = vec(r.scale2, 128), vec(r.gamma2, 128), vec(r.beta2, 128)
    outs, ptrs = _bn2_outs(r, ref, want, acc)
    outs['dB'] = (dB, ref['dB'])
    dW = framed(r.dW0, 36864, acc)
    outs['dW'] = (dW, R.with_prior(ref['dW'], r.dW0) if acc else ref['dW'])
    nws = L.query('gnx_conv3x3_bwd_f16_workspace', r.M)
    assert nws == R.ws_conv3(r.M)
    ws, ls, fl = Workspace(nws), ls_tensor(s), Flag() if flag else None
    grid = R.conv3_bwd_grid(r.M) if r.M % 128 == 0 else 1
    used = R.plan_of('conv3', c).slabs if r.M % 128 == 0 else 0

    def ws_ok(t):
        bn, w = t[:grid * 256], t[grid * 256:]
        return no_nan(bn[:used * 256]) and all_nan(bn[used * 256:]) and no_nan(w[:used * 36864]) and all_nan(w[used * 36864:])
    p = dict(dY16=dYb.ptr, lddy=dYb.ld, W2b16=W.ptr, A16=A.ptr, lda=A.ld, bsa=A.bs, dB16=dB.ptr, dW=dW.ptr, M=r.M, S=c.S,
             scale2=sc2.ptr, gamma2=g2.ptr, beta2=b2.ptr, dgamma=ptrs['dgamma'], dbeta=ptrs['dbeta'], workspace=ws.ptr,
             ls=ls.data_ptr(), accumulate=acc, flag=P(fl))
    return Call('gnx_conv3x3_bwd_f16_lb', 'gnx_conv3x3_bwd_f16_form', 2, R.form_conv3, p, [dYb, A, W, sc2, g2, b2], outs, ws, ws_ok,
                ls, fl)


def build_dgrad1(c, wg, acc=0, s=1.0, dB=None, flag=True, want=None, dense=False, operands=None):
    """dense: the half-live mask of a thinned case, without the BatchNorm sums.  operands: (recipe, reference) of the caller's own
    instead of the case's."""
    want = ('' if dense else c.want) if want is None else want
    r, ref = operands if operands else (R.recipe_dgrad1(c.M, c.K, dense), R.reference_dgrad1(c.M, c.K, s, dense))
    dBb = Buf(r.dB if dB is None else dB, c.M, 128, 'rows', -4321.0, extra=0)
    W1t = Plain(r.W1.t())
    X = Buf(r.X, c.M, c.K, c.lay, 1234.0)
    G = Buf(r.G0, c.M, c.K, c.lay, -999.0, pad=7)
    bn = bn_vecs(r.bn, c.K)
    outs = dict(G=(G, ref['G']))
    ptrs = dict(dgamma=None, dbeta=None, dW=None)
    for key, name, prior in (('g', 'dgamma', r.dg0), ('b', 'dbeta', r.db0)):
        if key in want:
            outs[name] = (vec(None, c.K, prior, acc), R.with_prior(ref[name], prior) if acc else ref[name])
            ptrs[name] = outs[name][0].ptr
    if wg:
        outs['dW'] = (framed(r.dW0, 128 * c.K, acc), R.with_prior(ref['dW'], r.dW0) if acc else ref['dW'])
        ptrs['dW'] = outs['dW'][0].ptr
    nws = L.query('gnx_conv1x1_dgrad_wgrad_f16_workspace' if wg else 'gnx_conv1x1_dgrad_bnrelu_bwd_f16_workspace', c.M, c.K)
    assert nws == R.ws_dgrad1(c.M, c.K, wg)
    ws, ls, fl = Workspace(nws), ls_tensor(s), Flag() if flag else None
    slabs, cw = R.plan_dgrad1(c.M, c.K, wg).slabs, -(-c.K // 128) * 128

    def ws_ok(t):
        bnp = t[:slabs * 2 * cw].view(slabs, 2, cw)
        ok = no_nan(bnp[:, :, :c.K]) and (c.K == cw or all_nan(bnp[:, :, c.K:]))
        if wg:                                                  # (the columns past K of the weight-gradient slabs are exempt)
            ok = ok and no_nan(t[slabs * 2 * cw:].view(slabs, 128, cw)[:, :, :c.K])
        return ok and t.numel() == slabs * (130 if wg else 2) * cw
    p = dict(dB16=dBb.ptr, W1t16=W1t.ptr, X16=X.ptr, ldx=X.ld, bsx=X.bs, G16=G.ptr, ldg=G.ld, bsg=G.bs, M=c.M, K=c.K, scale=bn[0].ptr,
             shift=bn[1].ptr, mean=bn[2].ptr, invstd=bn[3].ptr, dgamma=ptrs['dgamma'], dbeta=ptrs['dbeta'], dW=ptrs['dW'],
             workspace=ws.ptr, ls=ls.data_ptr(), accumulate=acc, flag=P(fl))
    return Call('gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_lb', 'gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_form', 3, R.form_dgrad1, p,
                [dBb, W1t, X] + bn, outs, ws, ws_ok, ls, fl)


def _bn_outs(r, ref, C, acc):
    outs = {}
    for name, prior in (('dgamma', r.dg0), ('dbeta', r.db0)):
        outs[name] = (vec(None, C, prior, acc), R.with_prior(ref[name], prior) if acc else ref[name])
    return outs


def build_tail(c, acc=0, s=1.0, dfeats=None, flag=True):
    r = R.recipe_tail(c.imgs, c.C, c.S2)
    ref = R.reference_tail(c.imgs, c.C, c.S2, s)
    df = Buf(r.dfeats if dfeats is None else dfeats, c.imgs, c.C, 'rows', -4321.0, extra=8, off=4, dtype=torch.float32)
    X = Buf(r.X, r.M, c.C, c.lay, 1234.0)
    G = Buf(None, r.M, c.C, c.lay, -999.0, pad=7)
    bn = bn_vecs(r.bn, c.C)
    outs = _bn_outs(r, ref, c.C, acc)
    outs['G'] = (G, ref['G'])
    nws = L.query('gnx_tail_bwd_f16_workspace', c.imgs, c.C)
    assert nws == R.ws_tail(c.imgs, c.C)
    ws, ls, fl = Workspace(nws), ls_tensor(s), Flag() if flag else None
    p = dict(dfeats=df.ptr, ldf=df.ld, X16=X.ptr, ldx=X.ld, bsx=X.bs, G16=G.ptr, ldg=G.ld, bsg=G.bs, imgs=c.imgs, C=c.C, S2=c.S2,
             scale=bn[0].ptr, shift=bn[1].ptr, mean=bn[2].ptr, invstd=bn[3].ptr, dgamma=outs['dgamma'][0].ptr, dbeta=outs['dbeta'][0].ptr,
             workspace=ws.ptr, ls=ls.data_ptr(), accumulate=acc, flag=P(fl))
    return Call('gnx_tail_bwd_f16_lb', 'gnx_tail_bwd_f16_form', 3, R.form_tail, p, [df, X] + bn, outs, ws, first_floats(nws), ls, fl)


def build_trans(c, acc=0, s=1.0, dP=None, flag=True):
    r = R.recipe_trans(c.imgs, c.C, c.S)
    ref = R.reference_trans(c.imgs, c.C, c.S, s)
    Mp = c.imgs * (c.S // 2) ** 2
    dPb = Buf(r.dP if dP is None else dP, Mp, c.C, c.lay, -4321.0, pad=3)
    X = Buf(r.X, r.M, c.C, c.lay, 1234.0)
    G = Buf(None, r.M, c.C, c.lay, -999.0, pad=7)
    assert c.lay == 'rows' or len({dPb.bs, X.bs, G.bs}) == 3
    bn = bn_vecs(r.bn, c.C)
    outs = _bn_outs(r, ref, c.C, acc)
    outs['G'] = (G, ref['G'])
    nws = L.query('gnx_trans_bwd_f16_workspace', c.imgs, c.C, c.S)
    assert nws == R.ws_trans(c.imgs, c.C, c.S)
    ws, ls, fl = Workspace(nws), ls_tensor(s), Flag() if flag else None
    p = dict(dP16=dPb.ptr, ldp=dPb.ld, bsp=dPb.bs, X16=X.ptr, ldx=X.ld, bsx=X.bs, G16=G.ptr, ldg=G.ld, bsg=G.bs, imgs=c.imgs, C=c.C,
             S=c.S, scale=bn[0].ptr, shift=bn[1].ptr, mean=bn[2].ptr, invstd=bn[3].ptr, dgamma=outs['dgamma'][0].ptr,
             dbeta=outs['dbeta'][0].ptr, workspace=ws.ptr, ls=ls.data_ptr(), accumulate=acc, flag=P(fl))
    return Call('gnx_trans_bwd_f16_lb', 'gnx_trans_bwd_f16_form', 3, R.form_trans, p, [dPb, X] + bn, outs, ws, first_floats(nws), ls, fl)


def build_h16(c, act):
    r = R.recipe_h16(c.M, c.N, c.K)
    ref = R.reference_h16(c.M, c.N, c.K, act)['out']
    A = Buf(r.X, c.M, c.K, 'rows', 1234.0)
    W = Plain(r.W)
    out = Buf(None, c.M, c.N, 'blocked' if c.cb else 'rows', -999.0)
    vs = [vec(r.pro[0], c.K), vec(r.pro[1], c.K), vec(r.con[0], c.N), vec(r.con[1], c.N)] if act else [None] * 4
    p = dict(A16=A.ptr, lda16=A.ld, W16=W.ptr, out16=out.ptr, ldc16=out.ld, rows_total=out.rows_total, M=c.M, N=c.N, K=c.K,
             scale=P(vs[0]), shift=P(vs[1]), out_scale=P(vs[2]), out_shift=P(vs[3]))
    name = 'gnx_conv1x1_bnrelu_h16' + ('_cb' if c.cb else '')
    return Call(name, name + '_form', 1, lambda a: R.form_h16(a, c.cb), p, [A, W] + [v for v in vs if v], dict(out=(out, ref)), None,
                None, None, None)


# ------------------------------------------------------------------------------------------------- 1. the whole grid
@pytest.mark.parametrize("c", R.WG1_GRID, ids=R.ids)
def test_wgrad1x1(c):
    for pro in (0, 1):
        full_case(lambda acc, s: build_wgrad1(c, pro, acc, s), 'wgrad1 %s pro %d' % (R.ids(c), pro))


@pytest.mark.parametrize("c", R.WG3_GRID, ids=R.ids)
def test_wgrad3x3(c):
    for lay in ('rows', 'blocked'):
        full_case(lambda acc, s: build_wgrad3(c, lay, acc, s), 'wgrad3 %s %s' % (R.ids(c), lay))
    if R.thinned('wgrad3', c):
        full_case(lambda acc, s: build_wgrad3(c, 'blocked', acc, s, dense=True), 'wgrad3 %s dense' % R.ids(c))


@pytest.mark.parametrize("c", R.DG3_GRID, ids=R.ids)
def test_conv3x3_dgrad(c):
    for lay in (('rows', 'blocked') if R.rows_of('dgrad3', c) <= 4096 else ('blocked',)):
        full_case(lambda acc, s: build_dgrad3(c, lay, acc, s), 'dgrad3 %s %s' % (R.ids(c), lay))
    if R.thinned('dgrad3', c):                                 # dB on a half-live mask at the same shape and plan
        full_case(lambda acc, s: build_dgrad3(c, 'blocked', acc, s, dense=True), 'dgrad3 %s dense' % R.ids(c))


@pytest.mark.parametrize("c", R.C3_GRID, ids=R.ids)
def test_conv3x3_bwd_one_pass(c):
    full_case(lambda acc, s: build_conv3(c, acc, s), 'conv3 ' + R.ids(c))
    if R.thinned('conv3', c):
        full_case(lambda acc, s: build_conv3(c, acc, s, dense=True), 'conv3 %s dense' % R.ids(c))


@pytest.mark.parametrize("c", R.DG1_GRID, ids=R.ids)
def test_conv1x1_dgrad(c):
    for wg in (0, 1):
        full_case(lambda acc, s: build_dgrad1(c, wg, acc, s), 'dgrad1 %s dW %d' % (R.ids(c), wg))
        if R.thinned('dgrad1', c):                             # G and dW1 on a half-live mask at the same shape and plans
            full_case(lambda acc, s: build_dgrad1(c, wg, acc, s, dense=True), 'dgrad1 %s dW %d dense' % (R.ids(c), wg))


def test_conv1x1_dgrad_is_bit_equal_with_and_without_the_weight_gradient():
    """M = 64 * 600 + 7, K = 32: 601 slabs of one tile without dW, 301 of two with it; G does not depend on the slab plan."""
    c = [k for k in R.DG1_GRID if k.edge == 'per1-per2'][0]
    assert (R.plan_dgrad1(c.M, c.K, False).per, R.plan_dgrad1(c.M, c.K, True).per) == (1, 2)
    a, b = run(build_dgrad1(c, 0), 'per 1', compare=False), run(build_dgrad1(c, 1), 'per 2', compare=False)
    assert torch.equal(a['G'], b['G'])


@pytest.mark.parametrize("c", R.TAIL_GRID, ids=R.ids)
def test_tail(c):
    full_case(lambda acc, s: build_tail(c, acc, s), 'tail ' + R.ids(c))


@pytest.mark.parametrize("c", R.TRANS_GRID, ids=R.ids)
def test_trans(c):
    full_case(lambda acc, s: build_trans(c, acc, s), 'trans ' + R.ids(c))


@pytest.mark.parametrize("c", R.H16_GRID, ids=R.ids)
def test_conv1x1_h16(c):
    failed = []
    for act in (0, 1):
        try:
            what = 'h16 %s act %d' % (R.ids(c), act)
            got = run(build_h16(c, act), what)
            assert torch.equal(got['out'], run(build_h16(c, act), what, compare=False)['out']), what + ': a second call gives other bits'
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)


def test_conv1x1_h16_without_rows_launches_nothing():
    call = build_h16(R.H16('small', 1, 8, 8, 0), 0)
    assert call.query(M=0) == (R.CODES['M128'], 0)
    call.launch(M=0)
    assert call.untouched()


@pytest.mark.parametrize("c", R.COLS_GRID, ids=R.ids)
def test_h16_cols_to_f32(c):
    g = torch.Generator().manual_seed(c.M)
    Gv = R._signed(g, 0.5, 1.5, c.M, c.C)
    for s in (1.0, 4096.0):
        G = Buf(Gv, c.M, c.C, 'rows', 1234.0)
        out = Buf(None, c.M, c.C, 'rows', -999.0, extra=12, off=4, dtype=torch.float32)
        ls, fl = ls_tensor(s), Flag()
        L.call('gnx_h16_cols_to_f32', G.ptr, G.ld, out.ptr, out.ld, c.M, c.C, ls.data_ptr(), fl.ptr, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(out.get().double(), Gv / s) and out.outside_unchanged() and G.unchanged() and fl.value() == 0, (c, s)
    for row in (0, c.M - 1):
        bad = Gv.clone()
        bad[row, c.C - 1] = float('inf')
        G, fl = Buf(bad, c.M, c.C, 'rows', 1234.0), Flag()
        L.call('gnx_h16_cols_to_f32', G.ptr, G.ld, out.ptr, out.ld, c.M, c.C, ls.data_ptr(), fl.ptr, L.stream())
        torch.cuda.synchronize()
        assert fl.value() == 1, (c, row)
    L.call('gnx_h16_cols_to_f32', G.ptr, G.ld, out.ptr, out.ld, c.M, c.C, ls.data_ptr(), None, L.stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 2. the loss scale
def test_loss_scale_2_to_the_12():
    s = ((0, 4096.0), (1, 4096.0))
    full_case(lambda acc, k: build_wgrad1(R.WG1_GRID[4], 1, acc, k), 'wgrad1 s', s)
    full_case(lambda acc, k: build_wgrad3(R.WG3_GRID[7], 'blocked', acc, k), 'wgrad3 s', s)
    full_case(lambda acc, k: build_dgrad3(R.DG3_GRID[6], 'blocked', acc, k), 'dgrad3 s', s)
    full_case(lambda acc, k: build_conv3(R.C3_GRID[0], acc, k), 'conv3 s', s)
    full_case(lambda acc, k: build_dgrad1(R.DG1_GRID[3], 1, acc, k), 'dgrad1 s', s)
    full_case(lambda acc, k: build_tail(R.TAIL_GRID[4], acc, k), 'tail s', s)
    full_case(lambda acc, k: build_trans(R.TRANS_GRID[3], acc, k), 'trans s', s)


# ------------------------------------------------------------------------------------------------- 3. the flag
def _poisoned(v, row, col):
    """ONE infinity: a reduce must raise the flag from whichever lane and block owns the result it reaches."""
    v = v.clone()
    v[row, col] = float('inf')
    assert int(torch.isinf(v).sum()) == 1
    return v


def _live_col(X, bn, rows, start):
    """The first channel from `start` on (never lane 0 of a 16-channel block) whose pre-activation is positive in one of `rows`: an
    infinity there passes the mask."""
    z = R.act16(X, bn.scale, bn.shift)[1][rows]
    return next(c for c in list(range(start, z.shape[1])) + list(range(start)) if c % 16 and bool((z[:, c] > 0).any()))


def _flag_runs(name, build, grad, spots):
    """`build(grad=..., flag=...)` -> Call.  One infinity at each (row, column) of `spots` - the first and the last valid row,
    columns that are not lane 0 of a reduce block - raises the flag; flag = NULL completes with the same outputs; 60000
    everywhere leaves the flag at 0."""
    assert len({col for _, col in spots}) == len(spots) and all(col % 16 for _, col in spots)
    for row, col in spots:
        call = build(grad=_poisoned(grad, row, col), flag=True)
        call.launch()
        assert call.flag.value() == 1, '%s: an infinity at row %d, column %d left the flag at 0' % (name, row, col)
    with_flag, without = build(grad=None, flag=True), build(grad=None, flag=False)
    a, b = run(with_flag, name + ' with a flag'), run(without, name + ' flag NULL')
    for k in a:
        assert torch.equal(a[k], b[k]), '%s: flag = NULL changes %s' % (name, k)
    call = build(grad=torch.full_like(grad, 60000.0), flag=True)
    call.launch()
    assert call.flag.value() == 0, name + ': finite sums of 60000s raised the flag'


def test_flag_of_the_slab_reduce():
    """reduce_slabs_kernel in its three index maps, each alone: no BatchNorm sums are asked for where the entry point allows."""
    c = R.Wg1('ragged', 65, 8, 8)
    _flag_runs('wgrad1', lambda grad, flag: build_wgrad1(c, 1, dY=grad, flag=flag), R.recipe_wgrad1(c).dY, ((0, 5), (c.M - 1, 3)))
    c = R.Wg3('generic-pow2-ragged', 5, 4)
    _flag_runs('wgrad3', lambda grad, flag: build_wgrad3(c, 'blocked', dY=grad, flag=flag), R.recipe_conv2(5, 4).dY, ((0, 7), (79, 29)))
    c = R.Dg1('ragged', 65, 96, 'rows', '')
    _flag_runs('dgrad1 dW', lambda grad, flag: build_dgrad1(c, 1, dB=grad, flag=flag), R.recipe_dgrad1(65, 96).dB, ((0, 21), (64, 127)))
    c = R.C3('tiles-1', 8, 4, 'blocked')
    _flag_runs('conv3 dW', lambda grad, flag: build_conv3(c, dY=grad, flag=flag, want=''), R.recipe_conv2(8, 4).dY, ((0, 9), (127, 18)))


def test_flag_of_the_batchnorm_reduce():
    """bn_reduce_kernel in both modes and with and without a loss scale, alone: no weight gradient is asked for."""
    c = R.Dg3('generic-pow2-ragged', 3, 8, 'gb')
    _flag_runs('dgrad3', lambda grad, flag: build_dgrad3(c, 'rows', dY=grad, flag=flag), R.recipe_conv2(3, 8).dY, ((0, 13), (191, 6)))
    c = R.Dg1('ragged', 65, 96, 'blocked', 'gb')
    _flag_runs('dgrad1', lambda grad, flag: build_dgrad1(c, 0, dB=grad, flag=flag), R.recipe_dgrad1(65, 96).dB, ((0, 2), (64, 77)))
    c = R.Tail('blocked-16', 17, 32, 4, 'blocked')
    r = R.recipe_tail(17, 32, 4)
    spots = ((0, _live_col(r.X, r.bn, slice(0, 4), 5)), (16, _live_col(r.X, r.bn, slice(64, 68), 19)))
    _flag_runs('tail', lambda grad, flag: build_tail(c, dfeats=grad, flag=flag), r.dfeats, spots)
    c = R.Trans('blocked-16', 17, 32, 2, 'blocked')
    r = R.recipe_trans(17, 32, 2)
    spots = ((0, _live_col(r.X, r.bn, slice(0, 4), 9)), (16, _live_col(r.X, r.bn, slice(64, 68), 23)))
    _flag_runs('trans', lambda grad, flag: build_trans(c, dP=grad, flag=flag), r.dP, spots)


# ------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_write_nothing():
    c = R.Wg1('ragged', 65, 8, 8)
    call = build_wgrad1(c, 1)
    for kw, code in ((dict(lddy=0), BAD_ARG), (dict(shift=None), BAD_ARG), (dict(M=0), BAD_ARG), (dict(ls=None), BAD_ARG),
                     (dict(workspace=None), BAD_ARG), (dict(N=4), UNSUPPORTED), (dict(ldx=call.p['ldx'] + 4), UNSUPPORTED),
                     (dict(X16=call.p['X16'] + 8), UNSUPPORTED)):
        refuse(call, kw, code, 'wgrad1')
    c3 = R.Wg3('padded', 4, 4)
    for call, fam in ((build_wgrad3(c3, 'rows'), 'wgrad3'), (build_dgrad3(R.Dg3('padded', 8, 4, 'gb'), 'rows'), 'dgrad3')):
        for kw, code in ((dict(S=65, M=4225), UNSUPPORTED), (dict(M=call.p['M'] - 1), BAD_ARG), (dict(lda=call.p['lda'] + 4), UNSUPPORTED),
                         (dict(A16=None), BAD_ARG), (dict(dY16=call.p['dY16'] + 8), UNSUPPORTED)):
            refuse(call, kw, code, fam)
    call = build_conv3(R.C3('tiles-1', 8, 4, 'rows'))
    for kw, code in ((dict(S=7, M=49 * 128), UNSUPPORTED), (dict(M=64), UNSUPPORTED), (dict(M=192), UNSUPPORTED), (dict(dW=None), BAD_ARG),
                     (dict(S=3, M=128), BAD_ARG)):
        refuse(call, kw, code, 'conv3')
    for lay in ('rows', 'blocked'):
        call = build_dgrad1(R.Dg1('ragged', 65, 96, lay, 'gb'), 1)
        runs = [(dict(K=40), UNSUPPORTED), (dict(ldx=call.p['ldx'] + 4), UNSUPPORTED), (dict(ldg=call.p['ldg'] + 4), UNSUPPORTED),
                (dict(X16=call.p['X16'] + 8), UNSUPPORTED), (dict(G16=call.p['G16'] + 8), UNSUPPORTED),
                (dict(dB16=call.p['dB16'] + 8), UNSUPPORTED), (dict(M=0), BAD_ARG), (dict(mean=None), BAD_ARG)]
        if lay == 'blocked':
            runs += [(dict(bsx=call.p['bsx'] + 4), UNSUPPORTED), (dict(bsg=call.p['bsg'] + 4), UNSUPPORTED), (dict(bsx=16), BAD_ARG)]
        else:
            runs += [(dict(ldx=88), BAD_ARG)]
        for kw, code in runs:
            refuse(call, kw, code, 'dgrad1 ' + lay)
    call = build_tail(R.Tail('rows-C8', 5, 8, 4, 'rows'))
    for kw, code in ((dict(ldf=4), BAD_ARG), (dict(S2=0), BAD_ARG), (dict(C=4, ldf=4), UNSUPPORTED), (dict(bsx=64), UNSUPPORTED),
                     (dict(dfeats=call.p['dfeats'] + 8), UNSUPPORTED)):
        refuse(call, kw, code, 'tail')
    call = build_trans(R.Trans('rows-C8', 5, 8, 4, 'rows'))
    for kw, code in ((dict(S=1), BAD_ARG), (dict(S=3), UNSUPPORTED), (dict(bsp=64), UNSUPPORTED), (dict(ldp=call.p['ldp'] + 4), UNSUPPORTED),
                     (dict(dP16=None), BAD_ARG)):
        refuse(call, kw, code, 'trans')
    for cb in (0, 1):
        call = build_h16(R.H16('small', 130, 32, 64, cb), 1)
        runs = [(dict(lda16=56), BAD_ARG), (dict(out_shift=None), BAD_ARG), (dict(K=4), UNSUPPORTED), (dict(A16=call.p['A16'] + 8), UNSUPPORTED),
                (dict(scale=call.p['scale'] + 8), UNSUPPORTED)]
        runs += [(dict(rows_total=129), BAD_ARG), (dict(N=40), BAD_ARG)] if cb else [(dict(ldc16=24), BAD_ARG), (dict(N=36), UNSUPPORTED)]
        for kw, code in runs:
            refuse(call, kw, code, 'h16 cb %d' % cb)


# ------------------------------------------------------------------------------------- 5. a pre-activation of exactly 0
def test_a_pre_activation_of_exactly_zero_passes_no_gradient():
    """relu'(0) = 0: fma(x, scale, shift) == 0 exactly (scale = +-1, shift = +-0.5, x = -+0.5) on an eighth of the elements of
    conv1's backward; the masks say `> 0`.  Outside bwd_f16_ref.GRID: its recipe keeps every pre-activation away from 0."""
    c = R.Dg1('ragged', 130, 96, 'rows', 'gb')
    r = R.recipe_dgrad1(c.M, c.K)
    g = torch.Generator().manual_seed(5)
    sign = lambda *shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    scale, shift = sign(c.K), 0.5 * sign(c.K)
    zero = torch.rand(c.M, c.K, generator=g) < 0.125
    X = torch.where(zero, -shift / scale, r.X.sign() * (r.X.abs() + 0.25))
    bn = NS(scale=scale, shift=shift, mean=r.bn.mean, invstd=r.bn.invstd)
    z = R.act16(X, scale, shift)[1]
    assert bool((z[zero] == 0).all()) and int(zero.sum()) > 1000 and z[~zero].abs().min().item() >= 0.25
    ref = R.dgrad1(r.dB, r.W1, X, r.G0, bn)
    mine = NS(dB=r.dB, W1=r.W1, X=X, G0=r.G0, bn=bn, dW0=r.dW0, dg0=r.dg0, db0=r.db0)
    for wg in (0, 1):
        run(build_dgrad1(c, wg, operands=(mine, ref)), 'dgrad1 with zero pre-activations, dW %d' % wg)


# ------------------------------------------------------------------------------------------------- where G comes from
def _device_mm(A, B):
    return torch.matmul(A.float().to(DEV), B.float().to(DEV))


@pytest.mark.parametrize("fc", [(fam, c) for fam, cases in R.GRID.items() if fam != 'cols' for c in cases],
                         ids=lambda fc: fc[0] + '-' + R.ids(fc[1]))
def test_plain_fp32_matmul_stays_within_the_ratio_G_was_set_from(fc, capsys):
    """The device half of the measurement behind bwd_f16_ref.G, kept runnable: every contraction of the case as an fp32
    torch.matmul on the device against float64, max |err| / (2^-24 T).  A torch whose GEMM rounds differently fails here with
    the figure to set TORCH_FP32_RATIO (and with it G) from."""
    ratio, name = R.plain_ratio(fc[0], fc[1], _device_mm)
    with capsys.disabled():
        print(' torch fp32 ratio at %s-%s: %.4f (%s)' % (fc[0], R.ids(fc[1]), ratio, name))
    assert ratio <= R.TORCH_FP32_RATIO, (ratio, name)


def test_report_worst_ratio_per_body_and_that_every_body_ran(capsys):
    """Prints what the tests above saw: per kernel body the largest |err| / tolerance and the number of runs.  After the whole
    file every body of DESIGN.md's "fp16 backward forms" is among the answers of the form queries (alone: nothing ran)."""
    with capsys.disabled():
        print('\n G = %.3f (torch fp32 %.4f at %s; fp32 chain %.4f at %s)' % (R.G, R.TORCH_FP32_RATIO, R.TORCH_FP32_AT,
                                                                            R.CHAIN_FP32_RATIO, R.CHAIN_FP32_AT))
        for body, (worst, n) in sorted(WORST.items()):
            print(' %-8s worst |err| / tolerance %.4f over %d runs' % (body, worst, n))
    assert all(w <= 1.0 for w, _ in WORST.values())
    assert not SEEN or SEEN == set(R.CODES.values()), sorted(R.NAMES[k] for k in set(R.CODES.values()) - SEEN)
