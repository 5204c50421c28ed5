"""Every kernel form of csrc/stem_pool.hip - the stem convolutions, the fused conv0 + norm0 + relu0 + pool0 kernels, the BN + ReLU
max and average pools and the uint8 converter - through the C ABI against the float64 references of tests/stem_ref.py, over
stem_ref.GRID: the smallest shapes at which each form can go wrong (one tile with both edges in a window, odd H, every slot of
the fp16 kernel's row ring, O of 4 and 36, a window of a wider buffer, more images / tiles / blocks than a launch's cap, index
lists with repeats and out-of-range entries, every part of the 16-byte condition broken alone) and the geometries that ship.

Every output is a window of a NaN- (bytes: 0xAB-) filled buffer between two frames: an element not written shows as NaN, a write
outside the window as a changed frame; operands stay alive (and on the device) across the raw-pointer calls.

Kind 1 (integer-exact operands): the bits of the float64 reference, values and window indices, ties included.  Kind 2: within
the per-element tolerance of stem_ref (G from plain fp32 evaluations of the reference operation, not from the kernel); indices
where the reference's two largest window values are further apart than their tolerances.  Relations the code promises: uint8 ==
float on torch-converted patches, _h16 == .half() of fp32, _argmax values == plain, _idx == plain on a gathered copy, channel-
blocked == row-major re-laid, an image alone == that image in the batch.  Refusals: each condition alone, the code, an untouched
output, then the accepted call.  In front of every call, the library's query (gnx_conv_stem_form, gnx_conv_stem_pool_form,
gnx_conv_stem_pool_f16mul_form, gnx_bnrelu_maxpool_form) is asked with the call's device pointers and must name the body and the
workgroups that stem_ref's mirror of the dispatch names.

Measured on an MI355X, kind 2, the largest |err| / tolerance over the fused cases: 0.23 with fp32 stores (the kernels' own
|err| / (2^-24 T) is about 4, what the plain fp32 chain on the CPU gives), 0.99 with fp16 stores (the half ulp of the store)."""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

import stem_ref as R
from gridnext_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FRAME = 64
NAN = float('nan')
BYTE = 0xAB
CODE = {'bad_arg': -1, 'unsupported': -3, R.EMPTY: 0}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.uint8: torch.uint8}

FUSED = [c for c in R.GRID if isinstance(c, R.Fused)]
STEMS = [c for c in R.GRID if isinstance(c, R.Stem)]
POOLS = [c for c in R.GRID if isinstance(c, R.Pool)]
AVGS = [c for c in R.GRID if isinstance(c, R.Avg)]
U8S = [c for c in R.GRID if isinstance(c, R.U8)]


def bits(t):
    return t.view(BITS[t.dtype])


class Buf:
    """n elements of `dtype`, filled with NaN (bytes: 0xAB), between two frames; the window starts `off` elements past a 16-B
    boundary."""

    def __init__(self, n, dtype=torch.float32, off=0, data=None):
        self.store = torch.full((n + 2 * FRAME + 8,), BYTE if dtype == torch.uint8 else NAN, dtype=dtype, device=DEV)
        assert self.store.data_ptr() % 16 == 0
        self.lo, self.n = FRAME + off, n
        self.win = self.store[self.lo:self.lo + n]
        if data is not None:
            self.win.copy_(data.reshape(-1))
        self.before = self.store.clone()

    @property
    def ptr(self):
        return self.win.data_ptr()

    def frames_unchanged(self):
        s, b = bits(self.store), bits(self.before)
        return torch.equal(s[:self.lo], b[:self.lo]) and torch.equal(s[self.lo + self.n:], b[self.lo + self.n:])

    def untouched(self):
        return torch.equal(bits(self.store), bits(self.before))


def cargs(entry, a, P):
    """The C argument list of an entry point from the scalars `a` and the pointers `P` (by name; None: NULL)."""
    st = (L.stream(),)
    if entry in R.FUSED_ENTRIES:
        geo = (a['imgs'], a['Cin'], a['H'], a['W'], a['O'], a['KH'], a['KW'], a['stride'], a['pad'], P['scale'], P['shift'])
        head = (P['x'], P['w'], P['out'], a['ldo'])
        if entry in ('f32', 'h16'):
            return head + geo + st
        if entry == 'idx':
            return head + geo + (P['idx'], a['src_imgs']) + st
        if entry == 'argmax':
            return head + (P['amax'],) + geo + st
        if entry in ('u8', 'u8_h16'):
            return head + geo + (P['norm'], int(entry == 'u8_h16')) + st
        if entry == 'u8_idx':
            return head + geo + (P['norm'], P['idx'], a['src_imgs']) + st
        ld = a['rows_total'] if entry in R.IS_CB else a['ldo']
        return (P['x'], int(entry in R.IS_U8), P['w'], P['out'], ld) + geo + (P['norm'],) + st
    if entry == 'conv_stem':
        return (P['x'], P['w'], P['out'], a['ldc'], a['imgs'], a['Cin'], a['H'], a['W'], a['O'], a['KH'], a['KW'], a['stride'],
                a['pad']) + st
    if entry in ('maxpool', 'maxpool_argmax'):
        am = (P['amax'],) if entry == 'maxpool_argmax' else ()
        return (P['in'], a['ldi'], P['out'], a['ldo']) + am + (a['imgs'], a['C'], a['Hi'], a['Wi'], P['scale'], P['shift']) + st
    if entry.startswith('avgpool.'):
        ld = a['rows_total'] if entry == 'avgpool.h16_cb' else a['ldi']
        tail = (P['idx'], a['dst_rows']) if entry == 'avgpool.idx' else ()
        return (P['in'], ld, P['out'], a['ldo'], a['imgs'], a['C'], a['S2'], P['scale'], P['shift']) + tail + st
    if entry == 'u8_to_f32':
        return (P['x'], P['out'], a['imgs'], a['C'], a['H'], a['W'], P['norm']) + st
    raise KeyError(entry)


NAME = dict(R.ENTRY_POINT, conv_stem='gnx_conv_stem', maxpool='gnx_bnrelu_maxpool', maxpool_argmax='gnx_bnrelu_maxpool_argmax',
            u8_to_f32='gnx_u8_to_f32', **{'avgpool.' + e: 'gnx_bnrelu_avgpool' + ('' if e == 'f32' else '_' + e)
                                          for e in ('f32', 'idx', 'h16', 'h16_cb')})


def asked(entry, a, P):
    """The library's query for this call, asked with the call's own pointers: it answers as the mirror does (the GNX_* code and the
    workgroups of R.query_answer).  Returns the mirror's form name; an entry with one body has no query."""
    q = R.query_call(entry, a, P)
    b = dict(a, **{k: None if P.get(k) is None else P[k] % 16 for k in R.POINTERS})
    form = R.form_of_call(entry, b)
    if q is not None:
        want = R.query_answer(entry, b)
        wg = ctypes.c_int(-7)
        got = L.query(q[0], *q[1], ctypes.addressof(wg)), wg.value
        assert got == (L.CONSTANTS[want[0]], want[1]), '%s %s: %s says %s, the mirror %s (%s)' % (entry, a, q[0], got, want, form)
    return form


def run(entry, a, P):
    form = asked(entry, a, P)
    assert form in R.FORMS, (entry, a, form)
    L.call(NAME[entry], *cargs(entry, a, P))
    torch.cuda.synchronize()
    return form


# ------------------------------------------------------------------------------------------------------------ fused stems
def launch_fused(entry, c, x, inp, imgs, lst=None):
    """One launch of a fused entry point on the device patches x (float32 or uint8): NS(rows [imgs Hp Wp][O] on the host, amax
    [rows][O] or None).  The frames and the buffer around the written window are checked here."""
    _, _, hp, wp = R.fused_sizes(c)
    M, O = imgs * hp * wp, c.O
    dt = torch.float16 if entry in R.IS_H16 else torch.float32
    cb, wide = entry in R.IS_CB, c.ldo > c.O
    total = M + (5 if wide else 0)
    ldo, col0 = (32, 0) if cb else (c.ldo, 4 if wide else 0)
    out = Buf((O // 32) * total * 32 if cb else M * ldo, dt)
    amax = Buf(M * O, torch.uint8) if entry == 'argmax' else None
    w, scale, shift = inp.w.to(DEV), inp.scale.to(DEV), inp.shift.to(DEV)
    norm = R.norm_vector().to(DEV) if (inp.norm and entry in R.IS_U8) else None
    idx = torch.tensor(lst, dtype=torch.int32, device=DEV) if lst is not None else None
    assert x.is_contiguous() and x.dtype == (torch.uint8 if entry in R.IS_U8 else torch.float32)
    a = dict(imgs=imgs, Cin=3, H=c.H, W=c.W, O=O, KH=7, KW=7, stride=2, pad=3, ldo=ldo, src_imgs=x.shape[0], rows_total=total)
    P = dict(x=x.data_ptr(), w=L.ptr(w), out=out.ptr + col0 * out.win.element_size(), scale=L.ptr(scale), shift=L.ptr(shift),
             norm=None if norm is None else L.ptr(norm), amax=None if amax is None else amax.ptr,
             idx=None if idx is None else idx.data_ptr())
    form = run(entry, a, P)
    assert out.frames_unchanged() and (amax is None or amax.frames_unchanged())
    assert torch.equal(w.cpu(), inp.w) and torch.equal(scale.cpu(), inp.scale) and torch.equal(shift.cpu(), inp.shift)
    flat = out.win.cpu()
    if cb:
        rows = R.from_cb(flat, M, O, total)
        written = ~torch.isnan(R.to_cb(torch.zeros(M, O), total))
        assert bool(torch.isnan(flat[~written]).all()), 'a write between the blocks of the channel-blocked buffer'
    else:
        mat = flat.view(M, ldo)
        rows = mat[:, col0:col0 + O]
        assert bool(torch.isnan(mat[:, :col0]).all()) and bool(torch.isnan(mat[:, col0 + O:]).all()), 'a write past column O'
    return NS(rows=rows.contiguous(), amax=None if amax is None else amax.win.cpu().view(M, O), form=form)


def device_patches(c, kind):
    """(x on the device as the entry is given it, the index list or None): an index-list entry gets the case's distinct patches
    and its list, every other entry the batch itself."""
    inp = R.fused_inputs(c, kind)
    xd = inp.x.to(DEV)
    if c.entry in R.IS_IDX:
        return xd, R.src_list(c)
    return xd[torch.tensor(R.image_map(c), device=DEV)].contiguous(), None


def check_fused(c, kind):
    inp, ref = R.fused_inputs(c, kind), R.fused_reference(c, kind)
    m = torch.tensor(R.image_map(c))
    x, lst = device_patches(c, kind)
    got = launch_fused(c.entry, c, x, inp, c.imgs, lst)
    want, O = ref.val[m].reshape(-1, c.O), c.O
    if kind == 'int':
        assert torch.equal(got.rows.double(), want), 'kind 1: not the bits of the float64 reference'
        if got.amax is not None:
            assert not R.idx_flagged(got.amax, ref.idx[m].reshape(-1, O)), 'kind 1: a window index differs (ties included)'
    else:
        tol = ref.tol[m].reshape(-1, O)
        if c.entry not in R.IS_U8:
            assert R.detectable(tol)
        assert not R.flagged(got.rows, want, tol), float(((got.rows.double() - want).abs() / tol).max())
        if got.amax is not None:
            cmp = ref.comparable[m].reshape(-1, O)
            assert R.excluded(cmp) <= R.MAX_EXCLUDED and int(got.amax.max()) <= 8
            assert not R.idx_flagged(got.amax, ref.idx[m].reshape(-1, O), cmp)
    return got, x, lst, inp


@pytest.mark.parametrize('c', FUSED, ids=R.ids)
def test_fused_stem_against_float64(c):
    assert check_fused(c, 'int')[0].form == R.form_of(c)
    got, x, lst, inp = check_fused(c, 'mag')
    # the entry this one must reproduce bit for bit
    cp = R.COUNTERPART.get(c.entry)
    if cp is not None:
        xc, lc = x, lst
        if c.entry in R.IS_U8 and cp not in R.IS_U8:
            xc = R.to_tensor(x.cpu(), inp.norm).to(DEV).contiguous()
        if c.entry in R.IS_IDX and cp not in R.IS_IDX:
            xc, lc = R.gather(xc.cpu(), lst).to(DEV).contiguous(), None
        other = launch_fused(cp, c, xc, inp, c.imgs, lc)
        rows = other.rows.half() if (c.entry in R.IS_H16 and cp not in R.IS_H16) else other.rows
        assert torch.equal(bits(got.rows), bits(rows)), '%s differs from %s' % (c.entry, cp)
    # an image alone: the bits it has in the batch
    if c.imgs == 3:
        _, _, hp, wp = R.fused_sizes(c)
        one = launch_fused(c.entry, c, x[1:2].contiguous(), inp, 1)
        assert torch.equal(bits(one.rows), bits(got.rows[hp * wp:2 * hp * wp])), 'image 1 alone differs from image 1 of the batch'
        if one.amax is not None:
            assert torch.equal(one.amax, got.amax[hp * wp:2 * hp * wp])
    # a second launch: the same bits
    again = launch_fused(c.entry, c, x, inp, c.imgs, lst)
    assert torch.equal(bits(again.rows), bits(got.rows))


# ------------------------------------------------------------------------------------------------------------ gnx_conv_stem
def check_stem(c, kind):
    r, ref = R.stem_inputs(c, kind), R.stem_reference(c, kind)
    d = r.x.shape[0]
    m = torch.arange(c.imgs) % d
    ho, wo = R.conv_out(c.H, c.KH, c.stride, c.pad), R.conv_out(c.W, c.KW, c.stride, c.pad)
    M, col0 = c.imgs * ho * wo, min(2, c.ldc - c.O)
    x, w = r.x.to(DEV)[m.to(DEV)].contiguous(), r.w.to(DEV)
    out = Buf(M * c.ldc)
    assert run('conv_stem', c._asdict(), dict(x=L.ptr(x), w=L.ptr(w), out=out.ptr + 4 * col0)) == R.form_of(c)
    assert out.frames_unchanged() and torch.equal(w.cpu(), r.w)
    mat = out.win.cpu().view(M, c.ldc)
    assert bool(torch.isnan(mat[:, :col0]).all()) and bool(torch.isnan(mat[:, col0 + c.O:]).all()), 'a write past column O'
    rows = mat[:, col0:col0 + c.O]
    want = ref.val.view(d, ho * wo, c.O)[m].reshape(M, c.O)
    if kind == 'int':
        assert torch.equal(rows.double(), want), 'kind 1: not the bits of the float64 reference'
    else:
        tol = ref.tol.view(d, ho * wo, c.O)[m].reshape(M, c.O)
        assert R.detectable(tol)
        assert not R.flagged(rows, want, tol), float(((rows.double() - want).abs() / tol).max())


@pytest.mark.parametrize('c', STEMS, ids=R.ids)
def test_conv_stem_against_float64(c):
    assert R.form_of(c) in ('stem.generic', 'stem.patch7', 'stem.patch3')
    check_stem(c, 'int')
    check_stem(c, 'mag')


# ------------------------------------------------------------------------------------------------------------ max pool
def check_pool(c, kind):
    r, ref = R.pool_inputs(c, kind), R.pool_reference(c, kind)
    d = r.x.shape[0]
    m = (torch.arange(c.imgs) % d).to(DEV)
    ho, wo = R.pooled(c.Hi), R.pooled(c.Wi)
    M, C = c.imgs * ho * wo, c.C
    rows_in = R.to_ld(R.as_rows(r.x), c.ldi, 0).view(d, c.Hi * c.Wi * c.ldi).to(DEV)
    xin = Buf(c.imgs * c.Hi * c.Wi * c.ldi, off=int(c.off == 'in'), data=rows_in[m])
    scale = Buf(C, off=int(c.off == 'scale'), data=r.scale.to(DEV))
    shift = Buf(C, off=int(c.off == 'shift'), data=r.shift.to(DEV))
    out = Buf(M * c.ldo, off=int(c.off == 'out'))
    amax = Buf(M * C, torch.uint8, off=int(c.off == 'amax')) if c.argmax else None
    P = {'in': xin.ptr, 'out': out.ptr, 'scale': scale.ptr, 'shift': shift.ptr, 'amax': None if amax is None else amax.ptr}
    assert run('maxpool_argmax' if c.argmax else 'maxpool', c._asdict(), P) == R.form_of(c)
    assert out.frames_unchanged() and xin.untouched() and scale.untouched() and shift.untouched()
    mat = out.win.view(M, c.ldo)
    assert bool(torch.isnan(mat[:, C:]).all()), 'a write past column C'
    rows = mat[:, :C]
    want = ref.val.to(DEV)[m].reshape(M, C)
    if kind == 'int':
        assert torch.equal(rows.double(), want), 'kind 1: not the bits of the float64 reference'
    else:
        tol = ref.tol.to(DEV)[m].reshape(M, C)
        assert R.detectable(tol) and not R.flagged(rows, want, tol)
    if amax is not None:
        assert amax.frames_unchanged()
        cmp = None if kind == 'int' else ref.comparable.to(DEV)[m].reshape(M, C)
        assert not R.idx_flagged(amax.win.view(M, C), ref.idx.to(DEV)[m].reshape(M, C), cmp)
    return rows


@pytest.mark.parametrize('c', POOLS, ids=R.ids)
def test_bnrelu_maxpool_against_float64(c):
    assert R.form_of(c) == 'maxpool.%s.%s' % ('scalar' if (c.off or c.C % 4 or c.ldi % 4 or c.ldo % 4) else 'vec4',
                                               'argmax' if c.argmax else 'plain')
    check_pool(c, 'int')
    rows = check_pool(c, 'mag')
    if c.argmax and c.off != 'amax':                       # the _argmax form's values: the plain form's bits
        assert torch.equal(bits(check_pool(c._replace(argmax=0), 'mag')), bits(rows))


# ------------------------------------------------------------------------------------------------------------ average pool
def check_avg(c, kind):
    r, ref = R.avg_inputs(c, kind), R.avg_reference(c, kind)
    rows_in, C = c.imgs * c.S2, c.C
    total = rows_in + c.extra
    if c.entry == 'h16_cb':
        xin = Buf((C // 32) * total * 32, torch.float16, data=R.to_cb(r.x.half(), total).to(DEV))
    elif c.entry == 'h16':
        xin = Buf(rows_in * c.ldi, torch.float16, data=R.to_ld(r.x.half(), c.ldi, 0).to(DEV))
    else:
        xin = Buf(rows_in * c.ldi, data=R.to_ld(r.x, c.ldi, 0).to(DEV))
    orows = c.imgs + (c.extra if c.entry == 'idx' else 0)
    out = Buf(orows * c.ldo)
    scale, shift = r.scale.to(DEV), r.shift.to(DEV)
    lst = R.avg_dst(c) if c.entry == 'idx' else None
    idx = torch.tensor(lst, dtype=torch.int32, device=DEV) if lst else None
    a = dict(c._asdict(), dst_rows=orows, rows_total=total)
    P = {'in': xin.ptr, 'out': out.ptr, 'scale': L.ptr(scale), 'shift': L.ptr(shift), 'idx': None if idx is None else idx.data_ptr()}
    assert run('avgpool.' + c.entry, a, P) == R.form_of(c)
    assert out.frames_unchanged() and xin.untouched()
    mat = out.win.cpu().view(orows, c.ldo)
    assert bool(torch.isnan(mat[:, C:]).all()), 'a write past column C'
    want, tol = ref.val, ref.tol
    if lst is not None:
        want, tol = R.scatter(ref.val, lst, orows), R.scatter(ref.tol, lst, orows, fill=0.0)
    hole = torch.isnan(want)
    assert torch.equal(torch.isnan(mat[:, :C]), hole), 'a row that dst_idx skips was written, or a row it names was not'
    rows, want = mat[:, :C][~hole], want[~hole]
    if kind == 'int':
        assert torch.equal(rows, want.float()), 'kind 1: not the float64 reference rounded to fp32'
    else:
        assert R.detectable(tol) and not R.flagged(rows, want, tol[~hole])


@pytest.mark.parametrize('c', AVGS, ids=R.ids)
def test_bnrelu_avgpool_against_float64(c):
    assert R.form_of(c) == 'avgpool.' + c.entry
    check_avg(c, 'int')
    check_avg(c, 'mag')


# ------------------------------------------------------------------------------------------------------------ uint8 converter
def check_u8(c):
    g = torch.Generator().manual_seed(c.imgs + 10 * c.C + 100 * c.H)
    x8 = torch.randint(0, 256, (c.imgs, c.C, c.H, c.W), generator=g).to(torch.uint8)
    x8.view(-1)[:min(256, x8.numel())] = torch.arange(min(256, x8.numel())).to(torch.uint8)
    xd, norm = x8.to(DEV), R.norm_vector().to(DEV) if c.norm else None
    out = Buf(x8.numel())
    assert run('u8_to_f32', c._asdict(), dict(x=xd.data_ptr(), out=out.ptr, norm=None if norm is None else L.ptr(norm))) == R.form_of(c)
    assert out.frames_unchanged() and torch.equal(xd.cpu(), x8)
    assert torch.equal(bits(out.win.cpu().view(x8.shape)), bits(R.to_tensor(x8, c.norm))), 'not the bits of torch\'s ToTensor / Normalize'


@pytest.mark.parametrize('c', U8S, ids=R.ids)
def test_u8_to_f32_is_torch_bit_for_bit(c):
    assert R.form_of(c) == 'u8_to_f32'
    check_u8(c)


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('e', list(R.REFUSALS), ids=str)
def test_refusals_leave_the_output_alone(e):
    """Each UNSUPPORTED / BAD_ARG condition of the launcher broken alone, and imgs == 0: the code, nothing written; then the
    accepted base call, which does write (and is checked like any case)."""
    base = R.REFUSAL_BASE[e]
    entry, a = R.call_of(base)
    h16 = e in R.IS_H16
    room = {k: torch.zeros(1 << 17, device=DEV) for k in ('x', 'w', 'in', 'scale', 'shift', 'norm', 'idx')}   # zeros: index 0, too
    out, amax = Buf(1 << 16, torch.float16 if h16 else torch.float32), Buf(1 << 16, torch.uint8)
    start = dict({k: v.data_ptr() for k, v in room.items()}, out=out.ptr, amax=amax.ptr)
    for over, want in R.REFUSALS[e] + [({'imgs': 0}, R.EMPTY)]:
        b = dict(a, **over)
        assert R.form_of_call(entry, b) == want
        P = {k: (None if b.get(k) is None else start[k] + b[k]) for k in start}
        assert asked(entry, b, P) == want
        code = L.query(NAME[entry], *cargs(entry, b, P))
        torch.cuda.synchronize()
        assert code == CODE[want], (over, want, code)
        assert out.untouched() and amax.untouched(), over
    if isinstance(base, R.Fused):
        check_fused(base, 'int')
    elif isinstance(base, R.Stem):
        check_stem(base, 'int')
    elif isinstance(base, R.Pool):
        check_pool(base, 'int')
    elif isinstance(base, R.Avg):
        check_avg(base, 'int')
    else:
        check_u8(base)
