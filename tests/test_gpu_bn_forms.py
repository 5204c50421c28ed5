"""Every kernel form of csrc/bn.hip at its boundaries, through the C ABI, against the float64 reference tests/bn_ref.py.

One call of gnx_bn_train_stats* / gnx_bn_relu_bwd* lands in one of nine kernels depending on M, C, the leading dimensions, the
pointers' alignment, `relu` and `training` ("BatchNorm forms"); bn_ref.GRID holds the smallest shapes at which each
form and each edge between two of them exists; bn_ref.form / bwd_form restate the dispatch, and each call first compares them with
gnx_bn_train_stats_form / gnx_bn_relu_bwd_form, so that a case which silently lands in another body fails.  Every operand is a window [0:M, off:off+C] of a larger tensor filled with a
sentinel of its own, every per-channel vector has a sentinel tail: after a call everything outside the window must be
bit-identical to the sentinel, and every input bit-unchanged.

Tolerances are per channel (bn_ref's docstring): |err_c| <= K 2^-24 sum_r |t_rc| for a reduced quantity, the propagated bound +
8 * 2^-24 * (magnitude sum of the last multiply-add chain) for an element-wise one.  Each case also asserts detectability:
the smallest single-row term of each reduction is at least four tolerances, so that a dropped, doubled or mis-masked row fails.

K.  A plain fp32 torch evaluation of the same formulas on the device (`.float()` tensors, `.sum(0)`) was measured against the
float64 reference over every shape of this file (K_SHAPES), training and running statistics, relu 0 / 1;
the figure is max_c |err_c| / (2^-24 sum_r |t_rc|), largest per reduced quantity (and where):
    column sum of x (the mean, gnx_colsum)    5.918   (4992 x 1040;  4.19 at 2049 x 1040, 3.15 at 2049 x 1024, 2.68 at 8193 x 67)
    centred second moment                     4.907   (4992 x 1040;  4.52 at 2049 x 1040, 4.47 at 49 x 68)
    sum dz (dbeta)                            1.320
    sum dz xhat (dgamma)                      2.954   (48 x 68)
K = max(8, 4 x 5.9181) = 23.67 (bn_ref.K).  The kernels' own error had no part in it.  The measurement stays runnable as
test_plain_fp32_torch_stays_within_the_ratio_K_was_set_from, which prints the figures of every shape.  With K = 23.67
detectability asks min / mean of a reduction's terms >= 0.74 at M = 131 329: bn_ref.recipe narrows its spreads above 32 768
rows (its docstring), which test_bn_ref_host.py checks on the CPU.
"""
import ctypes
import functools

import pytest
import torch

import bn_ref as R
from gridnext_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
K = R.K


# ----------------------------------------------------------------------------------------------------------- operands
class Emb:
    """A window [0:M, off:off+C] of an [M + 3][ld] tensor that starts `shift` floats into its storage, everything else sentinel."""

    def __init__(self, val, M, C, ld, off, sentinel, shift=0):
        self.M, self.C, self.ld, self.off, self.shift = M, C, ld, off, shift
        self.flat = torch.full(((M + 3) * ld + 8,), float(sentinel), device=DEV)
        self.win = self._window(self.flat)
        if val is not None:
            self.win.copy_(val.to(DEV))
        self.before = self.flat.clone()
        self.ptr = self.flat.data_ptr() + 4 * (shift + off)

    def _window(self, flat):
        return flat[self.shift:self.shift + (self.M + 3) * self.ld].view(self.M + 3, self.ld)[:self.M, self.off:self.off + self.C]

    def get(self):
        return self.win.cpu()

    def unchanged(self):
        return torch.equal(self.flat, self.before)

    def outside_unchanged(self):
        a, b = self.flat.clone(), self.before.clone()
        self._window(a).zero_()
        self._window(b).zero_()
        return torch.equal(a, b)


class Vec:
    """A per-channel vector of C entries with a sentinel tail of 8; val None: an output, sentinel throughout."""

    def __init__(self, val, C, sentinel, dtype=torch.float32):
        self.C = C
        self.buf = torch.full((C + 8,), sentinel, device=DEV, dtype=dtype)
        if val is not None:
            self.buf[:C] = val.to(DEV)
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr()

    def get(self):
        return self.buf[:self.C].cpu()

    def unchanged(self):
        return torch.equal(self.buf, self.before)

    def tail_unchanged(self):
        return torch.equal(self.buf[self.C:], self.before[self.C:])


def P(o):
    return None if o is None else o.ptr


def workspace(M, C):
    return torch.empty(L.query('gnx_bn_workspace', M, C), device=DEV)


def sync_words(C):
    n = L.query('gnx_bn_sync_words', C)
    w = torch.zeros(n + 8, dtype=torch.int32, device=DEV)
    w[n:] = 0x5A5A5A5A
    return w, n


def sync_left_zero(w, n):
    return int(w[:n].abs().sum().item()) == 0 and bool((w[n:] == 0x5A5A5A5A).all())


def check(what, got, ref, tol):
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.numel() == 0:
        return
    err = (got - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    miss = ~(err <= tol)                                       # a NaN or an infinity in `got` is a miss, not a pass
    if miss.any():
        ratio = torch.where(miss, torch.nan_to_num(err / tol, nan=R.INF), torch.zeros_like(err))
        worst = ratio.max().item()
        i = int(ratio.argmax())
        idx = divmod(i, err.shape[-1]) if err.dim() == 2 else (i,)
        raise AssertionError("%s: |err| %.4e = %.3g x tolerance %.4e at %s (got %.9g, want %.9g)" % (
            what, err.flatten()[i].item(), worst, tol.flatten()[i].item(), idx, got.flatten()[i].item(), ref.flatten()[i].item()))


def assert_detectable(what, r_min, tol):
    assert R.detectable(r_min, tol), "%s: the smallest single-row term is below 4 tolerances" % what


# ------------------------------------------------------------------------------------------------ 1. forward statistics
@functools.lru_cache(maxsize=4)
def _stats_ref(M, C, momentum, eps, gamma_null=False):
    rec = R.recipe(M, C)
    g, b = (None, None) if gamma_null else (rec.gamma, rec.beta)
    s = R.stats(rec.x, g, b, rec.running_mean, rec.running_var, momentum, eps)
    t = R.stats_tol(s, K)
    assert_detectable('sum', s.sum_min, t.sum)
    assert_detectable('m2', s.m2_min, t.m2)
    return rec, s, t


def al16(ptr):
    return ptr % 16 == 0


def query(name, *args):
    """(code, flag, workgroups) of gnx_bn_train_stats_form / gnx_bn_relu_bwd_form."""
    flag, wgs = ctypes.c_int(-7), ctypes.c_int(-7)
    return L.query(name, *args, ctypes.addressof(flag), ctypes.addressof(wgs)), flag.value, wgs.value


def run_stats(entry, rec, M, C, ld, off, ldy, momentum, eps, relu, gamma_null=False, running_null=False, shift=0, yoff=None,
              want=None):
    """One call of a gnx_bn_train_stats* entry point on embedded operands; the sentinel / unchanged-input checks; the outputs.
    First: gnx_bn_train_stats_form says what bn_ref.form says of these pointers (and `want`, the caller's expectation, if given),
    so that a case cannot silently test another body."""
    x = Emb(rec.x, M, C, ld, off, 1234.5, shift)
    gamma = None if gamma_null else Vec(rec.gamma, C, 11.0)
    beta = None if gamma_null else Vec(rec.beta, C, 12.0)
    rm = None if running_null else Vec(rec.running_mean, C, 13.0)
    rv = None if running_null else Vec(rec.running_var, C, 14.0)
    nbt = None if running_null else Vec(torch.tensor([7], dtype=torch.int64), 1, -99, torch.int64)
    outs = {k: Vec(None, C, s) for k, s in (('scale', 21.0), ('shift', 22.0), ('save_mean', 23.0), ('save_invstd', 24.0))}
    ws = workspace(M, C)
    args = [x.ptr, ld, M, C, P(gamma), P(beta), P(rm), P(rv), P(nbt), momentum, eps, outs['scale'].ptr, outs['shift'].ptr,
            outs['save_mean'].ptr, outs['save_invstd'].ptr]
    y = None
    if 'apply' in entry:
        y = Emb(None, M, C, ldy, off if yoff is None else yoff, 31337.0, shift)
        args += [y.ptr, ldy, relu]
    f = R.form(M, C, ld, al16(x.ptr), None if y is None else ldy, y is None or al16(y.ptr), al16(ws.data_ptr()))
    said = query('gnx_bn_train_stats_form', *args[:15], P(y), ldy if y else 0, relu, ws.data_ptr())
    assert said == (R.CODES[f.body], f.fused, f.workgroups), '%s %d x %d: gnx_bn_train_stats_form says %s, bn_ref.form %s' % (
        entry, M, C, said, f)
    assert want is None or f == want, '%s %d x %d: runs %s, the case expects %s' % (entry, M, C, f, want)
    args.append(ws.data_ptr())
    words = None
    if entry.endswith('_sync'):
        words, n = sync_words(C)
        args.append(words.data_ptr())
    L.call(entry, *args, L.stream())
    torch.cuda.synchronize()
    assert x.unchanged(), entry + ': x was written'
    assert all(v is None or v.unchanged() for v in (gamma, beta)), entry + ': gamma / beta were written'
    for k, v in outs.items():
        assert v.tail_unchanged(), '%s: wrote past the C entries of %s' % (entry, k)
    got = {k: v.get() for k, v in outs.items()}
    if not running_null:
        assert rm.tail_unchanged() and rv.tail_unchanged(), entry + ': wrote past the C entries of the running statistics'
        assert nbt.buf.tolist() == [8] + [-99] * 8, entry + ': num_batches_tracked %s' % nbt.buf.tolist()
        got['running_mean'], got['running_var'] = rm.get(), rv.get()
    if y is not None:
        assert y.outside_unchanged(), entry + ': y written outside its window'
        got['y'] = y.get()
    if words is not None:
        assert sync_left_zero(words, n), entry + ': the sync words were not left zero'
    return got


def check_stats(entry, got, rec, s, t, relu):
    check(entry + ' save_mean', got['save_mean'], s.mean, t.mean)
    check(entry + ' save_invstd', got['save_invstd'], s.invstd, t.invstd)
    check(entry + ' scale', got['scale'], s.scale, t.scale)
    check(entry + ' shift', got['shift'], s.shift, t.shift)
    if 'running_mean' in got:
        check(entry + ' running_mean', got['running_mean'], s.running_mean, t.running_mean)
        check(entry + ' running_var', got['running_var'], s.running_var, t.running_var)
    if 'y' in got:
        a = R.apply(rec.x, s.scale, s.shift, relu)
        check(entry + ' y', got['y'], a.y, R.apply_tol(a, rec.x, t.scale, t.shift))


def scale_shift_relu(xval, M, C, ldx, ldy, off, scale, shift, relu):
    x, y = Emb(xval, M, C, ldx, off, 1234.5), Emb(None, M, C, ldy, off, 31337.0)
    sc, sh = Vec(scale, C, 21.0), Vec(shift, C, 22.0)
    L.call('gnx_scale_shift_relu', x.ptr, ldx, y.ptr, ldy, M, C, sc.ptr, sh.ptr, relu, L.stream())
    torch.cuda.synchronize()
    assert x.unchanged() and sc.unchanged() and sh.unchanged() and y.outside_unchanged()
    return y.get()


STATS_ENTRIES = ('gnx_bn_train_stats', 'gnx_bn_train_stats_sync', 'gnx_bn_train_stats_apply', 'gnx_bn_train_stats_apply_sync')


@pytest.mark.parametrize("lay", R.LAYOUTS)
@pytest.mark.parametrize("M,C", R.GRID)
def test_forward_statistics(M, C, lay):
    i = R.GRID.index((M, C)) + R.LAYOUTS.index(lay)
    momentum, eps = R.mom_eps(i)
    relu = (i // 2) % 2
    rec, s, t = _stats_ref(M, C, momentum, eps)
    ld, off = R.layout(lay, C)
    ldy = ld + 4                                               # ldy != ld, same alignment class
    want = {e: R.form_of(M, C, lay, lay if 'apply' in e else None) for e in STATS_ENTRIES}
    if lay == ('window' if C % 4 == 0 else 'misaligned'):      # the layout the grid's groups are named for
        assert all(f.body == R.GRID_FORM[(M, C)] for f in want.values()), (want, R.GRID_FORM[(M, C)])
    got = {e: run_stats(e, rec, M, C, ld, off, ldy, momentum, eps, relu, want=want[e]) for e in STATS_ENTRIES}
    for e in STATS_ENTRIES:
        check_stats(e, got[e], rec, s, t, relu)
    # the _sync entry points are the plain ones but for where the barrier's counters live: bit for bit
    for plain in ('gnx_bn_train_stats', 'gnx_bn_train_stats_apply'):
        for k, v in got[plain].items():
            assert torch.equal(v, got[plain + '_sync'][k]), '%s_sync differs from %s in %s' % (plain, plain, k)
    # _apply == train_stats followed by gnx_scale_shift_relu.  x and y share an alignment class here, so both routes take the
    # same statistics kernel, and both apply y = fmaf(x, scale, shift) on the scale / shift they return (bn.hip: `apply` in the
    # single-launch forms, scale_shift_relu_kernel): bit for bit
    plain, fused = got['gnx_bn_train_stats'], got['gnx_bn_train_stats_apply']
    y2 = scale_shift_relu(rec.x, M, C, ld, ldy, off, plain['scale'], plain['shift'], relu)
    a = R.apply(rec.x, s.scale, s.shift, relu)
    check('gnx_scale_shift_relu y', y2, a.y, R.apply_tol(a, rec.x, t.scale, t.shift))
    for k in plain:
        assert torch.equal(plain[k], fused[k]), '_apply differs from train_stats in ' + k
    assert torch.equal(fused['y'], y2), '_apply: y is not fmaf(x, scale, shift) of its own scale and shift'
    # a y off 16 B beside a 16-B x: the statistics body x alone gets, then scale_shift_relu_kernel - the same bits again
    if want['gnx_bn_train_stats'].body not in ('slab', 'slab_vec'):
        ldm, offm = R.layout('misaligned', C)
        for e in ('gnx_bn_train_stats_apply', 'gnx_bn_train_stats_apply_sync'):
            mixed = R.form_of(M, C, lay, 'misaligned')
            assert (mixed.body, mixed.fused) == (want[e].body, 0) and want[e].fused == 1
            gm = run_stats(e, rec, M, C, ld, off, ldm + 4, momentum, eps, relu, yoff=offm, want=mixed)
            for k in plain:
                assert torch.equal(plain[k], gm[k]), '%s with a misaligned y differs from train_stats in %s' % (e, k)
            assert torch.equal(gm['y'], y2), e + ' with a misaligned y: y is not that of gnx_scale_shift_relu'


@pytest.mark.parametrize("M,C", [(257, 12), (4993, 12), (8193, 8), (300, 3)])
@pytest.mark.parametrize("which", ['gamma_beta', 'running'])
def test_forward_statistics_null_operands(M, C, which):
    momentum, eps = R.mom_eps(1)
    gamma_null = which == 'gamma_beta'
    rec, s, t = _stats_ref(M, C, momentum, eps, gamma_null)
    ld, off = R.layout('window', C)
    for e in STATS_ENTRIES:
        got = run_stats(e, rec, M, C, ld, off, ld + 4, momentum, eps, 1, gamma_null=gamma_null, running_null=not gamma_null)
        assert ('running_mean' in got) == gamma_null
        check_stats(e + ' NULL ' + which, got, rec, s, t, 1)


# ------------------------------------------------------------------------------------------------------- 2. backward
@functools.lru_cache(maxsize=4)
def _bwd_operands(M, C, relu, training, eps):
    return R.bwd_operands(R.recipe(M, C), relu, training, eps)


COMBOS = R.BWD_COMBOS    # relu training accumulate dx_accumulate dx_null dgamma_null also_sync


def run_bwd(entry, rec, o, M, C, lay, relu, training, accumulate, dx_accumulate, dx_null, dgamma_null, xval=None, shift=0,
            expect_unsupported=False, want=None):
    """One call of gnx_bn_relu_bwd[_sync] on embedded operands; the sentinel / unchanged-input checks; dx, dgamma, dbeta.
    First: gnx_bn_relu_bwd_form says what bn_ref.bwd_form says of these pointers (and `want`, if given)."""
    (ld, off), (lddx, offdx) = lay
    dy = Emb(rec.dy, M, C, ld, off, -777.25, shift)
    x = Emb(o.x if xval is None else xval, M, C, ld, off, 1234.5, shift)
    dx = None if dx_null else Emb(rec.dx_old if (dx_accumulate or expect_unsupported) else None, M, C, lddx, offdx, -4242.5)
    vecs = [Vec(v, C, 20.0 + j) for j, v in enumerate((o.scale, o.shift, o.mean, o.invstd))]
    dg = None if dgamma_null else Vec(rec.dgamma_old if (accumulate or expect_unsupported) else None, C, 31.0)
    db = None if dgamma_null else Vec(rec.dbeta_old if (accumulate or expect_unsupported) else None, C, 32.0)
    ws = workspace(M, C)
    args = [dy.ptr, ld, x.ptr, ld, P(dx), lddx, M, C] + [v.ptr for v in vecs] + [P(dg), P(db), relu, training, accumulate,
                                                                                dx_accumulate, ws.data_ptr()]
    f = R.bwd_form(M, C, ld, al16(dy.ptr), None if dx is None else lddx, dx is None or al16(dx.ptr), relu, training,
                   al16(ws.data_ptr()))
    said = query('gnx_bn_relu_bwd_form', *args)
    code = R.UNSUPPORTED if f.body is None else R.CODES[f.body]
    assert said == (code, f.dx_vec4, f.workgroups), '%s %d x %d: gnx_bn_relu_bwd_form says %s, bn_ref.bwd_form %s' % (entry, M, C, said, f)
    assert (f.body is None) == expect_unsupported and (want is None or f == want), (entry, M, C, f, want)
    words = None
    if entry.endswith('_sync'):
        words, n = sync_words(C)
        args.append(words.data_ptr())
    ran = L.try_call(entry, *args, L.stream())
    torch.cuda.synchronize()
    assert dy.unchanged() and x.unchanged() and all(v.unchanged() for v in vecs), entry + ': an input was written'
    if expect_unsupported:
        assert not ran, entry + ' accepted what its header excludes'
        assert all(v is None or v.unchanged() for v in (dx, dg, db)), entry + ': declined, yet wrote an output'
        return None
    assert ran, entry + ' declined a supported shape'
    assert dx is None or dx.outside_unchanged(), entry + ': dx written outside its window'
    assert all(v is None or v.tail_unchanged() for v in (dg, db)), entry + ': wrote past the C entries of dgamma / dbeta'
    if words is not None:
        assert sync_left_zero(words, n), entry + ': the sync words were not left zero'
    return {'dx': None if dx is None else dx.get(), 'dgamma': None if dg is None else dg.get(),
            'dbeta': None if db is None else db.get()}


def check_bwd(what, got, b, t):
    assert_detectable(what + ' s1', b.s1_min, t.s1)
    assert_detectable(what + ' s2', b.s2_min, t.s2)
    if got['dbeta'] is not None:
        check(what + ' dbeta', got['dbeta'], b.dbeta, t.dbeta)
        check(what + ' dgamma', got['dgamma'], b.dgamma, t.dgamma)
    if got['dx'] is not None:
        check(what + ' dx', got['dx'], b.dx, t.dx)


def bwd_layout(name, C):
    lay, dxlay = R.bwd_layouts(name)
    return R.layout(lay, C), R.layout(dxlay, C)


# (the mixed layout only where there is a 16-B form to mix with: 4 | C)
BWD_CASES = [(M, C, lay) for M, C in R.GRID for lay in R.BWD_LAYOUTS if lay != 'dx_misaligned' or C % 4 == 0]


@pytest.mark.parametrize("M,C,lay", BWD_CASES)
def test_backward(M, C, lay):
    rec = R.recipe(M, C)
    eps = R.mom_eps(R.GRID.index((M, C)))[1]
    failed = []                                                # every combination runs: a failure names all that miss
    for combo in COMBOS:
        relu, training, accumulate, dx_accumulate, dx_null, dgamma_null, also_sync = combo
        o = _bwd_operands(M, C, relu, training, eps)
        b = R.bwd(rec.dy, o.x, o.scale, o.shift, o.mean, o.invstd, relu, training, rec.dx_old if dx_accumulate else None,
                  rec.dgamma_old if accumulate else None, rec.dbeta_old if accumulate else None)
        t = R.bwd_tol(b, K)
        xlay, dxlay = R.bwd_layouts(lay)
        want = R.bwd_form_of(M, C, xlay, None if dx_null else dxlay, relu, training)
        try:
            got = run_bwd('gnx_bn_relu_bwd', rec, o, M, C, bwd_layout(lay, C), *combo[:6], want=want)
            check_bwd('bwd relu %d training %d' % (relu, training), got, b, t)
            if also_sync:
                got2 = run_bwd('gnx_bn_relu_bwd_sync', rec, o, M, C, bwd_layout(lay, C), *combo[:6], want=want)
                for k, v in got.items():
                    assert (v is None and got2[k] is None) or torch.equal(v, got2[k]), 'gnx_bn_relu_bwd_sync differs in ' + k
        except AssertionError as e:
            failed.append('relu %d training %d accumulate %d dx_accumulate %d dx NULL %d dgamma NULL %d: %s' % (combo[:6] + (e,)))
    assert not failed, '\n'.join(failed)


def test_backward_16B_dx_pass_beyond_4096_workgroups():
    """bn_bwd_dx_vec4_kernel covers 4 channels per thread, so the grid's shape at 131 329 rows (C = 12) stays under the
    4096-workgroup cap of elementwise_grid; C = 36 takes its grid-stride loop into a second round."""
    M, C = R.DX_VEC4_LOOP
    assert M * (C // 4) > 4096 * 256
    rec = R.recipe(M, C)
    eps = R.mom_eps(0)[1]
    for relu, dx_accumulate in ((0, 0), (1, 1)):
        o = _bwd_operands(M, C, relu, 1, eps)
        b = R.bwd(rec.dy, o.x, o.scale, o.shift, o.mean, o.invstd, relu, 1, rec.dx_old if dx_accumulate else None)
        want = R.bwd_form_of(M, C, 'window', 'window', relu, 1)
        assert (want.body, want.dx_vec4) == ('slab_vec', 1)
        got = run_bwd('gnx_bn_relu_bwd', rec, o, M, C, bwd_layout('window', C), relu, 1, 0, dx_accumulate, False, False, want=want)
        check_bwd('bwd 16-B dx loop relu %d' % relu, got, b, R.bwd_tol(b, K))


# --------------------------------------------------------------------------------------------- 3. activated-input form
@pytest.mark.parametrize("M,C", R.ACT_GRID)
def test_activated_input_form(M, C):
    rec = R.recipe(M, C)
    eps = R.mom_eps(0)[1]
    o = _bwd_operands(M, C, 2, 0, eps)
    assert (o.scale < 0).any() and (o.scale > 0).any()         # the form divides by scale: both signs
    win = bwd_layout('window', C)
    for accumulate, dx_accumulate, dx_null in ((0, 0, False), (1, 1, False), (1, 0, True), (0, 0, True)):
        b = R.bwd(rec.dy, o.a, o.scale, o.shift, o.mean, o.invstd, 2, 0, rec.dx_old if dx_accumulate else None,
                  rec.dgamma_old if accumulate else None, rec.dbeta_old if accumulate else None)
        want = R.bwd_form_of(M, C, 'window', None if dx_null else 'window', 2, 0)
        assert want.body == R.ACT_FORM
        got = run_bwd('gnx_bn_relu_bwd', rec, o, M, C, win, 2, 0, accumulate, dx_accumulate, dx_null, False, xval=o.a, want=want)
        check_bwd('bwd relu 2', got, b, R.bwd_tol(b, K))
    # batch statistics, or an operand that the 16-B form cannot read: declined, nothing written
    run_bwd('gnx_bn_relu_bwd', rec, o, M, C, win, 2, 1, 0, 0, False, False, xval=o.a, expect_unsupported=True)
    for lay in ('misaligned', 'dx_misaligned'):
        run_bwd('gnx_bn_relu_bwd', rec, o, M, C, bwd_layout(lay, C), 2, 0, 0, 0, False, False, xval=o.a, expect_unsupported=True)
    run_bwd('gnx_bn_relu_bwd_sync', rec, o, M, C, win, 2, 1, 0, 0, True, False, xval=o.a, expect_unsupported=True)


# --------------------------------------------------------------------------------- 4. the bit-identity the source claims
def colsum(xval, M, C, ld, off, accumulate, old, shift=0):
    x = Emb(xval, M, C, ld, off, 1234.5, shift)
    out = Vec(old if accumulate else None, C, 41.0)
    ws = workspace(M, C)
    L.call('gnx_colsum', x.ptr, ld, M, C, out.ptr, accumulate, ws.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert x.unchanged() and out.tail_unchanged()
    return out.get()


@pytest.mark.parametrize("M,C", [(8193, 8), (131329, 12)])
def test_16B_slabs_are_bit_identical_to_scalar_slabs(M, C):
    """bn.hip says of colsum_v4_kernel and bn_bwd_partial_v4_kernel that they add in the scalar kernels' order, "so the slabs are
    bit-identical": the same values once 16-B aligned and once one float further into the same kind of storage (4 | ld, so only
    the pointer decides) must give the same bits in everything that is a sum of slabs."""
    rec = R.recipe(M, C)
    momentum, eps = R.mom_eps(0)
    ld = C + 4
    stats = [run_stats('gnx_bn_train_stats', rec, M, C, ld, 0, ld, momentum, eps, 0, shift=s) for s in (0, 1)]
    for k in ('save_mean', 'save_invstd', 'scale', 'shift', 'running_mean', 'running_var'):
        assert torch.equal(stats[0][k], stats[1][k]), 'statistics from 16-B slabs differ from scalar slabs in ' + k
    sums = [colsum(rec.x, M, C, ld, 0, 1, rec.dbeta_old, shift=s) for s in (0, 1)]
    assert torch.equal(sums[0], sums[1]), 'gnx_colsum from 16-B loads differs from the scalar kernel'
    lay = ((ld, 0), (ld, 0))
    for relu in (0, 1):
        o = _bwd_operands(M, C, relu, 1, eps)
        b = R.bwd(rec.dy, o.x, o.scale, o.shift, o.mean, o.invstd, relu, 1)
        got = [run_bwd('gnx_bn_relu_bwd', rec, o, M, C, lay, relu, 1, 0, 0, False, False, shift=s) for s in (0, 1)]
        for g in got:
            check_bwd('bwd slabs relu %d' % relu, g, b, R.bwd_tol(b, K))
        for k in ('dgamma', 'dbeta'):
            assert torch.equal(got[0][k], got[1][k]), '%s from 16-B slabs differs from scalar slabs (relu %d)' % (k, relu)


# ------------------------------------------------------------------------------------------------ 5. small entry points
@pytest.mark.parametrize("M,C,lay", R.COLSUM_CASES)
def test_colsum(M, C, lay):
    rec = R.recipe(M, C)
    ld, off = R.layout(lay, C)
    for accumulate in (0, 1):
        r = R.colsum(rec.x, rec.dbeta_old if accumulate else None)
        tol = R.colsum_tol(r, K)
        assert_detectable('colsum', r.sum_min, K * R.U * r.sum_abs)
        check('gnx_colsum', colsum(rec.x, M, C, ld, off, accumulate, rec.dbeta_old), r.out, tol)


@pytest.mark.parametrize("M,C", [(300, 50), (257, 12), (131329, 12)])        # the last: more than 4096 workgroups' worth
@pytest.mark.parametrize("relu", [0, 1])
def test_scale_shift_relu(M, C, relu):
    rec = R.recipe(M, C)
    f = R.fold_eval(rec.gamma, rec.beta, rec.running_mean, rec.running_var, 1e-5)
    sc, sh = f.scale.float(), f.shift.float()
    a = R.apply(rec.x, sc, sh, relu)
    ld, off = R.layout('misaligned' if C % 4 else 'window', C)
    check('gnx_scale_shift_relu', scale_shift_relu(rec.x, M, C, ld, ld + 5, off, sc, sh, relu), a.y, R.apply_tol(a, rec.x))
    # M = 0: fine, and nothing happens
    x, y, vs, vh = Emb(rec.x[:4], 4, C, ld, off, 1234.5), Emb(None, 4, C, ld, off, 31337.0), Vec(sc, C, 21.0), Vec(sh, C, 22.0)
    L.call('gnx_scale_shift_relu', x.ptr, ld, y.ptr, ld, 0, C, vs.ptr, vh.ptr, relu, L.stream())
    torch.cuda.synchronize()
    assert y.unchanged() and x.unchanged()


@pytest.mark.parametrize("C", [3, 256, 257, 1040])
@pytest.mark.parametrize("nulls", ['none', 'save', 'gamma_beta'])
def test_fold_eval(C, nulls):
    rec = R.recipe(4, C)
    eps = R.f32(1e-3) if C % 2 else R.f32(1e-5)
    g, b = (None, None) if nulls == 'gamma_beta' else (rec.gamma, rec.beta)
    f = R.fold_eval(g, b, rec.running_mean, rec.running_var, eps)
    ins = [None if v is None else Vec(v, C, 10.0 + j) for j, v in enumerate((g, b, rec.running_mean, rec.running_var))]
    outs = [Vec(None, C, 20.0 + j) for j in range(4)]
    if nulls == 'save':
        outs[2] = outs[3] = None
    L.call('gnx_bn_fold_eval', C, *[P(v) for v in ins], eps, *[P(v) for v in outs], L.stream())
    torch.cuda.synchronize()
    assert all(v is None or v.unchanged() for v in ins) and all(v is None or v.tail_unchanged() for v in outs)
    t = R.fold_tol(f)
    check('fold scale', outs[0].get(), f.scale, t.scale)
    check('fold shift', outs[1].get(), f.shift, t.shift)
    if outs[2] is not None:
        assert torch.equal(outs[2].get(), rec.running_mean)
        check('fold invstd', outs[3].get(), f.invstd, t.invstd)


# --------------------------------------------------------------------------------------------------- 6. pooled forms
@pytest.mark.parametrize("S,imgs,C", R.POOL_GRID)
def test_pooled_forms(S, imgs, C):
    M, So = imgs * S * S, S // 2
    Mo = imgs * So * So
    rec = R.recipe(M, C)
    o = _bwd_operands(M, C, 1, 0, R.f32(1e-5))
    dYp = R.recipe(Mo, C, seed=1).dy
    ld, off = R.layout('window', C)
    ldp = C + 4                                                # the pooled map has a leading dimension of its own
    vecs = [Vec(v, C, 20.0 + j) for j, v in enumerate((o.scale, o.shift, o.mean, o.invstd))]
    # the adjoint: any S >= 2 (the last row and column of an odd map are not pooled and get dx = 0)
    for accumulate in (0, 1):
        b = R.pooled_bwd(dYp, o.x, o.scale, o.shift, o.mean, o.invstd, S, rec.dgamma_old if accumulate else None,
                         rec.dbeta_old if accumulate else None)
        x, dyp, dx = Emb(o.x, M, C, ld, off, 1234.5), Emb(dYp, Mo, C, ldp, 0, -777.25), Emb(None, M, C, ld, off, -4242.5)
        dg, db = Vec(rec.dgamma_old if accumulate else None, C, 31.0), Vec(rec.dbeta_old if accumulate else None, C, 32.0)
        ws = workspace(M, C)
        L.call('gnx_bn_relu_bwd_pooled', dyp.ptr, ldp, x.ptr, ld, dx.ptr, ld, imgs, S, C, *[v.ptr for v in vecs], dg.ptr, db.ptr,
               accumulate, ws.data_ptr(), L.stream())
        torch.cuda.synchronize()
        assert x.unchanged() and dyp.unchanged() and all(v.unchanged() for v in vecs)
        assert dx.outside_unchanged() and dg.tail_unchanged() and db.tail_unchanged()
        check_bwd('pooled bwd S %d' % S, {'dx': dx.get(), 'dgamma': dg.get(), 'dbeta': db.get()}, b, R.bwd_tol(b, K))
    # the pooled, activated input: even S only (include/gridnext_hip.h); an odd map is declined and nothing is written
    x, out = Emb(o.x, M, C, ld, off, 1234.5), Emb(None, Mo, C, ldp, 0, 31337.0)
    ran = L.try_call('gnx_bnrelu_avgpool2', x.ptr, ld, out.ptr, ldp, imgs, C, S, vecs[0].ptr, vecs[1].ptr, L.stream())
    torch.cuda.synchronize()
    assert x.unchanged() and vecs[0].unchanged() and vecs[1].unchanged()
    if S % 2:
        assert not ran and out.unchanged()
    else:
        assert ran and out.outside_unchanged()
        p = R.bnrelu_avgpool2(o.x, o.scale, o.shift, S)
        check('gnx_bnrelu_avgpool2', out.get(), p.out, R.EW * R.U * p.out_mag)


def test_pooled_forms_decline_a_channel_count_off_four():
    S, imgs, C = 4, 1, 6
    rec = R.recipe(imgs * S * S, C)
    o = _bwd_operands(imgs * S * S, C, 1, 0, R.f32(1e-5))
    vecs = [Vec(v, C, 20.0 + j) for j, v in enumerate((o.scale, o.shift, o.mean, o.invstd))]
    x, dyp = Emb(o.x, 16, C, 8, 0, 1234.5), Emb(rec.dy[:4], 4, C, 8, 0, -777.25)
    dx, out, dg, db = Emb(None, 16, C, 8, 0, -4242.5), Emb(None, 4, C, 8, 0, 31337.0), Vec(None, C, 31.0), Vec(None, C, 32.0)
    ws = workspace(16, C)
    assert not L.try_call('gnx_bn_relu_bwd_pooled', dyp.ptr, 8, x.ptr, 8, dx.ptr, 8, imgs, S, C, *[v.ptr for v in vecs], dg.ptr,
                          db.ptr, 0, ws.data_ptr(), L.stream())
    assert not L.try_call('gnx_bnrelu_avgpool2', x.ptr, 8, out.ptr, 8, imgs, C, S, vecs[0].ptr, vecs[1].ptr, L.stream())
    torch.cuda.synchronize()
    assert dx.unchanged() and out.unchanged() and dg.unchanged() and db.unchanged()


# ------------------------------------------------------------------------------------------------- where K comes from
K_SHAPES = sorted(set(R.GRID) | set(R.ACT_GRID) | {(M, C) for M, C, _ in R.COLSUM_CASES} | {R.DX_VEC4_LOOP} |
                  {(imgs * S * S, C) for S, imgs, C in R.POOL_GRID})


@pytest.mark.parametrize("M,C", K_SHAPES)
def test_plain_fp32_torch_stays_within_the_ratio_K_was_set_from(M, C, capsys):
    """The measurement behind bn_ref.TORCH_FP32_RATIO, kept runnable: the same reductions as plain fp32 torch on the device
    (`.sum(0)`) against the float64 reference, max_c |err_c| / (2^-24 sum_r |t_rc|), over every shape of this file.  A torch whose
    sums round differently fails here with the figure to set TORCH_FP32_RATIO (and with it K = max(8, 4 x ratio)) from."""
    rec = R.recipe(M, C)
    x, dy = rec.x.to(DEV), rec.dy.to(DEV)
    s = R.stats(rec.x, rec.gamma, rec.beta, None, None, 0.1, 1e-5)
    ratios = {}

    def note(what, got, ref, t_abs):
        keep = t_abs > 0
        if keep.any():
            r = ((got.double().cpu() - ref).abs()[keep] / (R.U * t_abs[keep])).max().item()
            ratios[what] = max(ratios.get(what, 0.0), r)
    sm = x.sum(0)
    note('sum', sm, s.sum, s.sum_abs)
    note('m2', ((x - sm / M) ** 2).sum(0), s.m2, s.m2_abs)
    for relu in (0, 1):
        for training in (0, 1):
            o = _bwd_operands(M, C, relu, training, R.f32(1e-5))
            b = R.bwd(rec.dy, o.x, o.scale, o.shift, o.mean, o.invstd, relu, training)
            xd, sc, sh, mu, iv = [t.to(DEV) for t in (o.x, o.scale, o.shift, o.mean, o.invstd)]
            dz = torch.where(xd * sc + sh > 0, dy, torch.zeros_like(dy)) if relu else dy
            note('s1', dz.sum(0), b.s1, b.s1_abs)
            note('s2', (dz * ((xd - mu) * iv)).sum(0), b.s2, b.s2_abs)
    with capsys.disabled():
        print(' torch fp32 ratios at %d x %d: %s' % (M, C, ' '.join('%s %.3f' % kv for kv in sorted(ratios.items()))))
    assert max(ratios.values()) <= R.TORCH_FP32_RATIO, ratios


# --------------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors_launch_nothing():
    M, C, ld = 64, 8, 12
    rec = R.recipe(M, C)
    o = _bwd_operands(M, C, 1, 1, R.f32(1e-5))
    x, dy = Emb(rec.x, M, C, ld, 0, 1234.5), Emb(rec.dy, M, C, ld, 0, -777.25)
    y, dx = Emb(None, M, C, ld, 0, 31337.0), Emb(None, M, C, ld, 0, -4242.5)
    vin = [Vec(v, C, 10.0 + j) for j, v in enumerate((rec.gamma, rec.beta, rec.running_mean, rec.running_var))]
    nbt = Vec(torch.tensor([7], dtype=torch.int64), 1, -99, torch.int64)
    vout = [Vec(None, C, 20.0 + j) for j in range(4)]                          # scale, shift, save_mean, save_invstd
    vst = [Vec(v, C, 20.0 + j) for j, v in enumerate((o.scale, o.shift, o.mean, o.invstd))]
    dg, db, out = Vec(None, C, 31.0), Vec(None, C, 32.0), Vec(None, C, 41.0)
    ws = workspace(M, C).data_ptr()
    st = L.stream()

    def stats_args(x_=x.ptr, ld_=ld, M_=M, C_=C, scale_=vout[0].ptr, ws_=ws):
        return [x_, ld_, M_, C_] + [v.ptr for v in vin] + [nbt.ptr, 0.1, 1e-5, scale_] + [v.ptr for v in vout[1:]], ws_

    def bwd_args(dy_=dy.ptr, lddy_=ld, x_=x.ptr, ldx_=ld, lddx_=ld, M_=M, C_=C, scale_=vst[0].ptr, ws_=ws):
        return [dy_, lddy_, x_, ldx_, dx.ptr, lddx_, M_, C_, scale_] + [v.ptr for v in vst[1:]] + [dg.ptr, db.ptr, 1, 1, 0, 0, ws_]

    bad = [dict(M_=0), dict(M_=-1), dict(C_=0), dict(ld_=C - 1), dict(x_=None), dict(scale_=None), dict(ws_=None)]
    calls = []
    for kw in bad:
        a, w = stats_args(**kw)
        calls.append(('gnx_bn_train_stats', a + [w, st]))
        calls.append(('gnx_bn_train_stats_sync', a + [w, None, st]))
        calls.append(('gnx_bn_train_stats_apply', a + [y.ptr, ld, 1, w, st]))
        calls.append(('gnx_bn_train_stats_apply_sync', a + [y.ptr, ld, 1, w, None, st]))
    a, w = stats_args()
    calls.append(('gnx_bn_train_stats_apply', a + [None, ld, 1, w, st]))
    calls.append(('gnx_bn_train_stats_apply', a + [y.ptr, C - 1, 1, w, st]))
    for kw in (dict(M_=0), dict(C_=0), dict(lddy_=C - 1), dict(ldx_=C - 1), dict(lddx_=C - 1), dict(dy_=None), dict(x_=None),
               dict(scale_=None), dict(ws_=None)):
        calls.append(('gnx_bn_relu_bwd', bwd_args(**kw) + [st]))
        calls.append(('gnx_bn_relu_bwd_sync', bwd_args(**kw) + [None, st]))
    for kw in (dict(M_=0), dict(C_=0), dict(ld_=C - 1), dict(x_=None), dict(o_=None), dict(ws_=None)):
        p = dict(x_=x.ptr, ld_=ld, M_=M, C_=C, o_=out.ptr, ws_=ws)
        p.update(kw)
        calls.append(('gnx_colsum', [p['x_'], p['ld_'], p['M_'], p['C_'], p['o_'], 0, p['ws_'], st]))
    for kw in (dict(M_=-1), dict(C_=0), dict(ldx_=C - 1), dict(ldy_=C - 1), dict(x_=None), dict(y_=None), dict(s_=None)):
        p = dict(x_=x.ptr, ldx_=ld, y_=y.ptr, ldy_=ld, M_=M, C_=C, s_=vst[0].ptr)
        p.update(kw)
        calls.append(('gnx_scale_shift_relu', [p['x_'], p['ldx_'], p['y_'], p['ldy_'], p['M_'], p['C_'], p['s_'], vst[1].ptr, 1, st]))
    for kw in (dict(C_=0), dict(rm_=None), dict(rv_=None), dict(scale_=None), dict(shift_=None)):
        p = dict(C_=C, rm_=vin[2].ptr, rv_=vin[3].ptr, scale_=vout[0].ptr, shift_=vout[1].ptr)
        p.update(kw)
        calls.append(('gnx_bn_fold_eval', [p['C_'], vin[0].ptr, vin[1].ptr, p['rm_'], p['rv_'], 1e-5, p['scale_'], p['shift_'],
                                           vout[2].ptr, vout[3].ptr, st]))
    for kw in (dict(imgs_=0), dict(S_=1), dict(C_=0), dict(lddy_=C - 1), dict(ldx_=C - 1), dict(lddx_=C - 1), dict(dx_=None),
               dict(dy_=None)):
        p = dict(imgs_=4, S_=4, C_=C, lddy_=ld, ldx_=ld, lddx_=ld, dx_=dx.ptr, dy_=dy.ptr)
        p.update(kw)
        calls.append(('gnx_bn_relu_bwd_pooled', [p['dy_'], p['lddy_'], x.ptr, p['ldx_'], p['dx_'], p['lddx_'], p['imgs_'], p['S_'], p['C_']] +
                      [v.ptr for v in vst] + [dg.ptr, db.ptr, 0, ws, st]))
    for kw in (dict(imgs_=-1), dict(S_=1), dict(C_=0), dict(ld_=C - 1), dict(in_=None), dict(out_=None)):
        p = dict(imgs_=4, S_=4, C_=C, ld_=ld, in_=x.ptr, out_=y.ptr)
        p.update(kw)
        calls.append(('gnx_bnrelu_avgpool2', [p['in_'], p['ld_'], p['out_'], p['ld_'], p['imgs_'], p['C_'], p['S_'], vst[0].ptr,
                                              vst[1].ptr, st]))
    for name, args in calls:
        with pytest.raises(RuntimeError, match='bad argument'):
            L.call(name, *args)
    torch.cuda.synchronize()
    for v in [x, dy, y, dx, nbt, dg, db, out] + vin + vout + vst:
        assert v.unchanged()
