"""csrc/sparse_linear.hip through the C ABI against tests/sparse_linear_ref.py: the forward and the weight gradient bit for bit
against the documented order restated in numpy float32 (fmaf emulated exactly: the float64 product is exact, the float64 sum's
rounding error is recovered and ties are resolved by it), per element within the DERIVED bound gamma(n) T of the float64 value,
the bit invariances (second call, position and neighbours of a line, alignment, leading dimensions, permutation of the batch,
accumulation over two arrays), the adjoint identity, buffers pre-filled with NaN, and every refusal.

Bound: n multiply-adds and one addition of the bias, each rounded once to fp32, in any order, lie within gamma T of the exact
value: gamma = (n + 1) u / (1 - (n + 1) u), u = 2^-24, T = |bias| + sum |val w| per element, n the kept entries.  Two arrays
accumulated: one more addition, gamma(n1 + n2 + 1).

Measured on an MI355X (printed by the tests): see the README's sparse-linear section."""
import numpy as np
import pytest
import torch

import sparse_counts_ref as R
import sparse_linear_ref as SL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [0, 1, 63, 64, 65, 257]
FS = [1, 3, 4, 63, 64, 65, 255, 256, 257, 500, 1000]
N_GENES, G = 400, 300
NAN = float('nan')


def _L():
    from gridnext_amd import _lib
    return _lib


def _dev(array, offset=False):
    """The array on the device: at the start of its (256-byte aligned) storage, or one element into it."""
    if array is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(array))
    t = torch.empty(src.numel() + 1, dtype=src.dtype, device=DEV)
    t[int(offset):int(offset) + src.numel()] = src.reshape(-1).to(DEV)
    return t[int(offset):int(offset) + src.numel()]


def _padded(M, ld):
    """(rows, ld) float32 with M in front and NaN in the padding: a kernel that read the padding would show it."""
    out = np.full((M.shape[0], ld), np.nan, dtype=np.float32)
    out[:, :M.shape[1]] = M
    return out


def _guarded(n, offset, fill=None):
    """(store, view of n floats): NaN (or `fill`) all over, a guard element in front (offset) and eight behind."""
    store = torch.full((n + 1 + 8,), NAN, dtype=torch.float32, device=DEV)
    view = store[int(offset):int(offset) + n]
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill)).reshape(-1))
    return store, view


def _check_guards(store, n, offset):
    assert torch.isnan(store[:int(offset)]).all() and torch.isnan(store[int(offset) + n:]).all()


def _fwd(mat, lines, n, chan, W, bias, ldw, ld_out, offset):
    """offset: (the sparse trio and bias, W, out) each at the start of the storage (False) or one element in (True)."""
    lib = _L()
    ptr, idx, val = mat
    F = W.shape[1]
    o_sp, o_w, o_out = offset
    args = (_dev(ptr), _dev(idx, o_sp), _dev(val, o_sp), _dev(lines), _dev(chan), _dev(_padded(W, ldw), o_w), _dev(bias, o_sp))
    store, out = _guarded(n * ld_out, o_out)
    lib.call('gnx_sparse_linear_fwd_f32', lib.ptr(args[0], torch.int64), lib.ptr(args[1], torch.int32), lib.ptr(args[2]),
             lib.ptr(args[3], torch.int32), n, lib.ptr(args[4], torch.int32), lib.ptr(args[5]), ldw, lib.ptr(args[6]),
             out.data_ptr(), ld_out, F, lib.stream())
    torch.cuda.synchronize()
    _check_guards(store, n * ld_out, o_out)
    got = out.cpu().numpy().reshape(n, ld_out)
    assert np.isnan(got[:, F:]).all() and not np.isnan(got[:, :F]).any()                 # padding untouched, body written
    return got[:, :F].copy()


def _wgrad(mat, gene_lines, n, pos, dY, ld_dy, ldw, offset, before=None, accumulate=0):
    lib = _L()
    ptr, idx, val = mat
    F = dY.shape[1]
    o_sp, o_dy, o_dw = offset
    args = (_dev(ptr), _dev(idx, o_sp), _dev(val, o_sp), _dev(gene_lines), _dev(pos), _dev(_padded(dY, ld_dy), o_dy))
    store, dW = _guarded(n * ldw, o_dw, None if before is None else _padded(before, ldw))
    lib.call('gnx_sparse_linear_wgrad_f32', lib.ptr(args[0], torch.int64), lib.ptr(args[1], torch.int32), lib.ptr(args[2]),
             lib.ptr(args[3], torch.int32), n, lib.ptr(args[4], torch.int32), lib.ptr(args[5]), ld_dy, dW.data_ptr(), ldw, F,
             accumulate, lib.stream())
    torch.cuda.synchronize()
    _check_guards(store, n * ldw, o_dw)
    got = dW.cpu().numpy().reshape(n, ldw)
    assert np.isnan(got[:, F:]).all() and not np.isnan(got[:, :F]).any()
    return got[:, :F].copy()


def _same(got, want):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(got)).view(torch.int32),
                       torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))


def _ratio(got, want64, T):
    """Largest |err| / (u T) over the elements with T > 0."""
    err = np.abs(got.astype(np.float64) - want64)
    return float((err[T > 0] / (SL.U * T[T > 0])).max()) if (T > 0).any() else 0.0


def _within(got, want64, T, n, extra=0):
    return bool((np.abs(got.astype(np.float64) - want64) <= SL.gamma(np.asarray(n) + extra)[:, None] * T).all())


def _up4(F):
    return (F + 3) // 4 * 4


# forms: (sparse trio and bias, dense operand, output) one element into the storage or not, and the two leading dimensions
def _forms(F):
    return [((True, True, True), F + 3, F + 3),                    # nothing 16-byte aligned: a thread per feature
            ((False, False, False), _up4(F) + 4, _up4(F) + 4),     # everything aligned: dwordx4 loads and stores
            ((False, False, True), _up4(F), F + 1),                # dwordx4 loads, dword stores
            ((True, True, False), F, F)]                           # dense rows back to back


@pytest.mark.parametrize("F", FS)
def test_forward_is_the_documented_order_and_within_the_bound(F):
    rng = np.random.default_rng(F)
    mat = R.random_lines(rng, LENGTHS + [300, 40], N_GENES, integer=False)
    chan = np.full(N_GENES, -1, dtype=np.int32)
    chan[rng.choice(N_GENES, size=G, replace=False)] = rng.permutation(G)               # 100 genes dropped, the rest permuted
    W = rng.standard_normal((N_GENES, F)).astype(np.float32)
    bias = rng.standard_normal(F).astype(np.float32)
    lines = np.array([7, 6, 5, 4, 3, 2, 1, 0, -1, 5, 5, 2, -1], dtype=np.int32)          # reversed, no line, repeats
    worst = 0.0
    for ls, n, ch, Wm, b in ((lines, len(lines), chan, W[:G], bias), (None, 8, chan, W[:G], None), (lines, len(lines), None, W, bias),
                             (None, 8, None, W, None)):
        want64, T, cnt = SL.fwd64(*mat, ls, n, ch, Wm, b)
        want32 = SL.fwd32(*mat, ls, n, ch, Wm, b)
        for offset, ldw, ld_out in _forms(F):
            got = _fwd(mat, ls, n, ch, Wm, b, ldw, ld_out, offset)
            assert _within(got, want64, T, cnt), (offset, ldw, ld_out)
            assert _same(got, want32), (offset, ldw, ld_out)
            worst = max(worst, _ratio(got, want64, T))
        if ls is not None:
            none = want32[np.flatnonzero(ls < 0)]
            assert _same(none, np.broadcast_to(bias, none.shape))                        # no line: the bias alone
    print("forward F=%d: largest |err| / (2^-24 T) = %.3f over lines of up to %d kept entries" % (F, worst, 300))
    ones = _fwd((mat[0], mat[1], np.ones_like(mat[2])), None, 8, None, np.ones((N_GENES, F), np.float32),
                np.full(F, 2, np.float32), F, F, (True, False, True))
    assert np.array_equal(ones, np.array(LENGTHS + [300, 40], np.float32)[:, None] + 2 + np.zeros((1, F), np.float32))


@pytest.mark.parametrize("F", [65, 500])
def test_a_lines_bits_do_not_depend_on_its_place_or_its_neighbours(F):
    rng = np.random.default_rng(100 + F)
    mat = R.random_lines(rng, LENGTHS + [300, 40] + [int(n) for n in rng.integers(0, 120, 30)], N_GENES, integer=False)
    W, bias = rng.standard_normal((N_GENES, F)).astype(np.float32), rng.standard_normal(F).astype(np.float32)
    form = ((False, False, False), _up4(F), _up4(F))
    for line in (5, 6, 2):
        alone = _fwd(mat, np.array([line], np.int32), 1, None, W, bias, form[1], form[2], form[0])
        again = _fwd(mat, np.array([line], np.int32), 1, None, W, bias, form[1], form[2], form[0])
        assert _same(alone, again)                                                       # a second call
        many = rng.integers(0, len(mat[0]) - 1, 201).astype(np.int32)
        many[0] = many[200] = many[77] = line
        got = _fwd(mat, many, 201, None, W, bias, F + 1, F + 2, (True, True, True))      # other place, neighbours, alignment
        assert _same(got[0:1], alone) and _same(got[200:201], alone) and _same(got[77:78], alone)
        order = _fwd(mat, None, line + 1, None, W, bias, form[1], form[2], form[0])      # NULL lines: as row `line`
        assert _same(order[line:line + 1], alone)


def _array(rng, n_spots, lengths=None):
    """One array's CSC: lines = genes, idx = the spot's row within the array."""
    lengths = LENGTHS + [300, 40] + [int(n) for n in rng.integers(0, 90, 12)] if lengths is None else lengths
    return R.random_lines(rng, [min(n, n_spots) for n in lengths], n_spots, integer=False)


@pytest.mark.parametrize("F", FS)
def test_weight_gradient_is_the_documented_order_and_within_the_bound(F):
    rng = np.random.default_rng(1000 + F)
    n_spots, B = 350, 200
    mat = _array(rng, n_spots)
    n_lines = len(mat[0]) - 1
    pos = np.full(n_spots, -1, dtype=np.int32)
    pos[rng.choice(n_spots, size=B, replace=False)] = rng.permutation(B)
    dY = rng.standard_normal((B, F)).astype(np.float32)
    gene_lines = np.concatenate([rng.permutation(n_lines), [5, 5, -1, 3]]).astype(np.int32)
    worst = 0.0
    for gl, n in ((None, n_lines), (gene_lines, len(gene_lines))):
        want64, T, cnt = SL.wgrad64(*mat, gl, n, pos, dY)
        want32 = SL.wgrad32(*mat, gl, n, pos, dY)
        for offset, ld_dy, ldw in _forms(F):
            got = _wgrad(mat, gl, n, pos, dY, ld_dy, ldw, offset)
            assert _within(got, want64, T, cnt) and _same(got, want32), (offset, ld_dy, ldw)
            worst = max(worst, _ratio(got, want64, T))
        assert (want32[np.asarray(cnt) == 0] == 0).all() and (np.asarray(cnt) == 0).sum() >= 1   # zeros are written
    print("weight gradient F=%d: largest |err| / (2^-24 T) = %.3f" % (F, worst))
    # the batch permuted, the rows of dY along: the same bits
    perm = rng.permutation(B)
    pos2 = np.where(pos >= 0, perm[np.maximum(pos, 0)], -1).astype(np.int32)
    dY2 = np.empty_like(dY)
    dY2[perm] = dY
    form = _forms(F)[1]
    base = _wgrad(mat, None, n_lines, pos, dY, form[1], form[2], form[0])
    assert _same(_wgrad(mat, None, n_lines, pos2, dY2, form[1], form[2], form[0]), base)
    assert _same(_wgrad(mat, None, n_lines, pos, dY, form[1], form[2], form[0]), base)   # a second call
    # a second array on top (accumulate): array after array, the documented chain, and one more rounding in the bound
    mat2 = _array(rng, 280, [n for n in rng.integers(0, 150, n_lines)])
    posb = np.full(280, -1, dtype=np.int32)
    free = np.setdiff1d(np.arange(B + 60), pos[pos >= 0])[:60]
    posb[rng.choice(280, size=60, replace=False)] = free
    dYb = np.concatenate([dY, rng.standard_normal((60, F)).astype(np.float32)])
    first = _wgrad(mat, None, n_lines, pos, dYb, form[1], form[2], form[0])
    assert _same(first, base)                                                            # more rows in dY: nothing changes
    w64a, Ta, na = SL.wgrad64(*mat, None, n_lines, pos, dYb)
    w64b, Tb, nb = SL.wgrad64(*mat2, None, n_lines, posb, dYb)
    want32 = SL.wgrad32(*mat2, None, n_lines, posb, dYb, first)
    for offset, ld_dy, ldw in _forms(F)[:3]:
        got = _wgrad(mat2, None, n_lines, posb, dYb, ld_dy, ldw, offset, before=first, accumulate=1)
        assert _same(got, want32), (offset, ld_dy, ldw)
        assert _within(got, w64a + w64b, Ta + Tb, na + nb, extra=1)


def test_all_ones_weight_gradient_counts_the_hits():
    rng = np.random.default_rng(9)
    mat = _array(rng, 350)
    n = len(mat[0]) - 1
    pos = np.full(350, -1, dtype=np.int32)
    pos[::2] = np.arange(175)
    got = _wgrad((mat[0], mat[1], np.ones_like(mat[2])), None, n, pos, np.ones((175, 6), np.float32), 8, 8, (False, False, False))
    hits = [int((mat[1][mat[0][g]:mat[0][g + 1]] % 2 == 0).sum()) for g in range(n)]
    assert np.array_equal(got, np.array(hits, np.float32)[:, None] + np.zeros((1, 6), np.float32))
    again = _wgrad((mat[0], mat[1], np.ones_like(mat[2])), None, n, pos, np.ones((175, 6), np.float32), 8, 8, (False, False, False),
                   before=got, accumulate=1)
    assert np.array_equal(again, 2 * got)


@pytest.mark.parametrize("F", [5, 500])
def test_adjoint_identity(F):
    """<fwd(X), dY> = <W, wgrad(dY)> (no bias), in float64 of the fp32 results, within the two bounds' sum: each side is
    within sum |dY| gamma T_fwd, resp. sum |W| gamma T_wgrad, of the exact bilinear form."""
    import scipy.sparse as sp
    rng = np.random.default_rng(50 + F)
    n_spots, n_genes, B = 220, 260, 150
    X = sp.random(n_spots, n_genes, density=0.2, random_state=3, format='csr', dtype=np.float32)
    X.data = (rng.random(X.nnz).astype(np.float32) * 9 + 0.01)
    X.sort_indices()
    Xc = X.tocsc()
    Xc.sort_indices()
    csr = (X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.float32))
    csc = (Xc.indptr.astype(np.int64), Xc.indices.astype(np.int32), Xc.data.astype(np.float32))
    rows = rng.permutation(n_spots)[:B].astype(np.int32)
    pos = np.full(n_spots, -1, dtype=np.int32)
    pos[rows] = np.arange(B, dtype=np.int32)
    W, dY = rng.standard_normal((n_genes, F)).astype(np.float32), rng.standard_normal((B, F)).astype(np.float32)
    out = _fwd(csr, rows, B, None, W, None, _up4(F), _up4(F), (False, False, False))
    dW = _wgrad(csc, None, n_genes, pos, dY, _up4(F), _up4(F), (False, False, False))
    _, Tf, nf = SL.fwd64(*csr, rows, B, None, W, None)
    _, Tw, nw = SL.wgrad64(*csc, None, n_genes, pos, dY)
    left = float((out.astype(np.float64) * dY).sum())
    right = float((dW.astype(np.float64) * W).sum())
    bar = float((np.abs(dY) * SL.gamma(nf)[:, None] * Tf).sum() + (np.abs(W) * SL.gamma(nw)[:, None] * Tw).sum())
    print("adjoint F=%d: <fwd, dY> %.9g, <W, wgrad> %.9g, |difference| %.3g, bound %.3g" % (F, left, right, abs(left - right), bar))
    assert abs(left - right) <= bar


def test_refusals_and_empty_launches():
    lib = _L()
    ptr, idx, val = R.random_lines(np.random.default_rng(5), [3, 4], 10)
    p, i, v = _dev(ptr), _dev(idx), _dev(val)
    w = torch.full((10 * 8,), 1.0, device=DEV)
    out = torch.full((64,), NAN, device=DEV)
    P, I, V, Wp, O, S = p.data_ptr(), i.data_ptr(), v.data_ptr(), w.data_ptr(), out.data_ptr(), lib.stream()
    bad, uns, ok = lib.CONSTANTS['GNX_ERR_BAD_ARG'], lib.ERR_UNSUPPORTED, 0
    q = lib.query
    fwd = lambda **k: q('gnx_sparse_linear_fwd_f32', *[{**dict(lineptr=P, idx=I, val=V, lines=None, n_lines=2, chan_of_idx=None, W=Wp,   # noqa: E731
                                                           ldw=8, bias=None, out=O, ld_out=8, F=8, stream=S), **k}[n]
                                                   for n in lib.PARAMS['gnx_sparse_linear_fwd_f32']])
    wg = lambda **k: q('gnx_sparse_linear_wgrad_f32', *[{**dict(lineptr=P, idx=I, val=V, gene_lines=None, n_channels=2,                 # noqa: E731
                                                            pos_of_idx=None, dY=Wp, ld_dy=8, dW=O, ldw=8, F=8, accumulate=0, stream=S),
                                                        **k}[n] for n in lib.PARAMS['gnx_sparse_linear_wgrad_f32']])
    big_f = lib.query('gnx_sparse_linear_max_f') + 1
    assert big_f - 1 >= 4096
    for call, lds in ((fwd, ('ldw', 'ld_out')), (wg, ('ldw', 'ld_dy'))):
        count = 'n_lines' if call is fwd else 'n_channels'
        assert call(F=0) == bad and call(F=-1) == bad
        assert all(call(**{ld: 7}) == bad for ld in lds)                                 # a leading dimension below F
        assert call(**{count: -1}) == bad
        assert call(lineptr=None) == bad and call(idx=None) == bad and call(val=None) == bad
        assert call(val=V + 2) == bad                                                    # not 4-byte aligned
        assert call(**{count: 0}) == ok and call(**{count: 0, 'idx': None, 'val': None}) == ok
        assert call(**{count: 2 ** 31}) == uns
        assert call(F=big_f, **{ld: big_f for ld in lds}) == uns
    assert fwd(W=None) == bad and fwd(out=None) == bad and fwd(W=Wp + 2) == bad and fwd(out=O + 1) == bad and fwd(bias=Wp + 3) == bad
    assert wg(dY=None) == bad and wg(dW=None) == bad and wg(dY=Wp + 2) == bad and wg(dW=O + 2) == bad
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                        # nothing was launched
    assert fwd() == ok and wg(accumulate=0) == ok
    torch.cuda.synchronize()
    assert not torch.isnan(out[:16]).any() and torch.isnan(out[16:]).all()
