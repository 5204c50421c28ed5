"""csrc/sparse_gram.hip through the C ABI against tests/sparse_pca_ref.py: raw integer counts equal to the int64 product in every
form, normalised + log1p values per element within the DERIVED bound of a math.fsum reference, equal bits on a second call,
symmetry within the bound, the padding and the guards untouched, and every refusal.

Bound: an element is a sum of n products, each exact in double; any order of n - 1 additions lies within n 2^-53 sum |v u| of
the exact sum (tests/sparse_counts_ref.py: moments_bound).  Accumulating a second array is one more way to order the n1 + n2
terms.  Integer products whose sums stay below 2^53 are exact in every order.

Shapes: one array of 280 spots x 320 genes behind a 40-spot array in one CSR (row0 = 40), with CSC lines (genes) of 0, 1, 63, 64,
65 and 257 entries and CSR rows (spots) of 0, 1, 63, 64, 65 and 300 entries, the rest at 10 %; and 50 spots x 2049 genes at
0.4 % for the chunk sizes.

Measured on an MI355X (printed by the tests): see the README's count-PCA section."""
import numpy as np
import pytest
import torch

import sparse_counts_ref as R
import sparse_pca_ref as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
N0, N1, GENES = 40, 280, 320
LINE_LENGTHS = [0, 1, 63, 64, 65, 257]           # genes 0 .. 5
ROW_LENGTHS = [0, 1, 63, 64, 65, 300]            # spots 0 .. 5 of the second array
_made = {}


def _L():
    from gridnext_amd import _lib
    return _lib


def _dense():
    """Integer counts (N0 + N1, GENES): the special rows take their entries among the ordinary genes, the special genes among
    the ordinary spots, so both lists of lengths hold at once."""
    rng = np.random.default_rng(0)
    D = (rng.integers(1, 200, size=(N0 + N1, GENES)) * (rng.random((N0 + N1, GENES)) < 0.10)).astype(np.int64)
    D[N0:N0 + 6] = 0
    D[N0:, :6] = 0
    for g, n in enumerate(LINE_LENGTHS):
        D[N0 + 6 + rng.choice(N1 - 6, size=n, replace=False), g] = rng.integers(1, 200, size=n)
    for r, n in enumerate(ROW_LENGTHS):
        D[N0 + r, 6 + rng.choice(GENES - 6, size=n, replace=False)] = rng.integers(1, 200, size=n)
    assert [int((D[N0:, g] != 0).sum()) for g in range(6)] == LINE_LENGTHS
    assert [int((D[N0 + r] != 0).sum()) for r in range(6)] == ROW_LENGTHS
    return D


def _trios(D, starts):
    """(CSR of D, the CSC of every array D[starts[a]:starts[a + 1]]) as (int64 ptr, int32 idx, float32 val)."""
    import scipy.sparse as sp

    def trio(m):
        m.sort_indices()
        return m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float32)
    return trio(sp.csr_matrix(D)), [trio(sp.csc_matrix(D[a:b])) for a, b in zip(starts[:-1], starts[1:])]


def _matrices():
    """{'int': raw counts, 'log': the same after normalize_total(1e4) and log1p}: (dense, csr, [csc0, csc1]); built once."""
    if 'm' not in _made:
        D = _dense()
        log = R.normalise_log1p_dense(D)[0]
        _made['m'] = {'int': (D,) + _trios(D.astype(np.float32), [0, N0, N0 + N1]),
                      'log': (log,) + _trios(log, [0, N0, N0 + N1])}
    return _made['m']


def _dev(array, offset=False):
    if array is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(array))
    t = torch.empty(src.numel() + 1, dtype=src.dtype, device=DEV)
    t[int(offset):int(offset) + src.numel()] = src.reshape(-1).to(DEV)
    return t[int(offset):int(offset) + src.numel()]


def _run(csc, gene_lines, n, csr, row0, chan, ldc=None, offset=False, before=None, accumulate=0, twice=True):
    """C (n, n) float64 after one call (and, twice, the assertion that a second call gives equal bits).  C sits `offset` doubles
    into a NaN-filled storage with eight guard doubles behind; the padding [n, ldc) must still be NaN afterwards."""
    lib = _L()
    ldc = n if ldc is None else ldc
    args = [_dev(csc[0]), _dev(csc[1], offset), _dev(csc[2], offset), _dev(gene_lines), _dev(csr[0]), _dev(csr[1], offset),
            _dev(csr[2], offset), _dev(chan)]
    results = []
    for _ in range(2 if twice else 1):
        store = torch.full((n * ldc + 1 + 8,), NAN, dtype=torch.float64, device=DEV)
        C = store[int(offset):int(offset) + n * ldc]
        if before is not None:
            C.view(n, ldc)[:, :n] = torch.from_numpy(before).to(DEV)
        lib.call('gnx_sparse_gram_f64', lib.ptr(args[0], torch.int64), lib.ptr(args[1], torch.int32), lib.ptr(args[2]),
                 lib.ptr(args[3], torch.int32), n, lib.ptr(args[4], torch.int64), lib.ptr(args[5], torch.int32), lib.ptr(args[6]),
                 row0, lib.ptr(args[7], torch.int32), C.data_ptr(), ldc, accumulate, lib.stream())
        torch.cuda.synchronize()
        assert torch.isnan(store[:int(offset)]).all() and torch.isnan(store[int(offset) + n * ldc:]).all()
        got = C.view(n, ldc).cpu()
        assert torch.isnan(got[:, n:]).all() and not torch.isnan(got[:, :n]).any()         # padding untouched, body written
        results.append(got[:, :n].contiguous())
    if twice:
        assert torch.equal(results[0].view(torch.int64), results[1].view(torch.int64))   # equal bits on a second call
    return results[0].numpy()


def _view(rng, n, must=()):
    """(gene_lines, chan_of_idx) of a view on n of the GENES genes, in random order, `must` among them: lines and map agree,
    so the result is the Gram matrix of the view."""
    rest = np.setdiff1d(np.arange(GENES), must)
    genes = rng.permutation(np.concatenate([must, rng.choice(rest, size=n - len(must), replace=False)]).astype(np.int64))
    chan = np.full(GENES, -1, dtype=np.int32)
    chan[genes] = np.arange(n, dtype=np.int32)
    return genes.astype(np.int32), chan


def _forms(n):
    """(gene_lines, chan_of_idx, ldc, C one double into its storage, symmetric) at n channels."""
    rng = np.random.default_rng(n)
    special = np.arange(6)[:min(n, 6)]
    lines, chan = _view(rng, n, special)
    forms = [(None, None, n, False, True),                                               # NULL lists: the first n genes
             (lines, chan, n + 3, True, True)]                                           # a permuted view with -1s, padded, offset
    if n >= 3:
        odd = np.arange(n - 1, -1, -1).astype(np.int32)                                  # reversed, one row without a line
        odd[n // 2] = -1
        forms.append((odd, None, n + 1, False, False))
        forms.append((None, chan, n, True, False))                                       # lines in storage order, channels permuted
    return forms


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300])
def test_gram_of_one_array_in_every_form(n):
    m = _matrices()
    worst = 0.0
    for lines, chan, ldc, offset, symmetric in _forms(n):
        _, csr, cscs = m['int']
        got = _run(cscs[1], lines, n, csr, N0, chan, ldc, offset)
        want = P.gram_int(cscs[1], N1, lines, n, csr, N0, chan)
        assert int(want.max()) < 2 ** 53 and torch.equal(torch.from_numpy(got), torch.from_numpy(want).double())
        if lines is not None and (lines < 0).any():
            assert (got[lines < 0] == 0).all()                                           # no line: a row of zeros, written
        _, csr, cscs = m['log']
        got = _run(cscs[1], lines, n, csr, N0, chan, ldc, offset)
        want, terms, T = P.gram_fsum(cscs[1], N1, lines, n, csr, N0, chan)
        bound = P.gram_bound(terms, T)
        assert (np.abs(got - want) <= bound).all()
        assert (got[terms == 0] == 0).all()
        if symmetric:
            assert (np.abs(got - got.T) <= bound).all()
        worst = max(worst, float((np.abs(got - want)[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    print("gram n=%d: largest |err| / (n 2^-53 sum |v u|) = %.4f over sums of up to %d terms" % (n, worst, N1))


def test_special_lines_and_rows_are_in_the_view():
    """The lengths the shapes are about are really walked: the 300-channel view holds the six special genes, and the special
    spots' rows lie in the second array."""
    lines, chan, _, _, _ = _forms(300)[1]
    assert set(range(6)) <= set(lines.tolist())
    D = _matrices()['int'][0]
    kept = (chan >= 0)
    assert sorted(int((D[N0 + r][kept] != 0).sum()) for r in range(6))[-1] >= 257 and int((D[N0][kept] != 0).sum()) == 0


def test_two_arrays_accumulated():
    m = _matrices()
    lines, chan, _, _, _ = _forms(300)[1]
    for kind in ('int', 'log'):
        D, csr, cscs = m[kind]
        first = _run(cscs[0], lines, 300, csr, 0, chan, 301, True)
        both = _run(cscs[1], lines, 300, csr, N0, chan, 301, True, before=first, accumulate=1)
        if kind == 'int':
            sub = D[:, lines.astype(np.int64)]
            assert torch.equal(torch.from_numpy(both), torch.from_numpy(sub.T @ sub).double())
            assert torch.equal(torch.from_numpy(first), torch.from_numpy(sub[:N0].T @ sub[:N0]).double())
        else:
            w0, n0, T0 = P.gram_fsum(cscs[0], N0, lines, 300, csr, 0, chan)
            w1, n1, T1 = P.gram_fsum(cscs[1], N1, lines, 300, csr, N0, chan)
            bound = P.gram_bound(n0 + n1, T0 + T1) + 2.0 ** -53 * np.abs(w0 + w1)       # + the rounding of the reference's own sum
            assert (np.abs(both - (w0 + w1)) <= bound).all()
            print("two arrays accumulated: largest |err| / bound = %.4f" % float((np.abs(both - (w0 + w1))[bound > 0] / bound[bound > 0]).max()))


def test_chunk_sizes():
    """n_channels = chunk - 1, chunk, chunk + 1 on a very sparse matrix: the last column of a full chunk, the first of the next,
    entries on both sides of the edge in one row."""
    import scipy.sparse as sp
    chunk = _L().query('gnx_sparse_gram_chunk')
    assert chunk >= 256
    rng = np.random.default_rng(3)
    spots, genes = 50, chunk + 1
    D = (rng.integers(1, 200, size=(spots, genes)) * (rng.random((spots, genes)) < 0.004)).astype(np.int64)
    D[:4, chunk - 2:] = rng.integers(1, 200, size=(4, 3))                                # both sides of the edge, in four rows
    for kind, values in (('int', D.astype(np.float32)), ('log', R.normalise_log1p_dense(D)[0])):
        csr, (csc,) = _trios(values, [0, spots])
        for n in (chunk - 1, chunk, chunk + 1):
            got = _run(csc, None, n, csr, 0, None, n + (n % 2), bool(n % 2), twice=(kind == 'int'))
            if kind == 'int':
                S = sp.csr_matrix(D[:, :n])
                assert torch.equal(torch.from_numpy(got), torch.from_numpy(np.asarray((S.T @ S).todense())).double())
                assert got[n - 1, n - 1] > 0 and got[0:n, n - 1].sum() > got[n - 1, n - 1]
            else:
                want, terms, T = P.gram_fsum(csc, spots, None, n, csr, 0, None)
                assert (np.abs(got - want) <= P.gram_bound(terms, T)).all() and (np.abs(got - got.T) <= P.gram_bound(terms, T)).all()


def test_refusals_and_empty_launches():
    lib = _L()
    _, csr, cscs = _matrices()['int']
    t = [_dev(x) for x in (cscs[1][0], cscs[1][1], cscs[1][2], csr[0], csr[1], csr[2])]
    out = torch.full((16,), NAN, dtype=torch.float64, device=DEV)
    CP, CI, CV, RP, RI, RV = (x.data_ptr() for x in t)
    O, S = out.data_ptr(), lib.stream()
    bad, uns, ok = lib.CONSTANTS['GNX_ERR_BAD_ARG'], lib.ERR_UNSUPPORTED, 0
    base = dict(csc_ptr=CP, csc_idx=CI, csc_val=CV, gene_lines=None, n_channels=3, csr_ptr=RP, csr_idx=RI, csr_val=RV, row0=N0,
                chan_of_idx=None, C=O, ldc=4, accumulate=0, stream=S)
    assert list(lib.PARAMS['gnx_sparse_gram_f64']) == list(base)
    call = lambda **k: lib.query('gnx_sparse_gram_f64', *[{**base, **k}[n] for n in lib.PARAMS['gnx_sparse_gram_f64']])   # noqa: E731
    assert call(n_channels=-1) == bad and call(ldc=2) == bad and call(row0=-1) == bad
    assert call(csc_ptr=None) == bad and call(csr_ptr=None) == bad and call(C=None) == bad
    assert all(call(**{name: None}) == bad for name in ('csc_idx', 'csc_val', 'csr_idx', 'csr_val'))
    assert call(C=O + 4) == bad and call(csc_val=CV + 2) == bad and call(csr_val=RV + 1) == bad
    assert call(n_channels=0, ldc=0) == ok and call(n_channels=0, csc_idx=None, csc_val=None, csr_idx=None, csr_val=None) == ok
    assert call(n_channels=65535 * lib.query('gnx_sparse_gram_chunk') + 1, ldc=2 ** 40) == uns
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                        # nothing was launched, C untouched
    assert call() == ok
    torch.cuda.synchronize()
    got = out.cpu().view(4, 4)
    assert not torch.isnan(got[:3, :3]).any() and torch.isnan(got[:3, 3]).all() and torch.isnan(got[3]).all()
