"""gnx_clf_curve / gnx_confusion_counts / gnx_misclass_density (csrc/metrics.hip) through the C ABI against tests/metrics_ref.py
(which test_metrics_ref_host.py proves against sklearn).

Curve: thresholds (float bits), tps, fps and n_thresholds are EQUAL to the restatement; auroc is EQUAL to the correctly rounded
rational (2 P N < 2^53 at every size here); auprc is within (T + 8) * 2^-53 of the exact rational for n <= 3000 and of the
math.fsum of its float64 terms above - the bar derived in test_metrics_ref_host.py, which sklearn's own auc meets there.

Shapes: n = 1, 2, around a wave (63, 64, 65), around the tile one workgroup sorts per step (TILE - 1, TILE, TILE + 1), several
tiles with a ragged end (3 TILE + 17), one element more than G workgroups of one tile each hold (G TILE + 1: from there a
workgroup walks several tiles), and 1 048 579; C in {1, 2, 7, 33}; ld = C and ld = C + 3 (the padding columns hold NaN: reading
one shows in `bad`).  There is no single-workgroup form for small n: every size takes the same kernels.
Every output and the workspace sit between canary words."""
import math

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 4                                    # canary words on either side of every buffer
CANARY = {torch.float32: 12345.678, torch.float64: -9876.54321, torch.int64: 0x5A5A5A5A5A5A5A5A}
BIG = 1048579


def _consts():
    from gridnext_amd import _lib as L
    return int(L.query('gnx_clf_curve_tile')), int(L.query('gnx_clf_curve_max_groups')), int(L.query('gnx_confusion_max_classes'))


def sizes():
    tile, groups = 2048, 256                 # restated from csrc/metrics.hip; test_constants pins them to the library's
    return [1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 17, groups * tile + 1, BIG]


def test_constants():
    assert _consts() == (2048, 256, 64)


class Guarded:
    """A device buffer of `numel` elements between GUARD canary words on either side, filled with the canary as well."""

    def __init__(self, numel, dtype):
        self.full = torch.full((numel + 2 * GUARD,), CANARY[dtype], device=DEV, dtype=dtype)
        self.view = self.full[GUARD:GUARD + numel]
        self.dtype = dtype

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        want = torch.full((GUARD,), CANARY[self.dtype], device=DEV, dtype=self.dtype)
        return torch.equal(self.full[:GUARD], want) and torch.equal(self.full[-GUARD:], want)

    def untouched(self):
        return torch.equal(self.full, torch.full_like(self.full, CANARY[self.dtype]))


def upload(scores, ld):
    """float32 [n][C] on the host -> device [n][ld]; the padding columns hold NaN."""
    n, C = scores.shape
    m = np.full((n, ld), np.nan, dtype=np.float32)
    m[:, :C] = scores
    return torch.from_numpy(m).to(DEV)


def run_curve(d_scores, ld, d_y, n, C, curves=True, stream=None):
    """One gnx_clf_curve call by hand.  Returns (rc, dict of host arrays, list of the Guarded buffers)."""
    from gridnext_amd import _lib as L
    nbytes = L.query('gnx_clf_curve_workspace', n, C)
    assert nbytes > 0 and nbytes % 8 == 0
    bufs = dict(ws=Guarded(nbytes // 8, torch.int64), n_thr=Guarded(C, torch.int64), auroc=Guarded(C, torch.float64),
                auprc=Guarded(C, torch.float64), bad=Guarded(1, torch.int64))
    if curves:
        bufs.update(thr=Guarded(C * n, torch.float32), tps=Guarded(C * n, torch.int64), fps=Guarded(C * n, torch.int64))
    p = {k: (bufs[k].ptr() if k in bufs else None) for k in ('thr', 'tps', 'fps')}
    st = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()
    rc = L.query('gnx_clf_curve', d_scores.data_ptr(), ld, d_y.data_ptr(), n, C, p['thr'], p['tps'], p['fps'],
                 bufs['n_thr'].ptr(), bufs['auroc'].ptr(), bufs['auprc'].ptr(), bufs['bad'].ptr(), bufs['ws'].ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    out = {k: b.view.cpu().numpy() for k, b in bufs.items() if k != 'ws'}
    for k in ('thr', 'tps', 'fps'):
        if k in out:
            out[k] = out[k].reshape(C, n)
    return rc, out, bufs


def same_bits(a, b):
    """Every output of two calls, bit for bit, over the entries that are defined (the first T of a curve row)."""
    if not np.array_equal(a['n_thr'], b['n_thr']) or int(a['bad'][0]) != int(b['bad'][0]):
        return False
    if not (np.array_equal(a['auroc'].view(np.int64), b['auroc'].view(np.int64))
            and np.array_equal(a['auprc'].view(np.int64), b['auprc'].view(np.int64))):
        return False
    if 'thr' in a and 'thr' in b:
        for c, T in enumerate(a['n_thr'].tolist()):
            if not (np.array_equal(a['thr'][c, :T].view(np.int32), b['thr'][c, :T].view(np.int32))
                    and np.array_equal(a['tps'][c, :T], b['tps'][c, :T]) and np.array_equal(a['fps'][c, :T], b['fps'][c, :T])):
                return False
    return True


# ---------------------------------------------------------------------------------------------- score patterns
def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


PATTERNS = {
    'distinct': lambda rng, n: (rng.permutation(n).astype(np.float32) * np.float32(2.0 ** -21)),
    'equal': lambda rng, n: np.full(n, 0.375, dtype=np.float32),
    'two': lambda rng, n: rng.choice(np.array([0.25, 0.75], dtype=np.float32), n),
    'q64': lambda rng, n: (np.round(rng.random(n) * 64) / 64).astype(np.float32),
    'top_byte': lambda rng, n: _bits((rng.integers(0, 128, n).astype(np.uint32) << 24) | 0x00123456),
    'bottom_byte': lambda rng, n: _bits(np.uint32(0x3F000000) | rng.integers(0, 256, n).astype(np.uint32)),
    'neg_zero': lambda rng, n: np.where(rng.random(n) < 0.4, rng.choice(np.array([-0.0, 0.0], dtype=np.float32), n),
                                        (np.round((rng.random(n) - 0.5) * 32) / 32).astype(np.float32)).astype(np.float32),
    'denormal': lambda rng, n: _bits((rng.integers(0, 2, n).astype(np.uint32) << 31) | rng.integers(0, 48, n).astype(np.uint32)),
    'inf': lambda rng, n: np.where(rng.random(n) < 0.1, np.float32(np.inf),
                                   np.where(rng.random(n) < 0.1, np.float32(-np.inf), rng.random(n).astype(np.float32))),
    'random': lambda rng, n: rng.random(n).astype(np.float32),
    'ascending': lambda rng, n: np.sort(rng.random(n).astype(np.float32)),
    'descending': lambda rng, n: np.sort(rng.random(n).astype(np.float32))[::-1].copy(),
}
NAMES = list(PATTERNS)


def make_scores(n, C, seed=0, first=0):
    """float32 [n][C]: column c holds pattern (first + c) mod 12, so C = 33 holds every pattern at least twice."""
    rng = np.random.default_rng(1000 * seed + n % 9973)
    return np.stack([PATTERNS[NAMES[(first + c) % len(NAMES)]](rng, n).astype(np.float32) for c in range(C)], axis=1)


def check_against_ref(out, scores, y, n, C):
    assert int(out['bad'][0]) == 0
    for c in range(C):
        thr, tps, fps = R.clf_curve_ref(y == c, scores[:, c], kind='stable' if n <= 100000 else 'quicksort')
        T = thr.size
        assert int(out['n_thr'][c]) == T, (c, NAMES[c % len(NAMES)])
        assert np.array_equal(out['thr'][c, :T].view(np.int32), thr.astype(np.float32).view(np.int32)), c
        assert np.array_equal(out['tps'][c, :T], tps) and np.array_equal(out['fps'][c, :T], fps), c
        check_areas(out, c, tps, fps, n)


def check_areas(out, c, tps, fps, n):
    want = R.auroc_exact(tps, fps)
    got = float(out['auroc'][c])
    assert (math.isnan(got) and math.isnan(want)) or got == want, (c, got, want)
    exact = float(R.auprc_exact(tps, fps)) if n <= 3000 else R.auprc_fsum(tps, fps)
    err = abs(float(out['auprc'][c]) - exact)
    print("n %d class %d T %d auprc err %.3g bound %.3g" % (n, c, tps.size, err, R.auc_bound(tps.size)))
    assert err <= R.auc_bound(tps.size), (c, err)


def canaries_intact(bufs):
    return all(b.intact() for b in bufs.values())


# ---------------------------------------------------------------------------------------------- the curve
@pytest.mark.parametrize('C', [1, 2, 7, 33])
@pytest.mark.parametrize('n', sizes())
def test_curve_every_size(n, C):
    scores = make_scores(n, C, first=n % 5)
    y = np.random.default_rng(n + C).integers(0, C + 1, n).astype(np.int64)          # C: a label of no class
    d_y = torch.from_numpy(y).to(DEV)
    names = [NAMES[(n % 5 + c) % len(NAMES)] for c in range(C)]
    ref = None
    for ld in (C, C + 3):
        rc, out, bufs = run_curve(upload(scores, ld), ld, d_y, n, C)
        assert rc == 0 and canaries_intact(bufs), (ld, names)
        if ref is None:
            check_against_ref(out, scores, y, n, C)
            ref = out
        else:
            assert same_bits(out, ref), (ld, names)


@pytest.mark.parametrize('n', [1, 65, 2049, 3 * 2048 + 17, 256 * 2048 + 1])
def test_curve_every_pattern(n):
    C = len(NAMES)
    scores = make_scores(n, C)
    y = np.random.default_rng(n).integers(0, C, n).astype(np.int64)
    rc, out, bufs = run_curve(upload(scores, C), C, torch.from_numpy(y).to(DEV), n, C)
    assert rc == 0 and canaries_intact(bufs)
    check_against_ref(out, scores, y, n, C)
    if n > 1:
        k = NAMES.index('equal')
        assert int(out['n_thr'][k]) == 1
        assert int(out['n_thr'][NAMES.index('distinct')]) == n


@pytest.mark.parametrize('n', [1, 2, 65, 2049, 3 * 2048 + 17])
def test_curve_label_patterns(n):
    C = 3
    scores = make_scores(n, C, seed=3, first=3)          # q64, top_byte, bottom_byte
    rng = np.random.default_rng(n)
    labels = {
        'first': np.r_[0, np.full(n - 1, 1)],            # class 0: one positive, in front; class 2: no positives
        'last': np.r_[np.full(n - 1, 1), 0],
        'none': np.full(n, 7),                           # no class has a positive
        'all': np.full(n, 0),                            # class 0 has no negatives
        'outside': rng.integers(-2, C + 3, n),
        'huge': np.where(rng.random(n) < 0.5, np.int64(2) ** 40 + 1, rng.integers(0, C, n)),     # 2^40 + 1 is not class 1
    }
    d_s = upload(scores, C)
    for name, y in labels.items():
        y = y.astype(np.int64)
        rc, out, bufs = run_curve(d_s, C, torch.from_numpy(y).to(DEV), n, C)
        assert rc == 0 and canaries_intact(bufs), name
        check_against_ref(out, scores, y, n, C)
        if name == 'none':
            assert np.isnan(out['auroc']).all() and (out['auprc'] == 0.5).all()
        if name == 'all':
            assert math.isnan(out['auroc'][0]) and out['auprc'][0] == 1.0 and out['auprc'][1] == 0.5


@pytest.fixture(scope='module')
def wide():
    """33 columns at 3 TILE + 17 and one call over them, shared (read-only) by the tests below."""
    n, C = 3 * 2048 + 17, 33
    scores = make_scores(n, C, seed=7)
    y = np.random.default_rng(7).integers(0, C, n).astype(np.int64)
    d_s, d_y = upload(scores, C), torch.from_numpy(y).to(DEV)
    rc, out, bufs = run_curve(d_s, C, d_y, n, C)
    assert rc == 0 and canaries_intact(bufs)
    return dict(n=n, C=C, scores=scores, y=y, d_s=d_s, d_y=d_y, out=out)


def test_curve_same_bits_on_every_call(wide):
    for _ in range(2):
        rc, out, bufs = run_curve(wide['d_s'], wide['C'], wide['d_y'], wide['n'], wide['C'])
        assert rc == 0 and canaries_intact(bufs) and same_bits(out, wide['out'])


def test_curve_same_bits_alone_and_among_33(wide):
    n = wide['n']
    for c in (0, 5, 17, 32):
        alone = np.ascontiguousarray(wide['scores'][:, c:c + 1])
        y1 = np.where(wide['y'] == c, 0, -1).astype(np.int64)
        rc, out, bufs = run_curve(upload(alone, 1), 1, torch.from_numpy(y1).to(DEV), n, 1)
        assert rc == 0 and canaries_intact(bufs)
        T = int(out['n_thr'][0])
        big = wide['out']
        assert T == int(big['n_thr'][c])
        assert np.array_equal(out['thr'][0, :T].view(np.int32), big['thr'][c, :T].view(np.int32))
        assert np.array_equal(out['tps'][0, :T], big['tps'][c, :T]) and np.array_equal(out['fps'][0, :T], big['fps'][c, :T])
        assert out['auroc'].view(np.int64)[0] == big['auroc'].view(np.int64)[c]
        assert out['auprc'].view(np.int64)[0] == big['auprc'].view(np.int64)[c]


def test_curve_on_a_side_stream(wide):
    side = torch.cuda.Stream()
    rc, out, bufs = run_curve(wide['d_s'], wide['C'], wide['d_y'], wide['n'], wide['C'], stream=side)
    assert rc == 0 and canaries_intact(bufs) and same_bits(out, wide['out'])


def test_curve_without_curve_outputs(wide):
    rc, out, bufs = run_curve(wide['d_s'], wide['C'], wide['d_y'], wide['n'], wide['C'], curves=False)
    assert rc == 0 and canaries_intact(bufs) and same_bits(out, wide['out'])
    big_n = 256 * 2048 + 1
    scores = make_scores(big_n, 2, seed=9, first=9)
    y = np.random.default_rng(9).integers(0, 2, big_n).astype(np.int64)
    d_s, d_y = upload(scores, 2), torch.from_numpy(y).to(DEV)
    rc, full, bufs = run_curve(d_s, 2, d_y, big_n, 2)
    rc2, areas, bufs2 = run_curve(d_s, 2, d_y, big_n, 2, curves=False)
    assert rc == 0 and rc2 == 0 and canaries_intact(bufs) and canaries_intact(bufs2) and same_bits(areas, full)


def test_curve_counts_nan_scores():
    n, C = 2048 + 5, 3
    scores = make_scores(n, C, seed=11, first=9)
    scores[[0, 7, n - 1], 0] = np.nan
    scores[100:110, 2] = _bits(np.full(10, 0xFFC00001))          # negative NaNs with a payload
    y = np.random.default_rng(11).integers(0, C, n).astype(np.int64)
    for ld in (C, C + 3):
        rc, out, bufs = run_curve(upload(scores, ld), ld, torch.from_numpy(y).to(DEV), n, C)
        assert rc == 0 and canaries_intact(bufs) and int(out['bad'][0]) == 13


def test_curve_refusals_write_nothing():
    from gridnext_amd import _lib as L
    n, C = 65, 3
    d_s = upload(make_scores(n, C), C)
    d_y = torch.zeros(n, device=DEV, dtype=torch.int64)
    assert L.query('gnx_clf_curve_workspace', 0, C) == 0 and L.query('gnx_clf_curve_workspace', n, 0) == 0
    assert L.query('gnx_clf_curve_workspace', 2 ** 31, 1) == 0
    nws = L.query('gnx_clf_curve_workspace', n, C) // 8

    def attempt(**kw):
        b = dict(thr=Guarded(C * n, torch.float32), tps=Guarded(C * n, torch.int64), fps=Guarded(C * n, torch.int64),
                 n_thr=Guarded(C, torch.int64), auroc=Guarded(C, torch.float64), auprc=Guarded(C, torch.float64),
                 bad=Guarded(1, torch.int64), ws=Guarded(nws, torch.int64))
        a = dict(scores=d_s.data_ptr(), ld=C, y=d_y.data_ptr(), n=n, C=C, thr=b['thr'].ptr(), tps=b['tps'].ptr(), fps=b['fps'].ptr(),
                 n_thr=b['n_thr'].ptr(), auroc=b['auroc'].ptr(), auprc=b['auprc'].ptr(), bad=b['bad'].ptr(), ws=b['ws'].ptr())
        a.update(kw)
        rc = L.query('gnx_clf_curve', a['scores'], a['ld'], a['y'], a['n'], a['C'], a['thr'], a['tps'], a['fps'], a['n_thr'],
                     a['auroc'], a['auprc'], a['bad'], a['ws'], L.stream())
        torch.cuda.synchronize()
        assert all(g.untouched() for g in b.values()), kw
        return rc

    for kw in (dict(n=0), dict(n=-1), dict(C=0), dict(ld=C - 1), dict(scores=None), dict(y=None), dict(n_thr=None),
               dict(auroc=None), dict(auprc=None), dict(bad=None), dict(ws=None)):
        assert attempt(**kw) == -1, kw
    assert attempt(n=2 ** 31) == -3


# ---------------------------------------------------------------------------------------------- confusion counts
def run_confusion(y_true, y_pred, K):
    from gridnext_amd import _lib as L
    n = len(y_true)
    counts, bad = Guarded(max(K * K, 1), torch.int64), Guarded(1, torch.int64)
    d_t = torch.from_numpy(np.asarray(y_true, dtype=np.int64)).to(DEV) if n else torch.zeros(1, device=DEV, dtype=torch.int64)
    d_p = torch.from_numpy(np.asarray(y_pred, dtype=np.int64)).to(DEV) if n else torch.zeros(1, device=DEV, dtype=torch.int64)
    torch.cuda.synchronize()
    rc = L.query('gnx_confusion_counts', d_t.data_ptr(), d_p.data_ptr(), n, K, counts.ptr(), bad.ptr(), L.stream())
    torch.cuda.synchronize()
    return rc, counts, bad


@pytest.mark.parametrize('K', [1, 2, 7, 64])
def test_confusion_every_size(K):
    rng = np.random.default_rng(K)
    t_all, p_all = rng.integers(0, K, BIG), rng.integers(0, K, BIG)
    for n in sizes():
        t, p = t_all[:n], p_all[:n]
        rc, counts, bad = run_confusion(t, p, K)
        assert rc == 0 and counts.intact() and bad.intact(), n
        want, _ = R.confusion_ref(t, p, K)
        assert np.array_equal(counts.view.cpu().numpy().reshape(K, K), want) and int(bad.view.item()) == 0, n


def test_confusion_all_mass_on_one_cell():
    K = 7
    t, p = np.full(BIG, 5), np.full(BIG, 2)
    rc, counts, bad = run_confusion(t, p, K)
    want = np.zeros((K, K), dtype=np.int64)
    want[5, 2] = BIG
    assert rc == 0 and counts.intact() and np.array_equal(counts.view.cpu().numpy().reshape(K, K), want)
    assert int(bad.view.item()) == 0


@pytest.mark.parametrize('n', [1, 65, 3 * 2048 + 17])
def test_confusion_labels_outside_the_range(n):
    K = 7
    rng = np.random.default_rng(n)
    t, p = rng.integers(-2, K + 2, n), rng.integers(-2, K + 2, n)
    t[0] = 2 ** 40 + 3                                   # not label 3
    rc, counts, bad = run_confusion(t, p, K)
    want, n_bad = R.confusion_ref(t, p, K)
    assert rc == 0 and counts.intact() and bad.intact()
    assert np.array_equal(counts.view.cpu().numpy().reshape(K, K), want) and int(bad.view.item()) == n_bad and n_bad > 0


def test_confusion_refusals_write_nothing():
    limit = _consts()[2]
    for n, K, want in ((0, 7, -1), (-5, 7, -1), (10, 0, -1), (10, -1, -1), (10, limit + 1, -3)):
        from gridnext_amd import _lib as L
        counts, bad = Guarded(max(K * K, 1), torch.int64), Guarded(1, torch.int64)
        d = torch.zeros(16, device=DEV, dtype=torch.int64)
        rc = L.query('gnx_confusion_counts', d.data_ptr(), d.data_ptr(), n, K, counts.ptr(), bad.ptr(), L.stream())
        torch.cuda.synchronize()
        assert rc == want and counts.untouched() and bad.untouched(), (n, K)
    from gridnext_amd import _lib as L
    d = torch.zeros(16, device=DEV, dtype=torch.int64)
    assert L.query('gnx_confusion_counts', None, d.data_ptr(), 10, 2, d.data_ptr(), d.data_ptr(), L.stream()) == -1
    assert L.query('gnx_confusion_counts', d.data_ptr(), d.data_ptr(), 10, 2, None, d.data_ptr(), L.stream()) == -1
    assert L.query('gnx_confusion_counts', d.data_ptr(), d.data_ptr(), 10, 2, d.data_ptr(), None, L.stream()) == -1


# ---------------------------------------------------------------------------------------------- misclassification density
def run_misclass(smax, true):
    from gridnext_amd import _lib as L
    C, H, W = smax.shape
    out, bad = Guarded(H * W, torch.float64), Guarded(1, torch.int64)
    d_s, d_t = torch.from_numpy(smax).to(DEV), torch.from_numpy(true.astype(np.int64)).to(DEV)
    torch.cuda.synchronize()
    rc = L.query('gnx_misclass_density', d_s.data_ptr(), d_t.data_ptr(), C, H, W, out.ptr(), bad.ptr(), L.stream())
    torch.cuda.synchronize()
    assert out.intact() and bad.intact()
    return rc, out.view.cpu().reshape(H, W), int(bad.view.item())


@pytest.mark.parametrize('H,W,fg', [(78, 64, 'random'), (1, 1, 'random'), (78, 64, 'none')])
def test_misclass_density(H, W, fg):
    C = 7
    rng = np.random.default_rng(H)
    smax = rng.random((C, H, W)).astype(np.float32)
    true = rng.integers(0, C + 1, (H, W)) if fg == 'random' else np.zeros((H, W), dtype=np.int64)
    if (H, W) == (1, 1):
        true[0, 0] = C
    rc, got, bad = run_misclass(smax, true)
    assert rc == 0 and bad == 0
    assert got.dtype == torch.float64 and torch.equal(got, torch.from_numpy(R.misclass_ref(smax, true)))


def test_misclass_density_label_above_the_classes():
    C, H, W = 3, 5, 9
    rng = np.random.default_rng(2)
    smax = rng.random((C, H, W)).astype(np.float32)
    true = rng.integers(-1, C + 1, (H, W))
    true[1, 1], true[4, 8] = C + 1, 2 ** 40
    rc, got, bad = run_misclass(smax, true)
    ok = np.where(true > C, 0, true)
    assert rc == 0 and bad == 2 and torch.equal(got, torch.from_numpy(R.misclass_ref(smax, ok)))
