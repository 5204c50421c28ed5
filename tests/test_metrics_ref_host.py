"""CPU: tests/metrics_ref.py - the restatement the GPU tests compare the metric kernels with - against sklearn itself.

The accuracy bar of the areas is derived, not measured: a float64 sum of T non-negative terms totalling at most 1 errs by at
most T * 2^-53 and each term carries a few roundings more, so |value - exact rational| <= (T + 8) * 2^-53.  sklearn's own
`auc` is held to that bar here against the exact rationals (it meets it with a margin of about 30x on these inputs); the
kernels are held to the same bar in test_gpu_metrics.py."""
import math
import warnings

import numpy as np
import pytest

sklearn = pytest.importorskip('sklearn')
from sklearn import metrics as skm                      # noqa: E402
from sklearn.metrics._ranking import _binary_clf_curve  # noqa: E402

import metrics_ref as R                                 # noqa: E402

QUANTA = (0.25, 1.0 / 64, 1e-5, None)
RATES = (0.02, 0.3, 0.9)


def finite(s):
    """sklearn refuses an infinite score; the order, and with it every count and area, is the same with +inf replaced by a
    finite value above all others."""
    return np.where(np.isinf(s), np.float32(4.0), s).astype(np.float32)


def make_case(seed, n, quantum, rate, kind='uniform'):
    rng = np.random.default_rng(seed)
    s = rng.random(n).astype(np.float32)
    if kind == 'negative':
        s = (s - 0.5).astype(np.float32)
    if quantum is not None:
        s = (np.round(s / quantum) * quantum).astype(np.float32)
    if kind == 'zeros':
        s = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        s[rng.random(n) < 0.3] = np.float32(0.5)
        s[rng.random(n) < 0.2] = np.float32(-0.5)
    if kind == 'denormal':
        s = (rng.integers(-40, 40, n).astype(np.float32) * np.float32(1e-45)).astype(np.float32)
    if kind == 'inf':
        s[rng.random(n) < 0.1] = np.inf
    y = (rng.random(n) < rate).astype(np.int64)
    if y.sum() == 0:
        y[n // 2] = 1
    if y.sum() == n:
        y[n // 3] = 0
    return y, s


CASES = [(seed, n, q, rate, 'uniform') for seed, (n, q, rate) in
         enumerate([(n, q, rate) for n in (1, 2, 65, 700, 3000) for q in QUANTA for rate in RATES if n > 1 or q is None])]
CASES += [(100 + i, 900, q, 0.3, kind) for i, (q, kind) in
          enumerate([(None, 'negative'), (0.25, 'negative'), (None, 'zeros'), (None, 'denormal'), (None, 'inf'),
                     (1.0 / 64, 'inf')])]


@pytest.mark.parametrize('seed,n,quantum,rate,kind', CASES)
def test_curve_equals_sklearn(seed, n, quantum, rate, kind):
    y, s = make_case(seed, n, quantum, rate, kind)
    if n == 1:
        y[:] = 1
    fps_sk, tps_sk, thr_sk = _binary_clf_curve(y, finite(s))
    thr, tps, fps = R.clf_curve_ref(y, s)
    assert tps.dtype == np.int64 and fps.dtype == np.int64
    assert all(np.array_equal(a, b) for a, b in zip((thr, tps, fps), R.clf_curve_ref(y, s, kind='quicksort')))
    assert np.array_equal(finite(thr), thr_sk.astype(np.float64))
    s = finite(s)
    assert np.array_equal(tps, tps_sk.astype(np.int64)) and np.array_equal(fps, fps_sk.astype(np.int64))
    if y.min() == y.max():
        return
    fpr, tpr, t_roc = skm.roc_curve(y, s, drop_intermediate=False)
    r_fpr, r_tpr, r_thr = R.roc_curve_ref(y, s)
    assert np.array_equal(r_fpr, fpr) and np.array_equal(r_tpr, tpr) and np.array_equal(r_thr, t_roc.astype(np.float64))
    prec, rec, t_pr = skm.precision_recall_curve(y, s)
    r_prec, r_rec, r_tpr_thr = R.pr_curve_ref(y, s)
    assert np.array_equal(r_prec, prec) and np.array_equal(r_rec, rec) and np.array_equal(r_tpr_thr, t_pr.astype(np.float64))


@pytest.mark.parametrize('seed,n,quantum,rate,kind', [c for c in CASES if c[1] > 1])     # n = 1 has one class only
def test_sklearn_auc_meets_the_derived_bar(seed, n, quantum, rate, kind):
    y, s = make_case(seed, n, quantum, rate, kind)
    thr, tps, fps = R.clf_curve_ref(y, s)
    bound = R.auc_bound(thr.size)
    fpr, tpr, _ = skm.roc_curve(y, finite(s))
    prec, rec, _ = skm.precision_recall_curve(y, finite(s))
    exact_roc, exact_pr = R.auroc_exact(tps, fps), R.auprc_exact(tps, fps)
    assert abs(skm.auc(fpr, tpr) - exact_roc) <= bound
    assert abs(skm.auc(rec, prec) - float(exact_pr)) <= bound
    # the fsum form used above n = 3000 is itself within the bar of the rational
    assert abs(R.auprc_fsum(tps, fps) - float(exact_pr)) <= bound
    # and the exact AUROC is the rational, rounded once: the Mann-Whitney count agrees
    pos, neg = s[y == 1].astype(np.float64) + 0.0, s[y == 0].astype(np.float64) + 0.0
    if n <= 700:
        u2 = int(2 * (pos[:, None] > neg[None, :]).sum() + (pos[:, None] == neg[None, :]).sum())
        assert exact_roc == u2 / (2 * pos.size * neg.size)


def test_degenerate_classes():
    s = np.array([0.1, 0.4, 0.4, 0.8], dtype=np.float32)
    for y, want_pr in ((np.zeros(4, dtype=np.int64), 0.5), (np.ones(4, dtype=np.int64), 1.0)):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fpr, tpr, _ = skm.roc_curve(y, s)
            prec, rec, _ = skm.precision_recall_curve(y, s)
            assert math.isnan(skm.auc(fpr, tpr))
            assert skm.auc(rec, prec) == want_pr
        thr, tps, fps = R.clf_curve_ref(y, s)
        assert math.isnan(R.auroc_exact(tps, fps))
        assert float(R.auprc_exact(tps, fps)) == want_pr and R.auprc_fsum(tps, fps) == want_pr
        r_prec, r_rec, _ = R.pr_curve_ref(y, s)
        assert np.array_equal(r_prec, prec) and np.array_equal(r_rec, rec)
        r_fpr, r_tpr, _ = R.roc_curve_ref(y, s)
        assert np.array_equal(r_fpr, fpr, equal_nan=True) and np.array_equal(r_tpr, tpr, equal_nan=True)


@pytest.mark.parametrize('labels', [[0, 1, 2, 3, 4, 5, 6], [0, 2, 5], [3]])
def test_confusion_equals_sklearn(labels):
    rng = np.random.default_rng(len(labels))
    t, p = rng.choice(labels, 500), rng.choice(labels, 500)
    if len(labels) == 3:
        p[t == 5] = 0                      # label 5 is never predicted; its row is not empty
        t[t == 2] = 0                      # label 2 is never true: an empty row under normalize='true'
    assert np.array_equal(R.confusion_matrix_ref(t, p), skm.confusion_matrix(t, p))
    assert np.array_equal(R.confusion_matrix_ref(t, p, 'true'), skm.confusion_matrix(t, p, normalize='true'))
    K = max(labels) + 1
    assert np.array_equal(R.confusion_ref(t, p, K)[0], skm.confusion_matrix(t, p, labels=list(range(K))))


def test_misclass_ref_is_float32_subtraction():
    rng = np.random.default_rng(5)
    smax = rng.random((7, 6, 5)).astype(np.float32)
    true = rng.integers(0, 8, (6, 5))
    m = R.misclass_ref(smax, true)
    assert m.dtype == np.float64
    fg = true > 0
    picked = np.take_along_axis(smax, np.maximum(true - 1, 0)[None], 0)[0]
    assert np.array_equal(m[fg], (np.float32(1.0) - picked[fg]).astype(np.float64)) and not m[~fg].any()
