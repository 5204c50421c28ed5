"""numpy / pure-Python restatement of the evaluation metrics (sklearn's _binary_clf_curve, roc_curve, precision_recall_curve,
auc, confusion_matrix and the reference's misclass_density), for machines without sklearn.  test_metrics_ref_host.py proves it
against sklearn itself; the GPU tests compare the kernels with it."""
import math
from fractions import Fraction

import numpy as np


def clf_curve_ref(y, s, kind='stable'):
    """(thresholds, tps, fps) of a binary problem: y bool/0-1 [n], s float [n].  Distinct scores in descending order
    (-0.0 and +0.0 are one value, +0.0), int64 cumulative counts at the end of each tie group.  sklearn sorts stably; the
    counts are read at the ends of the tie groups only, so the order inside a group does not show and kind='quicksort' (four
    times as fast at a million scores) gives the same arrays - test_metrics_ref_host.py holds it to that."""
    y = np.asarray(y).astype(np.int64)
    s = np.asarray(s).astype(np.float64) + 0.0
    order = np.argsort(-s, kind=kind)
    s, y = s[order], y[order]
    ends = np.r_[np.where(s[1:] != s[:-1])[0], s.size - 1]       # np.diff's nonzeros, but inf - inf stays one tie group
    tps = np.cumsum(y, dtype=np.int64)[ends]
    fps = ends.astype(np.int64) + 1 - tps
    return s[ends], tps, fps


def auroc_exact(tps, fps):
    """The correctly rounded area under the ROC polygon, float(S / (2 P N)) as a rational; NaN without positives or
    negatives.  S = sum (fp_k - fp_{k-1}) (tp_k + tp_{k-1}) <= 2 P N is summed in Python ints for short curves and in int64
    (exact: no partial sum exceeds 2 P N < 2^62) for long ones."""
    P, N = int(tps[-1]), int(fps[-1])
    if P == 0 or N == 0:
        return float('nan')
    if len(tps) <= 4096:
        S, tp0, fp0 = 0, 0, 0
        for tp, fp in zip(tps.tolist(), fps.tolist()):
            S += (fp - fp0) * (tp + tp0)
            tp0, fp0 = tp, fp
    else:
        assert 2 * P * N < 2 ** 62
        t, f = np.r_[0, tps].astype(np.int64), np.r_[0, fps].astype(np.int64)
        S = int(np.sum((f[1:] - f[:-1]) * (t[1:] + t[:-1]), dtype=np.int64))
    return float(Fraction(S, 2 * P * N))


def auprc_exact(tps, fps):
    """sklearn 1.7's auc(recall, precision) as an exact rational (use for n <= 3000)."""
    P = int(tps[-1])
    if P == 0:
        return Fraction(1, 2)
    total, tp0, p0 = Fraction(0), 0, Fraction(1)
    for tp, fp in zip(tps.tolist(), fps.tolist()):
        p = Fraction(tp, tp + fp)
        total += Fraction(tp - tp0, P) * (p + p0) / 2
        tp0, p0 = tp, p
    return total


def auprc_fsum(tps, fps):
    """The same sum as math.fsum of float64 terms (each term a few roundings from its rational; the sum correctly rounded)."""
    P = int(tps[-1])
    if P == 0:
        return 0.5
    tp = tps.astype(np.float64)
    prec = tp / (tps + fps).astype(np.float64)
    dr = np.diff(np.r_[0, tps]).astype(np.float64) / float(P)
    pm = prec + np.r_[1.0, prec[:-1]]
    return math.fsum((dr * pm * 0.5).tolist())


def auc_bound(T):
    """|float64 area - exact rational| allowed: a float64 sum of T non-negative terms totalling at most 1 errs by at most
    T * 2^-53, and each term carries a few roundings more."""
    return (T + 8) * 2.0 ** -53


def roc_curve_ref(y, s):
    """sklearn's roc_curve(drop_intermediate=False): (fpr, tpr, thresholds) with the leading (0, 0) point, threshold inf."""
    thr, tps, fps = clf_curve_ref(y, s)
    tps, fps = np.r_[0, tps].astype(np.float64), np.r_[0, fps].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        fpr = fps / fps[-1] if fps[-1] > 0 else np.full(fps.shape, np.nan)
        tpr = tps / tps[-1] if tps[-1] > 0 else np.full(tps.shape, np.nan)
    return fpr, tpr, np.r_[np.inf, thr]


def pr_curve_ref(y, s):
    """sklearn 1.7's precision_recall_curve: (precision, recall, thresholds), ascending thresholds, trailing (1, 0)."""
    thr, tps, fps = clf_curve_ref(y, s)
    ps = (tps + fps).astype(np.float64)
    precision = np.zeros(tps.shape, dtype=np.float64)
    np.divide(tps, ps, out=precision, where=ps != 0)
    recall = np.ones(tps.shape, dtype=np.float64) if tps[-1] == 0 else tps / float(tps[-1])
    return np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0], thr[::-1]


def confusion_ref(y_true, y_pred, K):
    m = np.zeros((K, K), dtype=np.int64)
    t, p = np.asarray(y_true, dtype=np.int64), np.asarray(y_pred, dtype=np.int64)
    ok = (t >= 0) & (t < K) & (p >= 0) & (p < K)
    np.add.at(m, (t[ok], p[ok]), 1)
    return m, int((~ok).sum())


def confusion_matrix_ref(y_true, y_pred, normalize=None):
    """sklearn's confusion_matrix with labels=None: the sorted union of the values present."""
    t, p = np.asarray(y_true, dtype=np.int64), np.asarray(y_pred, dtype=np.int64)
    labels = np.union1d(t, p)
    m = confusion_ref(np.searchsorted(labels, t), np.searchsorted(labels, p), labels.size)[0]
    if normalize == 'true':
        with np.errstate(all='ignore'):
            m = np.nan_to_num(m / m.sum(axis=1, keepdims=True))
    return m


def misclass_ref(out_softmax, true):
    """The reference's double loop (gridnext/plotting.py:138-149) on numpy arrays."""
    ydim, xdim = true.shape
    mcd = np.zeros((ydim, xdim))
    for y in range(ydim):
        for x in range(xdim):
            if true[y, x] > 0:
                p_correct = out_softmax[true[y, x] - 1, y, x]
                mcd[y][x] = 1 - p_correct
    return mcd
