"""Evaluation metrics of a finished run, computed on the HIP device.

The numeric half of the reference's gridnext/plotting.py, which hands host arrays to sklearn:
  * `performance_metrics`  - `performance_curves` (:14-98) without the figure: one-vs-rest AUROC / AUPRC per class and
    condition and their macro means; `class_aucs`, `clf_curves`, `roc_curve`, `precision_recall_curve` are its parts;
  * `confusion_matrix`     - sklearn's, as `plot_confusion` (:103-134) calls it;
  * `misclass_density`     - the per-spot misclassification map (:138-149).
Inputs are numpy arrays, CPU tensors or HIP tensors (`utils.all_fgd_predictions_device` keeps a run's predictions on the
device); host inputs are uploaded to `distributed.default_device()`.  Scores are float32, the type of the package's softmax:
scores of another type (float64, float16) are CAST to float32 first, so values that differ only beyond float32 fall into one
tie group and thresholds are the float32 values - sklearn on the same float64 array keeps them apart.
All counting, ordering and integration runs in the kernels of csrc/metrics.hip; there is no CPU path and sklearn is not
needed.  Results are tensors on the device unless a function says otherwise.  Workspaces are allocated per call; nothing is
cached.
"""
import warnings

import numpy as np
import torch

from . import _lib as L
from . import distributed as gdist


def _device_tensor(x, dtype, what):
    """`x` (numpy array, CPU tensor or HIP tensor) as a contiguous tensor of `dtype` on a HIP device."""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))
    if not t.is_cuda:
        dev = gdist.default_device()
        if dev.type != 'cuda':
            raise RuntimeError("gridnext_amd.metrics needs a HIP device for %s; there is no CPU path" % what)
        t = t.to(dev)
    if t.dtype != dtype:
        if dtype == torch.int64 and (t.is_floating_point() or t.dtype == torch.bool):
            raise TypeError("%s must hold integer labels, got %s" % (what, t.dtype))
        t = t.to(dtype)
    return t.contiguous()


def _labels(x, what):
    return _device_tensor(x, torch.int64, what).reshape(-1)


def _scores(x, what='scores'):
    """`x` as float32 (n_samples, n_classes) on the device; any other floating type is cast to float32 (module docstring)."""
    s = _device_tensor(x, torch.float32, what)
    if s.dim() != 2:
        raise ValueError("%s must be (n_samples, n_classes), got %s" % (what, tuple(s.shape)))
    return s


def _counts(y_true, y_pred, K):
    dev = y_true.device
    counts = torch.empty((K, K), device=dev, dtype=torch.int64)
    bad = torch.empty(1, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        L.call('gnx_confusion_counts', y_true.data_ptr(), y_pred.data_ptr(), y_true.numel(), K, counts.data_ptr(),
               bad.data_ptr(), L.stream())
    return counts, int(bad.item())


def confusion_matrix(y_true, y_pred, n_classes=None, normalize=None):
    """sklearn's confusion_matrix: int64 (K, K), rows true, columns predicted.  n_classes=None: the labels are the sorted union
    of the values present; n_classes=K: the labels are 0..K-1 and a label outside raises ValueError.  normalize='true':
    float64 rows divided by their sums, an empty row gives zeros.  The kernel counts labels 0..K-1 with K <= 64 (K = the
    largest label + 1 when n_classes is None): a larger K raises ValueError."""
    if normalize not in (None, 'true'):
        raise ValueError("normalize must be None or 'true'")
    yt, yp = _labels(y_true, 'y_true'), _labels(y_pred, 'y_pred')
    if yp.device != yt.device:
        yp = yp.to(yt.device)
    if yt.numel() != yp.numel():
        raise ValueError("y_true and y_pred differ in length: %d, %d" % (yt.numel(), yp.numel()))
    if yt.numel() == 0:
        raise ValueError("confusion_matrix of no samples")
    if n_classes is None:
        lo = int(torch.minimum(yt.min(), yp.min()).item())
        if lo < 0:
            raise ValueError("labels must not be negative (found %d)" % lo)
        K = int(torch.maximum(yt.max(), yp.max()).item()) + 1
    else:
        K = int(n_classes)
        if K <= 0:
            raise ValueError("n_classes must be positive, got %d" % K)
    k_max = int(L.query('gnx_confusion_max_classes'))
    if K > k_max:
        raise ValueError("confusion_matrix counts labels 0..K-1 for K <= %d; %s gives K = %d" %
                         (k_max, "the largest label present" if n_classes is None else "n_classes", K))
    counts, bad = _counts(yt, yp, K)
    if bad:
        raise ValueError("%d samples carry a label outside [0, %d)" % (bad, K))
    if n_classes is None:
        present = ((counts.sum(0) + counts.sum(1)) > 0).nonzero().reshape(-1)
        counts = counts.index_select(0, present).index_select(1, present)
    if normalize == 'true':
        sums = counts.sum(1, keepdim=True).double()
        counts = torch.where(sums > 0, counts.double() / sums.clamp(min=1.0), torch.zeros_like(sums))
    return counts


def _curve_call(y_true, scores, curves):
    """One gnx_clf_curve over all columns: (thresholds, tps, fps, n_thresholds, auroc, auprc); the first three None unless
    `curves`.  Raises ValueError on NaN scores."""
    s, y = _scores(scores), _labels(y_true, 'y_true')
    if y.device != s.device:
        y = y.to(s.device)
    n, C = s.shape
    if y.numel() != n:
        raise ValueError("y_true has %d entries, scores %d rows" % (y.numel(), n))
    if n == 0 or C == 0:
        raise ValueError("scores must not be empty, got %s" % (tuple(s.shape),))
    dev = s.device
    nbytes = L.query('gnx_clf_curve_workspace', n, C)
    if nbytes <= 0:
        raise RuntimeError("gnx_clf_curve does not take n = %d, C = %d" % (n, C))
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    thr = torch.empty((C, n), device=dev, dtype=torch.float32) if curves else None
    tps = torch.empty((C, n), device=dev, dtype=torch.int64) if curves else None
    fps = torch.empty((C, n), device=dev, dtype=torch.int64) if curves else None
    n_thr = torch.empty(C, device=dev, dtype=torch.int64)
    auroc = torch.empty(C, device=dev, dtype=torch.float64)
    auprc = torch.empty(C, device=dev, dtype=torch.float64)
    bad = torch.empty(1, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        L.call('gnx_clf_curve', s.data_ptr(), C, y.data_ptr(), n, C, L.ptr(thr), L.ptr(tps, torch.int64),
               L.ptr(fps, torch.int64), n_thr.data_ptr(), auroc.data_ptr(), auprc.data_ptr(), bad.data_ptr(), ws.data_ptr(),
               L.stream())
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError("scores contain %d NaN" % n_bad)
    return thr, tps, fps, n_thr, auroc, auprc, y


def _warn_degenerate(y, C):
    """sklearn's warnings for the classes whose areas are not defined, naming the class."""
    present = torch.bincount(y[(y >= 0) & (y < C)], minlength=C).cpu().tolist()
    n = y.numel()
    for c, p in enumerate(present):
        if p == 0:
            warnings.warn("class %d: no positive samples in y_true, true positive value should be meaningless "
                          "(auroc is nan, auprc 0.5)" % c, UserWarning, stacklevel=3)
        elif p == n:
            warnings.warn("class %d: no negative samples in y_true, false positive value should be meaningless "
                          "(auroc is nan, auprc 1.0)" % c, UserWarning, stacklevel=3)


def clf_curves(y_true, scores):
    """sklearn's _binary_clf_curve of every class against the rest: a list, one entry per column of `scores`, of
    (thresholds float32 [T], tps int64 [T], fps int64 [T]) on the device - the distinct scores in descending order and the
    cumulative counts of positives (y_true == c) and negatives (anything else) at or above each."""
    thr, tps, fps, n_thr, _, _, _ = _curve_call(y_true, scores, True)
    return [(thr[c, :T], tps[c, :T], fps[c, :T]) for c, T in enumerate(n_thr.cpu().tolist())]


def _one_curve(y_true, scores, c):
    s = _scores(scores)
    if not 0 <= c < s.shape[1]:
        raise ValueError("class %d outside the %d columns of scores" % (c, s.shape[1]))
    y = _labels(y_true, 'y_true')
    one = -(y.to(s.device) != c).long()              # column c alone is class 0 of the call: 0 = positive, -1 = negative
    thr, tps, fps, n_thr, _, _, _ = _curve_call(one, s[:, c:c + 1], True)
    T = int(n_thr.item())
    return (thr[0, :T].cpu().numpy().astype(np.float64), tps[0, :T].cpu().numpy().astype(np.float64),
            fps[0, :T].cpu().numpy().astype(np.float64))


def roc_curve(y_true, scores, c):
    """sklearn's roc_curve(y_true == c, scores[:, c], drop_intermediate=False) as numpy float64 (fpr, tpr, thresholds), with
    the leading (0, 0) point and its inf threshold.  A class without negatives (positives) has a NaN fpr (tpr) and warns."""
    thr, tps, fps = _one_curve(y_true, scores, c)
    tps, fps = np.r_[0.0, tps], np.r_[0.0, fps]
    if fps[-1] <= 0:
        warnings.warn("class %d: no negative samples in y_true, false positive value should be meaningless" % c, UserWarning,
                      stacklevel=2)
        fpr = np.full(fps.shape, np.nan)
    else:
        fpr = fps / fps[-1]
    if tps[-1] <= 0:
        warnings.warn("class %d: no positive samples in y_true, true positive value should be meaningless" % c, UserWarning,
                      stacklevel=2)
        tpr = np.full(tps.shape, np.nan)
    else:
        tpr = tps / tps[-1]
    return fpr, tpr, np.r_[np.inf, thr]


def precision_recall_curve(y_true, scores, c):
    """sklearn 1.7's precision_recall_curve(y_true == c, scores[:, c]) as numpy float64 (precision, recall, thresholds):
    ascending thresholds, the trailing (precision 1, recall 0) point.  Without positives recall is one throughout (warns)."""
    thr, tps, fps = _one_curve(y_true, scores, c)
    precision = tps / (tps + fps)                    # tps + fps >= 1 at every threshold
    if tps[-1] <= 0:
        warnings.warn("class %d: no positive class found in y_true, recall is set to one for all thresholds" % c, UserWarning,
                      stacklevel=2)
        recall = np.ones(tps.shape)
    else:
        recall = tps / tps[-1]
    return np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0], thr[::-1].copy()


def class_aucs(y_true, scores):
    """(auroc [C], auprc [C]) float64 on the device: the areas under every class's one-vs-rest ROC and precision-recall curve.
    auroc is the correctly rounded exact area (one division of integers); auprc is sklearn's auc(recall, precision), summed in
    a fixed order, so equal inputs give equal bits.  A class without positives gives (nan, 0.5), one without negatives
    (nan, 1.0); both warn."""
    _, _, _, _, auroc, auprc, y = _curve_call(y_true, scores, False)
    _warn_degenerate(y, auroc.numel())
    return auroc, auprc


def performance_metrics(true, smax, class_names=None, condition_names=None):
    """The numbers of the reference's `performance_curves`: (auroc [C, n_cond], auprc [C, n_cond], macro_auroc [n_cond],
    macro_auprc [n_cond]) float64 on the device.  `smax`: (n_samples, n_classes) class probabilities, or a list of them (one
    per condition, which then needs `condition_names`).  The macro values are plain means over the classes, as in the
    reference: a NaN propagates.  `class_names` only label the reference's sub-plots and are accepted for its signature."""
    if isinstance(smax, (list, tuple)):
        assert condition_names is not None, "Must provide names for each condition plotted"
        smax = list(smax)
    else:
        smax = [smax]
        condition_names = ['']
    if len(condition_names) != len(smax):
        raise ValueError("%d condition names for %d conditions" % (len(condition_names), len(smax)))
    n_classes = _scores(smax[0], 'smax').shape[1]
    if class_names is not None and len(class_names) != n_classes:
        raise ValueError("%d class names for %d classes" % (len(class_names), n_classes))
    aurocs, auprcs = [], []
    for s in smax:
        s = _scores(s, 'smax')
        if s.shape[1] != n_classes:
            raise ValueError("conditions differ in their number of classes")
        a, p = class_aucs(true, s)
        aurocs.append(a)
        auprcs.append(p.to(a.device))
    auroc = torch.stack([a.to(aurocs[0].device) for a in aurocs], 1)
    auprc = torch.stack([p.to(aurocs[0].device) for p in auprcs], 1)
    return auroc, auprc, auroc.mean(0), auprc.mean(0)


def misclass_density(out_softmax, true):
    """The reference's misclassification map: float64 (H, W) on the device, 1 - out_softmax[true - 1, y, x] (a float32
    subtraction, as numpy's on float32 probabilities) at foreground spots (true > 0), 0 at background.  out_softmax:
    (n_classes, H, W); true: (H, W) integer labels, 0 = background.  A label above n_classes raises ValueError."""
    s = _device_tensor(out_softmax, torch.float32, 'out_softmax')
    t = _device_tensor(true, torch.int64, 'true')
    if t.device != s.device:
        t = t.to(s.device)
    if s.dim() != 3 or t.dim() != 2 or tuple(s.shape[1:]) != tuple(t.shape):
        raise ValueError("out_softmax must be (n_classes, H, W) and true (H, W), got %s and %s" % (tuple(s.shape), tuple(t.shape)))
    C, H, W = s.shape
    out = torch.empty((H, W), device=s.device, dtype=torch.float64)
    bad = torch.empty(1, device=s.device, dtype=torch.int64)
    with torch.cuda.device(s.device):
        L.call('gnx_misclass_density', s.data_ptr(), t.data_ptr(), C, H, W, out.data_ptr(), bad.data_ptr(), L.stream())
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError("%d spots carry a label above the %d classes of out_softmax" % (n_bad, C))
    return out
