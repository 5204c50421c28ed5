"""gridnext_amd.metrics and utils.all_fgd_predictions_device on the device: the public functions against tests/metrics_ref.py
(numpy, CPU-tensor and HIP-tensor inputs), the warnings and errors, and a small GridNetHexOddr evaluated without its
predictions leaving the device.  The bars are those of test_gpu_metrics.py: counts and AUROC equal, AUPRC within
(T + 8) * 2^-53 of the exact rational."""
import math
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def data():
    """700 samples, 5 classes, scores quantised to 1/64 (ties) - shared, read-only."""
    rng = np.random.default_rng(0)
    n, C = 700, 5
    y = rng.integers(0, C, n).astype(np.int64)
    s = (np.round(rng.random((n, C)) * 64) / 64).astype(np.float32)
    s[np.arange(n), y] += np.float32(0.25)                # an informative classifier
    pred = s.argmax(1).astype(np.int64)
    return dict(n=n, C=C, y=y, s=s, pred=pred)


def forms(a):
    """The same array as numpy, CPU tensor and HIP tensor."""
    return a, torch.from_numpy(a), torch.from_numpy(a).to(DEV)


def check_aucs(auroc, auprc, y, s):
    auroc, auprc = auroc.cpu().numpy(), auprc.cpu().numpy()
    for c in range(s.shape[1]):
        thr, tps, fps = R.clf_curve_ref(y == c, s[:, c])
        want = R.auroc_exact(tps, fps)
        assert (math.isnan(want) and math.isnan(auroc[c])) or auroc[c] == want
        assert abs(auprc[c] - float(R.auprc_exact(tps, fps))) <= R.auc_bound(thr.size)


def test_inputs_of_every_kind_give_equal_results(data):
    from gridnext_amd import metrics as M
    results = []
    for y, s, p in zip(forms(data['y']), forms(data['s']), forms(data['pred'])):
        auroc, auprc = M.class_aucs(y, s)
        cm = M.confusion_matrix(y, p)
        curves = M.clf_curves(y, s)
        assert auroc.is_cuda and auprc.is_cuda and cm.is_cuda and curves[0][0].is_cuda
        assert auroc.dtype == torch.float64 and cm.dtype == torch.int64 and curves[0][1].dtype == torch.int64
        results.append((auroc, auprc, cm, curves))
    for other in results[1:]:
        assert torch.equal(other[0], results[0][0]) and torch.equal(other[1], results[0][1])
        assert torch.equal(other[2], results[0][2])
        for a, b in zip(other[3], results[0][3]):
            assert all(torch.equal(x, z) for x, z in zip(a, b))
    auroc, auprc, cm, curves = results[0]
    check_aucs(auroc, auprc, data['y'], data['s'])
    assert np.array_equal(cm.cpu().numpy(), R.confusion_matrix_ref(data['y'], data['pred']))
    for c, (thr, tps, fps) in enumerate(curves):
        r_thr, r_tps, r_fps = R.clf_curve_ref(data['y'] == c, data['s'][:, c])
        assert np.array_equal(thr.cpu().numpy(), r_thr.astype(np.float32))
        assert np.array_equal(tps.cpu().numpy(), r_tps) and np.array_equal(fps.cpu().numpy(), r_fps)


def test_plot_arrays(data):
    from gridnext_amd import metrics as M
    y, s = data['y'], data['s']
    for c in (0, 3):
        fpr, tpr, thr = M.roc_curve(y, s, c)
        r = R.roc_curve_ref(y == c, s[:, c])
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float64 for a in (fpr, tpr, thr))
        assert np.array_equal(fpr, r[0]) and np.array_equal(tpr, r[1]) and np.array_equal(thr, r[2])
        assert fpr[0] == 0 and tpr[0] == 0 and np.isinf(thr[0])
        prec, rec, thr = M.precision_recall_curve(torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV), c)
        r = R.pr_curve_ref(y == c, s[:, c])
        assert np.array_equal(prec, r[0]) and np.array_equal(rec, r[1]) and np.array_equal(thr, r[2])
        assert prec[-1] == 1 and rec[-1] == 0


def test_confusion_matrix_forms(data):
    from gridnext_amd import metrics as M
    y, p = data['y'], data['pred']
    holes_t, holes_p = np.array([0, 2, 5])[y % 3], np.array([0, 2, 5])[p % 3]
    holes_p[holes_t == 5] = 0
    holes_t[holes_t == 2] = 0                              # 2 is predicted, never true: an empty row
    cm = M.confusion_matrix(holes_t, holes_p)
    assert tuple(cm.shape) == (3, 3) and np.array_equal(cm.cpu().numpy(), R.confusion_matrix_ref(holes_t, holes_p))
    norm = M.confusion_matrix(holes_t, holes_p, normalize='true')
    assert norm.dtype == torch.float64 and np.array_equal(norm.cpu().numpy(), R.confusion_matrix_ref(holes_t, holes_p, 'true'))
    assert not norm[1].any()
    fixed = M.confusion_matrix(y, p, n_classes=8)
    assert tuple(fixed.shape) == (8, 8) and np.array_equal(fixed.cpu().numpy(), R.confusion_ref(y, p, 8)[0])
    with pytest.raises(ValueError, match="outside"):
        M.confusion_matrix(y, p, n_classes=3)
    with pytest.raises(ValueError, match="negative"):
        M.confusion_matrix(y - 1, p)
    with pytest.raises(ValueError, match="K <= 64"):       # the kernel's limit is named, not a generic failure of the call
        M.confusion_matrix(np.array([0, 100]), np.array([100, 0]))
    with pytest.raises(ValueError, match="K <= 64"):
        M.confusion_matrix(y, p, n_classes=65)
    top = M.confusion_matrix(np.array([0, 63]), np.array([63, 63]))
    assert np.array_equal(top.cpu().numpy(), np.array([[0, 1], [0, 1]]))


def test_performance_metrics_of_two_conditions(data):
    from gridnext_amd import metrics as M
    y, s = data['y'], data['s']
    s2 = np.ascontiguousarray(s[:, ::-1])                  # a second, worse condition
    with pytest.raises(AssertionError, match="Must provide names for each condition plotted"):
        M.performance_metrics(y, [s, s2])
    auroc, auprc, macro_roc, macro_pr = M.performance_metrics(y, [s, torch.from_numpy(s2).to(DEV)], condition_names=['a', 'b'])
    assert tuple(auroc.shape) == (data['C'], 2) and tuple(auprc.shape) == (data['C'], 2) and tuple(macro_roc.shape) == (2,)
    check_aucs(auroc[:, 0], auprc[:, 0], y, s)
    check_aucs(auroc[:, 1], auprc[:, 1], y, s2)
    assert torch.equal(macro_roc, auroc.mean(0)) and torch.equal(macro_pr, auprc.mean(0))
    one = M.performance_metrics(y, s, class_names=list('abcde'))
    assert tuple(one[0].shape) == (data['C'], 1) and torch.equal(one[0][:, 0], auroc[:, 0]) and torch.equal(one[3], macro_pr[:1])


def test_degenerate_classes_warn_and_propagate(data):
    from gridnext_amd import metrics as M
    y, s = data['y'].copy(), data['s']
    y[y == 4] = 0                                          # class 4 has no positives
    with pytest.warns(UserWarning, match="class 4: no positive"):
        auroc, auprc, macro_roc, macro_pr = M.performance_metrics(y, s)
    assert math.isnan(auroc[4, 0]) and auprc[4, 0] == 0.5 and math.isnan(macro_roc[0]) and not math.isnan(macro_pr[0])
    check_aucs(auroc[:, 0], auprc[:, 0], y, s)
    with pytest.warns(UserWarning, match="class 0: no negative"):
        auroc, auprc = M.class_aucs(np.zeros(50, dtype=np.int64), s[:50, :1])
    assert math.isnan(auroc[0]) and auprc[0] == 1.0
    with warnings.catch_warnings():
        warnings.simplefilter('error')                     # a well-posed problem warns about nothing
        M.class_aucs(data['y'], s)


def test_value_errors(data):
    from gridnext_amd import metrics as M
    s = data['s'].copy()
    s[3, 1] = np.nan
    s[9, 4] = np.nan
    with pytest.raises(ValueError, match="2 NaN"):
        M.class_aucs(data['y'], s)
    with pytest.raises(ValueError, match="NaN"):
        M.roc_curve(data['y'], s, 1)
    with pytest.raises(ValueError):
        M.class_aucs(data['y'][:-1], data['s'])
    smax = np.random.default_rng(1).random((3, 4, 5)).astype(np.float32)
    true = np.full((4, 5), 4)
    with pytest.raises(ValueError, match="above"):
        M.misclass_density(smax, true)


def test_misclass_density_public(data):
    from gridnext_amd import metrics as M
    rng = np.random.default_rng(3)
    smax = rng.random((7, 78, 64)).astype(np.float32)
    true = rng.integers(0, 8, (78, 64))
    want = torch.from_numpy(R.misclass_ref(smax, true))
    for s, t in zip(forms(smax), forms(true)):
        got = M.misclass_density(s, t)
        assert got.is_cuda and got.dtype == torch.float64 and torch.equal(got.cpu(), want)


def _hex_model_and_loader():
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    G, C, hw = 24, 4, (9, 7)
    torch.manual_seed(3)
    m = ga.GridNetHexOddr(count_mlp(G, C), (G,), hw, C)
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 10, (2, G) + hw, generator=g).float()
    y = torch.randint(0, C + 1, (2,) + hw, generator=g)
    return m, DataLoader(TensorDataset(x, y), batch_size=1), C


@pytest.mark.parametrize('f_only', [False, True])
def test_all_fgd_predictions_device(f_only):
    from gridnext_amd import metrics as M
    from gridnext_amd.utils import all_fgd_predictions, all_fgd_predictions_device
    m, dl, C = _hex_model_and_loader()
    true, pred, smax = all_fgd_predictions(dl, m, f_only=f_only)
    d_true, d_pred, d_smax = all_fgd_predictions_device(dl, m, f_only=f_only)
    assert d_true.is_cuda and d_pred.is_cuda and d_smax.is_cuda
    assert d_true.dtype == torch.int64 and d_pred.dtype == torch.int64 and d_smax.dtype == torch.float32
    assert np.array_equal(d_true.cpu().numpy(), true) and np.array_equal(d_pred.cpu().numpy(), pred)
    assert np.array_equal(d_smax.cpu().numpy(), smax) and smax.shape == (len(true), C)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                    # a class may be absent among 2 small arrays
        auroc, auprc = M.class_aucs(d_true, d_smax)
    check_aucs(auroc, auprc, true, smax)
    assert np.array_equal(M.confusion_matrix(d_true, d_pred, n_classes=C).cpu().numpy(), R.confusion_ref(true, pred, C)[0])


def test_against_sklearn_end_to_end(data):
    """The reference's expression (plotting.py:57-73) where sklearn is installed; skipped where it is not."""
    pytest.importorskip('sklearn')
    from sklearn.metrics import auc, precision_recall_curve, roc_curve
    from sklearn.preprocessing import label_binarize
    from gridnext_amd import metrics as M
    y, s = data['y'], data['s']
    onehot = label_binarize(y, classes=list(range(data['C'])))
    auroc, auprc, macro_roc, macro_pr = M.performance_metrics(y, s)
    for c in range(data['C']):
        bound = R.auc_bound(len(np.unique(s[:, c])))
        fpr, tpr, _ = roc_curve(onehot[:, c], s[:, c])
        prec, rec, _ = precision_recall_curve(onehot[:, c], s[:, c])
        d_roc, d_pr = abs(float(auroc[c, 0]) - auc(fpr, tpr)), abs(float(auprc[c, 0]) - auc(rec, prec))
        print("class %d: |auroc - sklearn| = %.3g, |auprc - sklearn| = %.3g, bound %.3g" % (c, d_roc, d_pr, bound))
        assert d_roc <= bound and d_pr <= bound
