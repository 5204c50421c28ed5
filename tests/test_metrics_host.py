"""CPU: the host side of gridnext_amd.metrics - its names are exported, its entry points are declared on both sides of the
C ABI, and without a HIP device every call raises the package's usual error instead of computing on the host."""
import numpy as np
import pytest
import torch

ENTRY_POINTS = ('gnx_confusion_counts', 'gnx_clf_curve_workspace', 'gnx_clf_curve', 'gnx_misclass_density',
                'gnx_clf_curve_tile', 'gnx_clf_curve_max_groups', 'gnx_confusion_max_classes')


def test_names_are_exported():
    import gridnext_amd as ga
    from gridnext_amd import _lib, metrics, utils
    assert ga.metrics is metrics and ga.all_fgd_predictions_device is utils.all_fgd_predictions_device
    for name in ('confusion_matrix', 'clf_curves', 'roc_curve', 'precision_recall_curve', 'class_aucs', 'performance_metrics',
                 'misclass_density'):
        assert callable(getattr(metrics, name)), name
    handle = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
    assert _lib.query('gnx_clf_curve_workspace', 0, 7) == 0 and _lib.query('gnx_clf_curve_workspace', 100, 0) == 0
    # two element buffers, the digit table, the spans' sums, the totals, the partial sums: one workgroup per class at n = 100
    assert _lib.query('gnx_clf_curve_workspace', 100, 7) == 7 * (2 * 100 * 8 + 256 * 4 + 16 + 16 + 16)


def test_condition_names_are_required_before_anything_runs():
    from gridnext_amd import metrics
    with pytest.raises(AssertionError, match="Must provide names for each condition plotted"):
        metrics.performance_metrics(np.zeros(4, dtype=np.int64), [np.zeros((4, 2), dtype=np.float32)] * 2)


def test_no_cpu_path():
    if torch.cuda.is_available():
        pytest.skip("needs a CPU-only box")
    from gridnext_amd import metrics
    y, s = np.array([0, 1, 1, 0]), np.random.default_rng(0).random((4, 2)).astype(np.float32)
    for call in (lambda: metrics.class_aucs(y, s), lambda: metrics.clf_curves(torch.from_numpy(y), torch.from_numpy(s)),
                 lambda: metrics.roc_curve(y, s, 0), lambda: metrics.precision_recall_curve(y, s, 1),
                 lambda: metrics.performance_metrics(y, s), lambda: metrics.confusion_matrix(y, y),
                 lambda: metrics.misclass_density(s.reshape(2, 2, 2), y.reshape(2, 2))):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
