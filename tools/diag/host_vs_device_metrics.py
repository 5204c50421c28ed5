#!/usr/bin/env python3
"""What the evaluation cell of the tutorials costs on the host and on the device (public API only).

    python tools/diag/host_vs_device_metrics.py [--rounds 3] [--sizes 59904,4194304]

Synthetic predictions of 7 classes (softmax of noise with the true class lifted) at one run's size (12 arrays of 4 992 spots) and
at 2^22 spots.  Per round, alternating, wall time of
  (a) host:   the reference's expression (gridnext/plotting.py:57-73): label_binarize, then per class sklearn's roc_curve,
              precision_recall_curve and two auc calls, on host arrays - skipped with a message where sklearn is not installed;
  (b) device: `metrics.performance_metrics(true, smax)` on resident tensors (one gnx_clf_curve call), synchronised; and the same
              with the results read back to the host (`.cpu()` of the four result tensors).
Reports the median and the spread, and how far the two sides' areas are apart.
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gridnext_amd import metrics as M                      # noqa: E402

DEV = 'cuda:0'
C = 7


def host_expression(true, smax):
    from sklearn.metrics import auc, precision_recall_curve, roc_curve
    from sklearn.preprocessing import label_binarize
    onehot = label_binarize(true, classes=list(range(C)))
    auroc, auprc = np.zeros(C), np.zeros(C)
    for c in range(C):
        fpr, tpr, _ = roc_curve(onehot[:, c], smax[:, c])
        auroc[c] = auc(fpr, tpr)
        precision, recall, _ = precision_recall_curve(onehot[:, c], smax[:, c])
        auprc[c] = auc(recall, precision)
    return auroc, auprc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sizes', default='%d,%d' % (12 * 4992, 1 << 22))
    args = ap.parse_args()
    try:
        import sklearn
        print("sklearn %s" % sklearn.__version__)
    except ImportError:
        sklearn = None
        print("sklearn is not installed here: the host side is skipped, the device side is timed alone")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    for n in (int(v) for v in args.sizes.split(',')):
        rng = np.random.default_rng(n % 1000)
        true = rng.integers(0, C, n).astype(np.int64)
        logits = rng.standard_normal((n, C)).astype(np.float32)
        logits[np.arange(n), true] += 1.5
        smax = torch.softmax(torch.from_numpy(logits), 1).numpy()
        d_true, d_smax = torch.from_numpy(true).to(DEV), torch.from_numpy(smax).to(DEV)
        M.performance_metrics(d_true[:64], d_smax[:64].contiguous())          # module load
        totals = {'host sklearn': [], 'device': [], 'device + readback': []}
        worst = 0.0
        for r in range(args.rounds):
            host, th = (None, float('nan'))
            if sklearn is not None:
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    host, th = timed(lambda: host_expression(true, smax))
            dev, td = timed(lambda: M.performance_metrics(d_true, d_smax))
            back, tb = timed(lambda: [t.cpu() for t in M.performance_metrics(d_true, d_smax)])
            if host is not None:
                worst = max(worst, float(np.abs(back[0][:, 0].numpy() - host[0]).max()),
                            float(np.abs(back[1][:, 0].numpy() - host[1]).max()))
            for k, t in zip(totals, (th, td, tb)):
                totals[k].append(t)
            print("n=%d round %d  host sklearn %.4f s | device %.5f s | device + readback %.5f s" % (n, r, th, td, tb), flush=True)
        for k, v in totals.items():
            print("n=%d %-18s median %.5f s, min %.5f s, max %.5f s" % (n, k, float(np.median(v)), min(v), max(v)))
        if sklearn is not None:
            print("n=%d ratio of medians host / device: %.0f; largest |device - sklearn| over the 14 areas: %.3g" %
                  (n, float(np.median(totals['host sklearn'])) / float(np.median(totals['device'])), worst))


if __name__ == '__main__':
    main()
