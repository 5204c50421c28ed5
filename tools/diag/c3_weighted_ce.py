#!/usr/bin/env python3
"""What a criterion with options costs the count-f + hex-g loop (BASELINE config 3, as `tools/bench_configs.py --only c3`:
40 epochs x (8 train + 2 val) arrays of 78x64, batch 1, count MLP frozen): train_gridwise with a plain nn.CrossEntropyLoss()
and with nn.CrossEntropyLoss(weight=w, label_smoothing=0.1), the same model and data, alternating, `--rounds` times.

Public API only (gridnext_amd.train_gridwise, GridNetHexOddr, synthetic): the script runs on any commit of the project, so the
same file measures a commit whose loops take the generic path for the weighted criterion and one that fuses it.  One JSON line
per (round, criterion), then one summary line per criterion (median, min, max spots/s)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga                                   # noqa: E402
from gridnext_amd.synthetic import count_mlp, visium_array   # noqa: E402

DEV = 'cuda:0'
N_CLASSES = 8


def criteria():
    # class weights as inverse class frequencies come out: several-fold apart
    w = torch.tensor([0.3, 0.6, 1.0, 1.0, 1.5, 2.0, 3.0, 0.8], device=DEV)
    return {'plain': nn.CrossEntropyLoss(), 'weight + label_smoothing 0.1': nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)}


def loop(criterion, epochs, label, tag):
    xs, ys = [], []
    for a in range(10):
        _, xc, y = visium_array(a, image=False, device=DEV)
        xs.append(xc)
        ys.append(y)
    x, y = torch.stack(xs), torch.stack(ys)
    dl = {'train': DataLoader(TensorDataset(x[:8], y[:8]), batch_size=1, shuffle=True),
          'val': DataLoader(TensorDataset(x[8:], y[8:]), batch_size=1)}
    torch.manual_seed(0)
    m = ga.GridNetHexOddr(count_mlp(2000, N_CLASSES), (2000,), (78, 64), N_CLASSES)
    for p in m.patch_classifier.parameters():
        p.requires_grad = False
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        ga.train_gridwise(m, dl, criterion, opt, num_epochs=1)                                   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, vh, th = ga.train_gridwise(m, dl, criterion, opt, num_epochs=epochs)
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"tag": tag, "criterion": label, "spots_per_s": epochs * 10 * 4992 / dt, "arrays_per_s": epochs * 10 / dt, "seconds": dt,
            "last_train_loss": th[-1], "last_val_loss": vh[-1]}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--tag', default='', help="free text copied into every line (which commit this is)")
    args = ap.parse_args()
    seen = {}
    for r in range(args.rounds):
        for label, crit in criteria().items():
            res = loop(crit, args.epochs, label, args.tag)
            res["round"] = r
            seen.setdefault(label, []).append(res["spots_per_s"])
            print(json.dumps(res), flush=True)
    for label, v in seen.items():
        print(json.dumps({"tag": args.tag, "criterion": label, "rounds": len(v), "median_spots_per_s": statistics.median(v),
                          "min_spots_per_s": min(v), "max_spots_per_s": max(v)}), flush=True)
