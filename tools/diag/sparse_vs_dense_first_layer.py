#!/usr/bin/env python3
"""What an epoch of `train_spotwise` costs with the tutorial count MLP on expanded rows and with the sparse first layer (public
API only).

    python tools/diag/sparse_vs_dense_first_layer.py [--batch 128] [--rounds 3] [--matrices 2000:0.1,33000:0.03]

Synthetic counts: two arrays of 78 x 64 = 4 992 spots (one trains, one validates) at each `genes:density` of `--matrices`, after
normalize_total(1e4).log1p(), resident on the device.  Three feeds of the same loop, one epoch each, alternating over
`--rounds` rounds:
  (a) dense, eager:   `SparseCountDataset` (one expand launch per batch) + the tutorial MLP, GNX_GRAPH=0;
  (b) dense, default: the same, the step captured and replayed as the loop does by default;
  (c) sparse:         `SparseCountDataset(as_rows=True)` + `SparseCountMLP` (eager: the loop does not capture it).
Per run: wall seconds of the epoch and the peak device memory over the memory held before the run.
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import pandas as pd
import scipy.sparse as sp
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga                                   # noqa: E402
from gridnext_amd.synthetic import count_mlp                # noqa: E402

DEV = 'cuda:0'
H, W, CLASSES = 78, 64, 4


def _counts(genes, density, rng):
    blocks, frames = [], []
    rows, cols = np.divmod(np.arange(H * W), W)
    for a in range(2):
        blocks.append(sp.random(H * W, genes, density=density, format='csr', random_state=rng,
                                data_rvs=lambda n: rng.integers(1, 60, n).astype(np.float64)))
        frames.append(pd.DataFrame({'x': 2 * cols + rows % 2, 'y': rows, 'array': 'array%d' % a,
                                    'annotation': ['c%d' % k for k in rng.integers(0, CLASSES, H * W)]}))
    return ga.SpotCounts(sp.vstack(blocks, format='csr'), pd.concat(frames, ignore_index=True), ['g%d' % g for g in range(genes)])


def _epoch(model, train, val, batch):
    """(wall seconds, peak bytes over the base) of one epoch of train_spotwise."""
    dl = {'train': DataLoader(train, batch_size=batch, shuffle=True, generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(val, batch_size=batch)}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        ga.train_spotwise(model, dl, nn.CrossEntropyLoss(), opt, num_epochs=1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--matrices', default='2000:0.1,33000:0.03')
    args = ap.parse_args()
    for spec in args.matrices.split(','):
        genes, density = int(spec.split(':')[0]), float(spec.split(':')[1])
        counts = _counts(genes, density, np.random.default_rng(0))
        counts.normalize_total(1e4).log1p()
        resident = counts.to(DEV)
        print("2 arrays x %d spots x %d genes, %.1f %% non-zero: %.1f MB resident; a dense array would be %.1f MB" %
              (H * W, genes, 100.0 * counts.nnz / (counts.n_spots * genes), resident.resident_bytes() / 1e6,
               4.0 * H * W * genes / 1e6), flush=True)
        classes = ga.SparseCountDataset(resident).classes
        views = [resident.subset_arrays([name]) for name in resident.arrays]
        dense_sets = [ga.SparseCountDataset(v, classes=classes) for v in views]
        row_sets = [ga.SparseCountDataset(v, classes=classes, as_rows=True) for v in views]

        def dense_model():
            torch.manual_seed(0)
            return count_mlp(genes, CLASSES)

        def sparse_model():
            torch.manual_seed(0)
            dense = count_mlp(genes, CLASSES)
            return ga.SparseCountMLP(ga.SparseCountLinear.from_linear(dense[0], resident), nn.Sequential(*list(dense)[1:]))
        feeds = (('dense, GNX_GRAPH=0', dense_model, dense_sets, '0'), ('dense, default    ', dense_model, dense_sets, None),
                 ('sparse first layer', sparse_model, row_sets, None))
        seen = {name: [] for name, _, _, _ in feeds}
        for r in range(args.rounds):
            for name, make, sets, graph in feeds:
                if graph is None:
                    os.environ.pop('GNX_GRAPH', None)
                else:
                    os.environ['GNX_GRAPH'] = graph
                t, peak = _epoch(make(), sets[0], sets[1], args.batch)
                seen[name].append((t, peak))
                print("G=%5d round %d  %s  %.4f s per epoch, peak %.1f MB over the base" % (genes, r, name, t, peak / 1e6), flush=True)
        os.environ.pop('GNX_GRAPH', None)
        for name, v in seen.items():
            ts = [t for t, _ in v]
            print("G=%5d batch %d  %s: median %.4f s per epoch [%.4f .. %.4f], peak %.1f MB" %
                  (genes, args.batch, name, float(np.median(ts)), min(ts), max(ts), max(p for _, p in v) / 1e6), flush=True)
        del resident, views, dense_sets, row_sets
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
