#!/usr/bin/env python3
"""What an epoch of `train_gridwise` costs when its count grids come from the host and when they are expanded from resident
sparse counts (public API only).

    python tools/diag/host_vs_device_counts.py [--arrays 6] [--genes 2000] [--density 0.1] [--epochs 3] [--rounds 3]

Synthetic counts: `--arrays` arrays of 78 x 64 = 4 992 spots x `--genes` genes, about `--density` of the entries non-zero.  Two
feeds of the same loop (a frozen count MLP under a trained GridNetHexOddr, the last array for validation):
  (a) host:   a `TensorDataset` of the dense (G, 78, 64) grids on the host - what `load_count_grid_dataset` or the tutorial's
              `anndata_arrays_to_tensordataset` hands the loop; every item is copied to the device every epoch;
  (b) device: `SparseCountGridDataset` over `SpotCounts.to(device)`: one expand launch per array per epoch.
The two feed the same numbers (asserted: the grids and labels are equal).  Per round, alternating, wall time per epoch of
`train_gridwise` over `--epochs` epochs; and the resident bytes of each feed.
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
from torch.utils.data import DataLoader, Subset, TensorDataset

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga                                   # noqa: E402
from gridnext_amd.synthetic import count_mlp                # noqa: E402

DEV = 'cuda:0'
H, W, CLASSES = 78, 64, 4


def _counts(arrays, genes, density, rng):
    blocks, frames = [], []
    rows, cols = np.divmod(np.arange(H * W), W)
    for a in range(arrays):
        m = sp.random(H * W, genes, density=density, format='csr', random_state=rng,
                      data_rvs=lambda n: rng.integers(1, 60, n).astype(np.float64))
        blocks.append(m)
        frames.append(pd.DataFrame({'x': 2 * cols + rows % 2, 'y': rows, 'array': 'array%d' % a,
                                    'annotation': ['c%d' % k for k in rng.integers(0, CLASSES, H * W)]}))
    return ga.SpotCounts(sp.vstack(blocks, format='csr'), pd.concat(frames, ignore_index=True), ['g%d' % g for g in range(genes)])


def _epochs(dataset, n_train, epochs, genes):
    """Wall seconds per epoch of train_gridwise over `dataset` (the first n_train arrays train, the rest validate)."""
    torch.manual_seed(0)
    f = count_mlp(genes, CLASSES)
    for p in f.parameters():
        p.requires_grad = False
    m = ga.GridNetHexOddr(f, (genes,), (H, W), CLASSES)
    dl = {'train': DataLoader(Subset(dataset, range(n_train)), batch_size=1, shuffle=True,
                              generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(Subset(dataset, range(n_train, len(dataset))), batch_size=1)}
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        ga.train_gridwise(m, dl, nn.CrossEntropyLoss(), opt, num_epochs=epochs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arrays', type=int, default=6)
    ap.add_argument('--genes', type=int, default=2000)
    ap.add_argument('--density', type=float, default=0.1)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    counts = _counts(args.arrays, args.genes, args.density, rng)
    counts.normalize_total(1e4).log1p()
    t1 = time.perf_counter()
    resident = counts.to(DEV)
    torch.cuda.synchronize()
    print("%d arrays x %d spots x %d genes, %.1f %% non-zero: built and normalised on the host in %.2f s, uploaded in %.3f s" %
          (args.arrays, H * W, args.genes, 100.0 * counts.nnz / (counts.n_spots * args.genes), t1 - t0,
           time.perf_counter() - t1), flush=True)
    device_feed = ga.SparseCountGridDataset(resident)
    host_items = [ga.SparseCountGridDataset(counts)[k] for k in range(args.arrays)]
    host_feed = TensorDataset(torch.stack([x for x, _ in host_items]), torch.stack([y for _, y in host_items]))
    for k in range(args.arrays):
        x, y = device_feed[k]
        assert torch.equal(x.cpu(), host_feed[k][0]) and torch.equal(y.cpu(), host_feed[k][1]), "array %d differs" % k
    dense = sum(t.numel() * t.element_size() for t in host_feed.tensors)
    print("resident bytes: host TensorDataset %.1f MB (dense, on the host; %.1f MB cross to the device per epoch); sparse counts "
          "%.1f MB on the device (CSR + one CSC per array), one item of %.1f MB alive at a time" %
          (dense / 1e6, dense / 1e6, resident.resident_bytes() / 1e6, 4.0 * args.genes * H * W / 1e6), flush=True)
    n_train = max(1, args.arrays - 1)
    feeds = (('host  ', host_feed), ('device', device_feed))
    times = {name: [] for name, _ in feeds}
    for r in range(args.rounds):
        for name, ds in feeds:
            t = _epochs(ds, n_train, args.epochs, args.genes)
            times[name].append(t)
            print("round %d  %s  %.4f s per epoch" % (r, name, t), flush=True)
    for name, v in times.items():
        print("%s: %d arrays, %d epochs: median %.4f s per epoch, min %.4f, max %.4f" %
              (name, args.arrays, args.epochs, float(np.median(v)), min(v), max(v)))


if __name__ == '__main__':
    main()
