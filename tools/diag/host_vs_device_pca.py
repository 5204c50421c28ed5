#!/usr/bin/env python3
"""What fitting a PCA costs on the densified host matrix with sklearn and on resident sparse counts with `fit_pca` (public API
only).

    python tools/diag/host_vs_device_pca.py [--arrays 4] [--genes 2000] [--density 0.1] [--rounds 3]

Synthetic counts: `--arrays` arrays of 78 x 64 = 4 992 spots x `--genes` genes, about `--density` of the entries non-zero, after
normalize_total(1e4) and log1p.  Two routes to the same model (the recipe of the reference's scripts/fit_pca_unified_cortex.py
without its clipping):
  (a) host:   densify to float64 (N, G), z-score each gene, `sklearn.decomposition.PCA(svd_solver='full').fit`;
  (b) device: `SpotCounts.to(device).fit_pca(scale=True)`: one Gram launch per array, one (G, G) read-back, float64 eigh on the
              host.
Per round, alternating, wall time of each route (the densifying and the z-scoring count as part of (a): they are what the
route needs); then how far the two models are apart: eigenvalues relative to the largest, and the first components' angles.
"""
import argparse
import os
import sys
import time

import numpy as np
import pandas as pd
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga                                   # noqa: E402

DEV = 'cuda:0'
H, W = 78, 64


def _counts(arrays, genes, density, rng):
    blocks, frames = [], []
    rows, cols = np.divmod(np.arange(H * W), W)
    level = rng.gamma(2.0, 3.0, size=genes) + 0.5
    for a in range(arrays):
        m = sp.random(H * W, genes, density=density, format='csr', random_state=rng,
                      data_rvs=lambda n: rng.integers(1, 60, n).astype(np.float64))
        z = rng.normal(size=(H * W, 5)) * np.array([1.0, 0.8, 0.6, 0.45, 0.3])  # five spot factors, one per group of genes
        m = m.tocoo()
        m.data = np.ceil(m.data * level[m.col] / 10.0 * np.exp(z[m.row, m.col % 5]))      # genes differ in level
        blocks.append(m.tocsr())
        frames.append(pd.DataFrame({'x': 2 * cols + rows % 2, 'y': rows, 'array': 'array%d' % a, 'annotation': 'c0'}))
    return ga.SpotCounts(sp.vstack(blocks, format='csr'), pd.concat(frames, ignore_index=True), ['g%d' % g for g in range(genes)])


def _dense(counts):
    """(N, G) float64 of the stored values, through the public item path of the host dataset."""
    ds = ga.SparseCountDataset(counts)
    return torch.stack([x for x, _ in ds.__getitems__(range(len(ds)))]).double().numpy()


def _host_fit(counts):
    from sklearn.decomposition import PCA
    X = _dense(counts)
    std = X.std(0)
    X = (X - X.mean(0)) / np.where(std == 0, 1.0, std)
    return PCA(svd_solver='full').fit(X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arrays', type=int, default=4)
    ap.add_argument('--genes', type=int, default=2000)
    ap.add_argument('--density', type=float, default=0.1)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    counts = _counts(args.arrays, args.genes, args.density, rng)
    counts.normalize_total(1e4).log1p()
    resident = counts.to(DEV)
    torch.cuda.synchronize()
    print("%d arrays x %d spots x %d genes, %.1f %% non-zero; sparse counts %.1f MB on the device, the dense float64 matrix "
          "%.1f MB on the host" % (args.arrays, H * W, args.genes, 100.0 * counts.nnz / (counts.n_spots * args.genes),
                                   resident.resident_bytes() / 1e6, 8.0 * counts.n_spots * args.genes / 1e6), flush=True)
    resident.fit_pca(n_components=1)                                       # code objects loaded, maps built
    times = {'host   sklearn PCA on the dense matrix': [], 'device fit_pca on the resident counts ': []}
    for r in range(args.rounds):
        for name in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model = _host_fit(counts) if name.startswith('host') else resident.fit_pca(scale=True)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            print("round %d  %s  %.3f s" % (r, name, times[name][-1]), flush=True)
            if name.startswith('host'):
                sk = model
            else:
                pca = model
    for name, v in times.items():
        print("%s: median %.3f s, min %.3f, max %.3f" % (name, float(np.median(v)), min(v), max(v)))
    lam, ref = pca.explained_variance_.numpy(), sk.explained_variance_
    k = min(len(lam), len(ref))
    cos = np.abs((pca.components_.numpy()[:5] * sk.components_[:5]).sum(1))
    print("the two models: largest |d lambda| / lambda_1 = %.3g (G 2^-52 = %.3g); 1 - |cos| of the first five components: %s; "
          "PCs for half the variance: %d (device), %d (host)"
          % (np.abs(lam[:k] - ref[:k]).max() / ref[0], args.genes * 2.0 ** -52, ' '.join('%.2g' % (1 - c) for c in cos),
             pca.n_pcs_for(0.5), int(np.where(np.cumsum(sk.explained_variance_ratio_) > 0.5)[0][0]) + 1))


if __name__ == '__main__':
    main()
