#!/usr/bin/env python3
"""What an epoch of `train_gridwise` costs when its arrays come from JPEG patch files and when they come from resident slides
(public API only).

    python tools/diag/slides_vs_jpeg_epochs.py [--slides 3] [--slide 6000] [--patch 32] [--window 48] [--epochs 3] [--rounds 3]

A few synthetic slides (uint8, `--slide` pixels square, written as TIFF) with Spaceranger-style position trees of 78 x 64 = 4 992
in-tissue spots on Visium spacing and a Loupe annotation CSV each, in a temporary directory.  Two feeds of the same loop (a frozen
small DenseNet under a trained GridNetHexOddr, the last array for validation):
  (a) files:  `save_visium_patches_all(..., device=...)` once (timed on its own), then `PatchGridDataset(raw_uint8=True)`: 4 992
              JPEGs decoded per array per epoch, the grid moved to the device by the loop's prefetcher;
  (b) slides: `SlideGridDataset(device=..., remove_cast=...)`: slides uploaded on first use, one gather per array per epoch.
Per round, alternating, wall time per epoch of `train_gridwise` over `--epochs` epochs, without and with `enable_f_cache()`.
The two feeds do not give the same numbers (JPEG is lossy); the label grids are asserted equal.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn as nn
from PIL import Image
from torch.utils.data import DataLoader, Subset

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga                                   # noqa: E402
from gridnext_amd import imgprocess as IP                  # noqa: E402

DEV = 'cuda:0'
CLASSES = ('a', 'b', 'c', 'd')


def _array(tmp, k, S, rng):
    """Slide k as a TIFF, its position tree and its annotation CSV: (image file, spaceranger dir, annotation file)."""
    base = rng.integers(1, 256, (S // 8 + 1, S // 8 + 1, 3), dtype=np.uint8)          # blocks of 8 x 8: JPEG-friendly
    slide = np.ascontiguousarray(np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:S, :S])
    img = os.path.join(tmp, 'slide%d.tif' % k)
    Image.fromarray(slide).save(img)
    margin = S * 0.075
    pitch = (S - 2 * margin) / IP.VISIUM_W_ST
    spatial = os.path.join(tmp, 'array%d' % k, 'outs', 'spatial')
    os.makedirs(spatial)
    annot = os.path.join(tmp, 'annot%d.csv' % k)
    with open(os.path.join(spatial, 'tissue_positions.csv'), 'w') as fh, open(annot, 'w') as fa:
        fh.write('barcode,in_tissue,array_row,array_col,pxl_row_in_fullres,pxl_col_in_fullres\n')
        fa.write('Barcode,region\n')
        for r in range(IP.VISIUM_H_ST):
            for c in range(IP.VISIUM_W_ST):
                fh.write('BC_%d_%d-1,1,%d,%d,%d,%d\n' % (r, c, r, 2 * c + r % 2, int(margin + pitch * 0.866 * r),
                                                        int(margin + pitch * (c + 0.5 * (r % 2)))))
                if (r + c) % 5:
                    fa.write('BC_%d_%d-1,%s\n' % (r, c, CLASSES[int(rng.integers(0, len(CLASSES)))]))
    return img, os.path.join(tmp, 'array%d' % k), annot


def _epochs(dataset, n_train, epochs, cached, patch):
    """Wall seconds per epoch of train_gridwise over `dataset` (the first n_train arrays train, the rest validate)."""
    torch.manual_seed(0)
    f = ga.DenseNet(num_classes=len(CLASSES), growth_rate=8, block_config=(2, 2), num_init_features=16, bn_size=2,
                    small_inputs=patch <= 32)
    for p in f.parameters():
        p.requires_grad = False
    m = ga.GridNetHexOddr(f, (3, patch, patch), (IP.VISIUM_H_ST, IP.VISIUM_W_ST), len(CLASSES))
    if cached:
        m.enable_f_cache()
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
    ap.add_argument('--slides', type=int, default=3)
    ap.add_argument('--slide', type=int, default=6000)
    ap.add_argument('--patch', type=int, default=32)
    ap.add_argument('--window', type=int, default=48)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--remove-cast', action='store_true')
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        imgs, srds, annots = zip(*[_array(tmp, k, args.slide, rng) for k in range(args.slides)])
        kw = dict(patch_size=args.patch, window_size=args.window, remove_cast=args.remove_cast)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            IP.save_visium_patches_all(imgs, srds, os.path.join(tmp, 'patches'), device=DEV, **kw)
        n_files = sum(len(os.listdir(os.path.join(tmp, 'patches', 'slide%d' % k))) for k in range(args.slides))
        print("%d slides of %d x %d: save_visium_patches_all wrote %d JPEGs of %d px in %.2f s (once)" %
              (args.slides, args.slide, args.slide, n_files, args.patch, time.perf_counter() - t0), flush=True)
        files = ga.PatchGridDataset([os.path.join(tmp, 'patches', 'slide%d' % k) for k in range(args.slides)], list(annots),
                                    [IP.visium_find_position_file(d) for d in srds], raw_uint8=True)
        slides = ga.SlideGridDataset(list(imgs), list(srds), list(annots), device=DEV, **kw)
        t0 = time.perf_counter()
        for k in range(args.slides):
            assert torch.equal(slides[k][1], files[k][1]), "the label grids of array %d differ" % k
        print("label grids equal; first pass over both datasets (slides decoded and uploaded, %s resident): %.2f s" %
              (slides.resident(), time.perf_counter() - t0), flush=True)
        n_train = max(1, args.slides - 1)
        feeds = (('files ', files), ('slides', slides))
        times = {(name, cached): [] for name, _ in feeds for cached in (False, True)}
        for r in range(args.rounds):
            for cached in (False, True):
                for name, ds in feeds:
                    t = _epochs(ds, n_train, args.epochs, cached, args.patch)
                    times[(name, cached)].append(t)
                    print("round %d  %s  f cache %-3s  %.3f s per epoch" % (r, name, 'on' if cached else 'off', t), flush=True)
        for (name, cached), v in times.items():
            print("%s f cache %-3s: %d arrays, %d epochs: median %.3f s per epoch, min %.3f, max %.3f" %
                  (name, 'on' if cached else 'off', args.slides, args.epochs, float(np.median(v)), min(v), max(v)))


if __name__ == '__main__':
    main()
