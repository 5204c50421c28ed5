#!/usr/bin/env python3
"""What one Visium array's patch grid costs from the decoded slide, on the host and on the device (public API only).

    python tools/diag/host_vs_device_wsi.py [--slide 20000] [--patch 256] [--window 256] [--rounds 3]

A synthetic decoded slide (uint8, `--slide` pixels square) and a Spaceranger-style tissue_positions.csv of 78 x 64 = 4 992
in-tissue spots on Visium spacing, written to a temporary directory.  Per round, alternating, wall time from the decoded slide
to the uint8 grid resident on the device:
  (a) host:   `grid_from_wsi_visium(slide, dir, device=None)` (the reference's algorithm: one window and one Pillow resize
              per spot, float32 grid), converted to uint8 and copied to the device - what a user had to do before;
  (b) device: `grid_from_wsi_visium(resident_slide, dir, device=..., raw_uint8=True)` (gnx_wsi_patch_grid_u8).
The one-off upload of the slide is timed on its own.  Ends by asserting that both grids are equal.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gridnext_amd import imgprocess as IP                  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slide', type=int, default=20000)
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--window', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    S = args.slide
    rng = np.random.default_rng(0)
    slide = rng.integers(1, 256, (S, S, 3), dtype=np.uint8)
    margin = S * 0.075
    pitch = (S - 2 * margin) / IP.VISIUM_W_ST
    with tempfile.TemporaryDirectory() as tmp:
        spatial = os.path.join(tmp, 'array0', 'outs', 'spatial')
        os.makedirs(spatial)
        with open(os.path.join(spatial, 'tissue_positions.csv'), 'w') as fh:
            fh.write('barcode,in_tissue,array_row,array_col,pxl_row_in_fullres,pxl_col_in_fullres\n')
            for r in range(IP.VISIUM_H_ST):
                for c in range(IP.VISIUM_W_ST):
                    fh.write('BC_%d_%d-1,1,%d,%d,%d,%d\n' % (r, c, r, 2 * c + r % 2, int(margin + pitch * 0.866 * r),
                                                            int(margin + pitch * (c + 0.5 * (r % 2)))))
        srd = os.path.join(tmp, 'array0')
        kw = dict(patch_size=args.patch, window_size=args.window)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        resident = torch.from_numpy(slide).to(DEV)
        torch.cuda.synchronize()
        print("slide %d x %d x 3 (%.2f GB): upload %.3f s (once per slide)" % (S, S, slide.nbytes / 1e9, time.perf_counter() - t0))
        IP.grid_from_wsi_visium(resident[:64, :64], _tiny_tree(tmp), device=DEV, raw_uint8=True, **kw)      # tables, module load

        def host():
            t0 = time.perf_counter()
            g = IP.grid_from_wsi_visium(slide, srd, **kw).to(torch.uint8).to(DEV)
            torch.cuda.synchronize()
            return g, time.perf_counter() - t0

        def device():
            t0 = time.perf_counter()
            g = IP.grid_from_wsi_visium(resident, srd, device=DEV, raw_uint8=True, **kw)
            torch.cuda.synchronize()
            return g, time.perf_counter() - t0

        totals = {'host': [], 'device': []}
        same = True
        for r in range(args.rounds):
            ga, ta = host()
            gb, tb = device()
            same = same and torch.equal(ga, gb)
            del ga, gb
            totals['host'].append(ta)
            totals['device'].append(tb)
            print("round %d  host %.3f s | device %.4f s" % (r, ta, tb), flush=True)
        for k, v in totals.items():
            print("%-6s per array of 4992 spots, window %d -> %d px: median %.4f s, min %.4f s, max %.4f s" %
                  (k, args.window, args.patch, float(np.median(v)), min(v), max(v)))
        print("ratio of medians host / device: %.1f" % (float(np.median(totals['host'])) / float(np.median(totals['device']))))
        assert same, "the host and the device grid differ"
        print("both grids are equal")


def _tiny_tree(tmp):
    spatial = os.path.join(tmp, 'warm', 'outs', 'spatial')
    os.makedirs(spatial)
    with open(os.path.join(spatial, 'tissue_positions.csv'), 'w') as fh:
        fh.write('barcode,in_tissue,array_row,array_col,pxl_row_in_fullres,pxl_col_in_fullres\nW-1,1,0,0,32,32\n')
    return os.path.join(tmp, 'warm')


if __name__ == '__main__':
    main()
