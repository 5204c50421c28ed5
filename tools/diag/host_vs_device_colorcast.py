#!/usr/bin/env python3
"""What removing the colour cast of one decoded slide costs on the host and on the device (public API only).

    python tools/diag/host_vs_device_colorcast.py [--slide 10000] [--rounds 3]

A synthetic decoded slide (uint8, `--slide` pixels square; the default 10 000 x 10 000 = 0.3 GB keeps the host side bearable:
a quarter of the README's 20 000 x 20 000): a bright background on 60 % of the pixels, tinted noise elsewhere.  Per round,
alternating, wall time of
  (a) host:   `remove_color_cast(slide)` on the numpy array (bincount, percentile from the histogram, table, fancy index), and
              `remove_color_cast(Image)`: the reference's expression through Pillow (np.percentile + three point() + merge);
  (b) device: `remove_color_cast(resident_slide)` on the resident tensor (gnx_rgb_hist_u8, one 6 KB copy, gnx_rgb_lut_u8),
              out of place and in place.
Ends by asserting that all of them give the same bytes.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gridnext_amd import imgprocess as IP                  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slide', type=int, default=10000)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    S = args.slide
    rng = np.random.default_rng(0)
    slide = np.empty((S, S, 3), dtype=np.uint8)
    for c, top in enumerate((231, 197, 246)):
        slide[:, :, c] = rng.integers(1, top, (S, S), dtype=np.uint8)
    slide[rng.random((S, S)) < 0.6] = (228, 190, 241)
    pil = Image.fromarray(slide)
    resident = torch.from_numpy(slide).to(DEV)
    torch.cuda.synchronize()
    print("slide %d x %d x 3 (%.2f GB)" % (S, S, slide.nbytes / 1e9))
    IP.remove_color_cast(resident[:64].contiguous())        # module load

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    totals = {'host numpy': [], 'host Pillow': [], 'device': [], 'device in place': []}
    same = True
    for r in range(args.rounds):
        a, ta = timed(lambda: IP.remove_color_cast(slide))
        p, tp = timed(lambda: IP.remove_color_cast(pil))
        d, td = timed(lambda: IP.remove_color_cast(resident))
        work = resident.clone()
        _, ti = timed(lambda: IP.remove_color_cast(work, inplace=True))
        same = same and np.array_equal(a, np.array(p)) and torch.equal(d.cpu(), torch.from_numpy(a)) and torch.equal(d, work)
        del a, p, d, work
        for k, t in zip(totals, (ta, tp, td, ti)):
            totals[k].append(t)
        print("round %d  host numpy %.3f s | host Pillow %.3f s | device %.4f s | device in place %.4f s" % (r, ta, tp, td, ti),
              flush=True)
    for k, v in totals.items():
        print("%-16s median %.4f s, min %.4f s, max %.4f s" % (k, float(np.median(v)), min(v), max(v)))
    print("ratio of medians host Pillow / device: %.0f" %
          (float(np.median(totals['host Pillow'])) / float(np.median(totals['device']))))
    assert same, "the host and the device result differ"
    print("all results are equal")


if __name__ == '__main__':
    main()
