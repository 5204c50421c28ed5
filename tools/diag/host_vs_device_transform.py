#!/usr/bin/env python3
"""What the tutorials' transform costs per array on the host and on the device (public API only).

    python tools/diag/host_vs_device_transform.py [--spots 4992] [--stored 260] [--rounds 3]

One synthetic array of `--spots` decoded 260-px RGB patches (PIL images, as `Image.open` of a spot file gives them).  Per
round, alternating, wall time from the decoded images to transformed float patches resident on the device:
  (a) host:   Compose([Resize(256), CenterCrop(224), ToTensor(), Normalize]) per image (what `PatchGridDataset(img_transforms=...)`
              does), stacked, then the float32 host -> device copy;
  (b) device: `to_tensor_u8` per image (what `raw_uint8=True` does), stacked, the uint8 host -> device copy, then
              `transforms.resize_crop(..., out_float=True)` (gnx_resize_crop_u8_f32).
Both end in the same floats (checked on the first round).  Prints one line per round and the spread between rounds.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from PIL import Image                                      # noqa: E402
from gridnext_amd import transforms as T                   # noqa: E402
from gridnext_amd.image_datasets import to_tensor_u8       # noqa: E402

DEV = 'cuda:0'
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spots', type=int, default=4992)
    ap.add_argument('--stored', type=int, default=260)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    imgs = [Image.fromarray(rng.integers(0, 256, (args.stored, args.stored, 3), dtype=np.uint8)) for _ in range(args.spots)]
    comp = T.Compose([T.Resize(256), T.CenterCrop(224), T.ToTensor(), T.Normalize(MEAN, STD)])
    sd = torch.tensor(STD)
    nrm = torch.cat([torch.tensor(MEAN), sd, 1.0 / sd]).to(DEV)
    torch.cuda.synchronize()

    def host():
        t0 = time.perf_counter()
        x = torch.stack([comp(im) for im in imgs])
        t1 = time.perf_counter()
        y = x.to(DEV)
        torch.cuda.synchronize()
        return y, t1 - t0, time.perf_counter() - t1

    def device():
        t0 = time.perf_counter()
        x = torch.stack([to_tensor_u8(im) for im in imgs])
        t1 = time.perf_counter()
        xd = x.to(DEV)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        y = T.resize_crop(xd, 256, 224, nrm, True)
        torch.cuda.synchronize()
        return y, t1 - t0, t2 - t1, time.perf_counter() - t2

    T.resize_crop(torch.zeros((1, 3, args.stored, args.stored), device=DEV, dtype=torch.uint8), 256, 224, nrm, True)   # tables, module load
    totals = {'host': [], 'device': []}
    for r in range(args.rounds):
        ya, a_cpu, a_copy = host()
        yb, b_cpu, b_copy, b_kernel = device()
        if r == 0:
            print("same floats on both paths: %s" % torch.equal(ya, yb))
        del ya, yb
        totals['host'].append(a_cpu + a_copy)
        totals['device'].append(b_cpu + b_copy + b_kernel)
        print("round %d  host: transform %.3f s + float H2D %.3f s = %.3f s | device: decode-to-uint8 %.3f s + uint8 H2D %.3f s + "
              "kernel %.4f s = %.3f s" % (r, a_cpu, a_copy, a_cpu + a_copy, b_cpu, b_copy, b_kernel, b_cpu + b_copy + b_kernel),
              flush=True)
    for k, v in totals.items():
        print("%-6s per array of %d spots: median %.3f s, min %.3f s, max %.3f s" % (k, args.spots, float(np.median(v)), min(v), max(v)))
    print("ratio of medians host / device: %.1f" % (float(np.median(totals['host'])) / float(np.median(totals['device']))))


if __name__ == '__main__':
    main()
