"""Config 4 (frozen DenseNet-121 image f + count MLP f + hex g on 78 x 64 arrays of 128-px patches) through `train_gridwise`
for several epochs over the SAME arrays, with and without the frozen-classifier row cache (GridNet.enable_f_cache): wall
time per epoch, epoch 0 (every array a miss) apart from the later ones (every array a hit).  Public API only.

    python tools/diag/c4_cached_epochs.py --cache off
    python tools/diag/c4_cached_epochs.py --cache on [--u8] [--arrays 10] [--epochs 5]
    python tools/diag/c4_cached_epochs.py --fingerprint        # the fingerprint kernel alone: GB/s on one array

`--cache off` never touches the cache's API, so the same file times a checkout that predates it.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga   # noqa: E402
from gridnext_amd.synthetic import count_mlp, visium_array   # noqa: E402

DEV = torch.device('cuda:0')
H, W, GENES, CLASSES = 78, 64, 2000, 8
DENSENET121 = dict(growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4, drop_rate=0,
                   small_inputs=False)


class Timed:
    """A loader that notes when each pass over it starts (device drained).  The loop's prefetcher pulls batches one ahead
    from its own thread, so only the START of a pass is a point of the loop's own timeline: an epoch is measured from the
    start of its train pass to the start of the next epoch's, and one extra epoch is run to close the last interval."""

    def __init__(self, batches):
        self.dataset = batches
        self.starts = []

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        torch.cuda.synchronize()
        self.starts.append(time.perf_counter())
        for b in self.dataset:
            yield b


def arrays(n, patch, u8):
    out = []
    for a in range(n):
        x_img, x_cnt, y = visium_array(a, GENES, CLASSES, patch, device=DEV)
        if u8:
            x_img = (x_img * 255.0).round().to(torch.uint8)
        out.append(([x_img.unsqueeze(0), x_cnt.unsqueeze(0)], y.unsqueeze(0)))
    return out


def epochs(args):
    torch.manual_seed(0)
    model = ga.GridNetHexMM(ga.DenseNet(num_classes=CLASSES, **DENSENET121), count_mlp(GENES, CLASSES), (3, args.patch, args.patch),
                            (GENES,), (H, W), CLASSES).to(DEV)
    for p in model.patch_classifier.parameters():                   # Tutorial_multimodal.ipynb cell 27
        p.requires_grad = False
    if args.cache == 'on':
        model.enable_f_cache()
    data = arrays(args.arrays, args.patch, args.u8)
    n_val = max(1, args.arrays // 5)
    loaders = {'train': Timed(data[n_val:]), 'val': Timed(data[:n_val])}
    opt = torch.optim.Adam(model.corrector.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        model, vh, th = ga.train_gridwise(model, loaders, nn.CrossEntropyLoss(), opt, num_epochs=args.epochs + 1)
    starts = loaders['train'].starts
    per_epoch = [b - a for a, b in zip(starts[:-1], starts[1:])]
    out = {"cache": args.cache, "arrays": args.arrays, "patch": args.patch, "input": "uint8" if args.u8 else "float32",
           "epoch_s": [round(t, 4) for t in per_epoch],
           "ms_per_array": [round(1e3 * t / args.arrays, 3) for t in per_epoch],
           "train_loss": th[:args.epochs], "val_loss": vh[:args.epochs]}
    if args.cache == 'on':
        c = model.image_f_cache
        out["image_cache"] = {"hits": c.hits, "misses": c.misses, "bypassed": c.bypassed, "bytes": c.bytes}
        c = model.count_f_cache
        out["count_cache"] = {"hits": c.hits, "misses": c.misses, "bypassed": c.bypassed, "bytes": c.bytes}
    print(json.dumps(out))


def fingerprint(args):
    """The kernel alone, timed with events over `reps` launches on arrays that do not fit the caches together."""
    from gridnext_amd import _lib as L
    res = {}
    for name, dtype in (("uint8", torch.uint8), ("float32", torch.float32)):
        n = H * W * 3 * args.patch * args.patch
        bufs = [torch.randint(0, 255, (n,), device=DEV, dtype=torch.uint8).to(dtype) for _ in range(4)]
        nbytes = n * bufs[0].element_size()
        out = torch.empty((1, 2), device=DEV, dtype=torch.int64)
        ws = torch.empty(max(1, L.query('gnx_fingerprint128_batch_workspace', nbytes, 1) // 8), device=DEV, dtype=torch.int64)

        def launch(b):
            L.call('gnx_fingerprint128_batch', b.data_ptr(), nbytes, 1, out.data_ptr(), ws.data_ptr(), L.stream())
        for b in bufs:
            launch(b)
        torch.cuda.synchronize()
        reps, times = 500, []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(reps):
                launch(bufs[r % len(bufs)])
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps)
        res[name] = {"bytes": nbytes, "ms": [round(t, 4) for t in times],
                     "GB_per_s": [round(nbytes / t / 1e6, 1) for t in times]}
    print(json.dumps({"fingerprint_kernel": res}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--cache', choices=('on', 'off'), default='on')
    ap.add_argument('--arrays', type=int, default=10)
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--patch', type=int, default=128)
    ap.add_argument('--u8', action='store_true')
    ap.add_argument('--fingerprint', action='store_true')
    a = ap.parse_args()
    fingerprint(a) if a.fingerprint else epochs(a)
