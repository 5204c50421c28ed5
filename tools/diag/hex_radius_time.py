"""Radius-k hex conv layers timed on the device (HIP events, as tools/kbench.py:timeit), one 78 x 64 array (B = 1):
forward, data gradient and weight gradient (slab kernel + reduce) of 14 -> 32, 32 -> 32 and 32 -> 7 layers at k = 1 (the
size-1 entry points), 2 and 3 in both addressings; then one captured config-3 step (count f frozen, train_gridwise's graph
replay) with the default corrector and with a corrector whose first layer of each pair has radius 2.
    python tools/diag/hex_radius_time.py [--reps N] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga   # noqa: E402
import gridnext_amd.hexconv as hexagdly   # noqa: E402
from gridnext_amd import _lib as L, graphs, training as gtrain   # noqa: E402
from gridnext_amd.synthetic import count_mlp, visium_array   # noqa: E402

DEV = torch.device('cuda:0')
H, W = 78, 64


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / reps          # us


def layer_ops(I, O, k, mode):
    """(forward, data gradient, weight gradient) callables of one layer on one array."""
    g = torch.Generator(device=DEV).manual_seed(I * 100 + O + k)
    x = torch.randn(1, H, W, I, device=DEV, generator=g)
    dy = torch.randn(1, H, W, O, device=DEV, generator=g)
    m = hexagdly.Conv2d(I, O, kernel_size=k).to(DEV)
    ks = [p.detach() for p in m.kernels()]
    b = m.bias_tensor.detach()
    y, dx = torch.empty(1, H, W, O, device=DEV), torch.empty(1, H, W, I, device=DEV)
    dks, db = [torch.empty_like(t) for t in ks], torch.empty_like(b)
    st = L.stream()
    if k == 1:
        ws = torch.empty(L.query('gnx_hexconv_bwd_weight_workspace', 1, H, W, I, O), device=DEV)
        return (lambda: L.call('gnx_hexconv_fwd', L.ptr(x), L.ptr(ks[0]), L.ptr(ks[1]), L.ptr(b), L.ptr(y), 1, H, W, I, O, mode, st),
                lambda: L.call('gnx_hexconv_bwd_data', L.ptr(dy), L.ptr(ks[0]), L.ptr(ks[1]), L.ptr(dx), 1, H, W, I, O, mode, st),
                lambda: L.call('gnx_hexconv_bwd_weight', L.ptr(x), L.ptr(dy), L.ptr(dks[0]), L.ptr(dks[1]), L.ptr(db), L.ptr(ws),
                               1, H, W, I, O, mode, 0, st))
    kp = (ctypes.c_void_p * (k + 1))(*[t.data_ptr() for t in ks])
    dp = (ctypes.c_void_p * (k + 1))(*[t.data_ptr() for t in dks])
    ws = torch.empty(L.query('gnx_hexconv_k_bwd_weight_workspace', 1, H, W, I, O, k), device=DEV)
    return (lambda: L.call('gnx_hexconv_k_fwd', L.ptr(x), ctypes.addressof(kp), L.ptr(b), L.ptr(y), 1, H, W, I, O, k, mode, st),
            lambda: L.call('gnx_hexconv_k_bwd_data', L.ptr(dy), ctypes.addressof(kp), L.ptr(dx), 1, H, W, I, O, k, mode, st),
            lambda: L.call('gnx_hexconv_k_bwd_weight', L.ptr(x), L.ptr(dy), ctypes.addressof(dp), L.ptr(db), L.ptr(ws), 1, H, W, I,
                           O, k, mode, 0, st))


class Radius2Oddr(ga.GridNetHexOddr):
    """The default corrector with the first layer of each pair at radius 2."""

    def _init_corrector(self):
        def conv(i, o, k):
            return hexagdly.Conv2d(i, o, kernel_size=k, stride=1, bias=True)
        return nn.Sequential(conv(self.f_dim, 32, 2), conv(32, 32, 1), nn.BatchNorm2d(32), nn.ReLU(),
                             conv(32, 32, 2), conv(32, 32, 1), nn.BatchNorm2d(32), nn.ReLU(), conv(32, self.n_classes, 1))


def captured_step_us(cls, reps):
    """Device time of one replayed config-3 train step (f forward, g forward, masked CE, g backward) of one array."""
    torch.manual_seed(0)
    m = cls(count_mlp(2000, 8), (2000,), (H, W), 8).to(DEV)
    for p in m.patch_classifier.parameters():
        p.requires_grad = False
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    crit = nn.CrossEntropyLoss()
    _, xc, y = visium_array(3, image=False, device=DEV)
    x, y = xc.unsqueeze(0), y.unsqueeze(0)
    m.train()
    m.patch_classifier.eval()
    stepper = graphs.GridStepGraphs(lambda i, lab: gtrain._grid_loss(m, i, lab, crit, 1, True), m.parameters(), models=(m,))
    for _ in range(graphs.WARMUP + 2):
        if stepper.run(True, x, y) is None:
            gtrain._grid_loss(m, x, y, crit, 1, True)[0].backward()
        opt.step()
        opt.zero_grad()
    assert stepper.run(True, x, y) is not None, "the step was not captured"
    opt.zero_grad()
    return timeit(lambda: (stepper.run(True, x, y), opt.zero_grad()), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    rows = []
    print("%-10s %2s %4s %9s %9s %9s   (us per call, one 78 x 64 array)" % ('layer', 'k', 'mode', 'fwd', 'dgrad', 'wgrad'))
    for I, O in ((14, 32), (32, 32), (32, 7)):
        for k in (1, 2, 3):
            for mode in (0, 1):
                fw, dg, wg = (timeit(f, args.reps) for f in layer_ops(I, O, k, mode))
                rows.append(dict(I=I, O=O, k=k, mode=mode, fwd_us=fw, dgrad_us=dg, wgrad_us=wg))
                print("%3d -> %-3d %2d %4d %9.1f %9.1f %9.1f" % (I, O, k, mode, fw, dg, wg))
    for r in rows:
        base = next(b for b in rows if (b['I'], b['O'], b['mode'], b['k']) == (r['I'], r['O'], r['mode'], 1))
        r['fwd_over_k1'], r['dgrad_over_k1'] = r['fwd_us'] / base['fwd_us'], r['dgrad_us'] / base['dgrad_us']
        r['taps_over_7'] = (1 + 3 * r['k'] * (r['k'] + 1)) / 7.0
    steps = {'default': captured_step_us(ga.GridNetHexOddr, args.reps), 'radius2': captured_step_us(Radius2Oddr, args.reps)}
    print("captured config-3 train step (replay + zero_grad, device time): default corrector %.1f us, radius-2 corrector %.1f us"
          % (steps['default'], steps['radius2']))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'layers': rows, 'captured_step_us': steps}, f, indent=1)


if __name__ == '__main__':
    main()
