"""The Cartesian corrector timed on the device, HIP route beside the torch route it replaces (HIP events, one 78 x 64 array,
C = 8, a frozen count MLP of 2000 genes):
  * the four default layers (8 -> 8: 3x3, 5x5, 5x5, 3x3): forward, data gradient, weight gradient per call, gnx_gridconv_*
    against torch's convolution (aten.convolution_backward with one output at a time);
  * the first train step of each route (wall clock, after f alone has run once: library loading and torch's algorithm
    search are what a user waits for once);
  * the steady train step (forward, loss, backward, Adam, zero_grad): the torch route run eagerly - `model.corrector` on NCHW
    and train_gridwise's unfused loss, what GridNet did before it had a channels-last forward -, the HIP route run eagerly,
    and the HIP route captured and replayed (graphs.py).  The three alternate, round after round, in one process; the
    spread over the rounds is reported with the medians.
    python tools/diag/gridconv_time.py [--reps N] [--rounds R] [--out FILE.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gridnext_amd as ga   # noqa: E402
from gridnext_amd import _lib as L, graphs, training as gtrain   # noqa: E402
from gridnext_amd.synthetic import count_mlp, visium_array   # noqa: E402

DEV = torch.device('cuda:0')
H, W, C, G = 78, 64, 8, 2000


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


def layer_ops(I, O, k):
    """{route: (forward, data gradient, weight gradient)} callables of one k x k layer on one array."""
    g = torch.Generator(device=DEV).manual_seed(I * 100 + O + k)
    x = torch.randn(1, H, W, I, device=DEV, generator=g)
    dy = torch.randn(1, H, W, O, device=DEV, generator=g)
    m = nn.Conv2d(I, O, k, padding=k // 2).to(DEV)
    w, b = m.weight.detach(), m.bias.detach()
    y, dx, dw, db = torch.empty(1, H, W, O, device=DEV), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    ws = torch.empty(L.query('gnx_gridconv_bwd_weight_workspace', 1, H, W, I, O, k, k), device=DEV)
    st = L.stream()
    hip = (lambda: L.call('gnx_gridconv_fwd', L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), 1, H, W, I, O, k, k, st),
           lambda: L.call('gnx_gridconv_bwd_data', L.ptr(dy), L.ptr(w), L.ptr(dx), 1, H, W, I, O, k, k, st),
           lambda: L.call('gnx_gridconv_bwd_weight', L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), L.ptr(ws), 1, H, W, I, O, k, k, 0,
                          st))
    xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)      # what the torch route's layers see: NCHW views of the rows
    p = [k // 2, k // 2]

    def bwd(mask):
        return torch.ops.aten.convolution_backward(dyn, xn, w, [O], [1, 1], p, [1, 1], False, [0, 0], 1, mask)
    stock = (lambda: torch.nn.functional.conv2d(xn, w, b, padding=k // 2),
             lambda: bwd([True, False, False]), lambda: bwd([False, True, True]))
    return {'hip': hip, 'torch': stock}


class TorchRoute(nn.Module):
    """GridNet as it ran before it had a channels-last forward: f on the HIP kernels, the corrector's stock layers called on
    the NCHW view; having no `forward_nhwc`, train_gridwise's `_grid_loss` takes its unfused loss for it."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        return self.net.corrector(self.net.patch_predictions(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    layers = []
    print("%-12s %-6s %9s %9s %9s   (us per call, one %d x %d array)" % ('layer', 'route', 'fwd', 'dgrad', 'wgrad', H, W))
    for idx, k in enumerate((3, 5, 5, 3)):
        ops = layer_ops(C, C, k)
        for fn3 in ops.values():                                  # every shape warmed on both routes before any is timed
            for fn in fn3:
                fn()
        torch.cuda.synchronize()
        row = dict(layer=idx, I=C, O=C, k=k)
        for route, fn3 in ops.items():
            fw, dg, wg = (timeit(fn, args.reps) for fn in fn3)
            row.update({route + '_fwd_us': fw, route + '_dgrad_us': dg, route + '_wgrad_us': wg})
            print("%d: %d->%d %dx%d %-6s %9.1f %9.1f %9.1f" % (idx, C, C, k, k, route, fw, dg, wg))
        layers.append(row)

    torch.manual_seed(0)
    base = ga.GridNet(count_mlp(G, C), (G,), (H, W), C)
    for p in base.patch_classifier.parameters():
        p.requires_grad = False
    crit = nn.CrossEntropyLoss()
    _, xc, y = visium_array(3, G, C, image=False, device=DEV)
    x, y = xc.permute(1, 2, 0).contiguous().unsqueeze(0), y.unsqueeze(0)

    def make(route):
        net = copy.deepcopy(base).to(DEV)
        net.train()
        net.patch_classifier.eval()
        model = TorchRoute(net) if route == 'torch' else net
        opt = torch.optim.Adam(net.corrector.parameters(), lr=1e-3)
        return net, model, opt

    def eager_step(model, opt):
        loss = gtrain._grid_loss(model, x, y, crit, 1, True)[0]
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    nets = {r: make(r) for r in ('torch', 'hip', 'hip_replayed')}
    with torch.no_grad():
        nets['hip'][0].patch_predictions(x)                       # f alone, once: its code objects are loaded for both routes
    torch.cuda.synchronize()
    first = {}
    for r in ('hip', 'torch'):
        t0 = time.perf_counter()
        eager_step(nets[r][1], nets[r][2])
        torch.cuda.synchronize()
        first[r] = 1e3 * (time.perf_counter() - t0)
    print("first train step (wall, ms): HIP route %.1f, torch route %.1f" % (first['hip'], first['torch']))

    net, _, opt = nets['hip_replayed']
    stepper = graphs.GridStepGraphs(lambda i, lab: gtrain._grid_loss(net, i, lab, crit, 1, True), net.parameters(), models=(net,))

    def replayed_step():
        if stepper.run(True, x, y) is None:
            gtrain._grid_loss(net, x, y, crit, 1, True)[0].backward()
        opt.step()
        opt.zero_grad()
    for _ in range(graphs.WARMUP + 2):
        replayed_step()
    assert stepper.run(True, x, y) is not None, "the step was not captured"
    opt.zero_grad()
    steps = {'torch_eager': lambda: eager_step(nets['torch'][1], nets['torch'][2]),
             'hip_eager': lambda: eager_step(nets['hip'][1], nets['hip'][2]),
             'hip_replayed': replayed_step}
    for fn in steps.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    series = {n: [] for n in steps}
    for _ in range(args.rounds):                                  # alternating: every round times each route once
        for n, fn in steps.items():
            series[n].append(timeit(fn, args.reps))
    summary = {n: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), rounds_us=v) for n, v in series.items()}
    print("train step of one array (forward, loss, backward, Adam, zero_grad), us per step over %d rounds of %d steps:"
          % (args.rounds, args.reps))
    for n, s in summary.items():
        print("  %-13s median %9.1f   min %9.1f   max %9.1f" % (n, s['median_us'], s['min_us'], s['max_us']))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'array': [H, W], 'n_classes': C, 'genes': G, 'reps': args.reps, 'rounds': args.rounds, 'layers': layers,
                       'first_step_wall_ms': first, 'train_step_us': summary}, f, indent=1)


if __name__ == '__main__':
    main()
