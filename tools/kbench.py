#!/usr/bin/env python3
"""Kernel micro-benchmark harness for the DenseNet conv kernels (tuning aid; runs on the GPU box).

    python tools/kbench.py [--spots 4992] [--reps 5] [--only conv3x3|conv1x1|stem|pool|dgrad0|resize|wsi|colorcast|augment|augment_hs|metrics|counts|sparse_linear|gram|exprmetrics|hvg|spatial]
    python tools/kbench.py --only winowide --reps 200 --rounds 3 --libs narrow=PATH,...   (8-wave Winograd conv2 beside other builds)
Prints per-shape time and achieved TFLOP/s (algorithmic FLOPs) using HIP events on the launch stream.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gridnext_amd import _lib as L   # noqa: E402

DEV = 'cuda:0'


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spots', type=int, default=4992)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', default='')
    ap.add_argument('--noact', action='store_true', help='conv3x3 without the BN+ReLU prologue')
    ap.add_argument('--const', action='store_true', help='constant operands (low bit toggling) instead of randn')
    ap.add_argument('--wino', action='store_true', help='conv3x3 in its Winograd F(2,3) form (prologue-free operand)')
    ap.add_argument('--dense', action='store_true', help='operand rows exactly K wide (lda = K) instead of the block buffer stride')
    ap.add_argument('--libs', default='', help='--only winowide: comparison builds to time beside the loaded library, label=path,...')
    ap.add_argument('--rounds', type=int, default=1, help='--only winowide / counts / sparse_linear / gram / exprmetrics / hvg / spatial: repetitions of the whole table')
    args = ap.parse_args()
    n = args.spots
    st = L.stream()
    torch.manual_seed(0)
    shapes = [(32, 64, 256), (32, 224, 256), (16, 128, 512), (16, 480, 512), (8, 256, 1024), (8, 992, 1024),
              (4, 512, 1024), (4, 992, 1024)]
    if args.dense:
        shapes = [(S, K, K) for S, K, _ in shapes]
    if args.only in ('', 'conv1x1'):
        for S, K, ct in shapes:
            M = n * S * S
            A = torch.randn(M, ct, device=DEV)
            W = torch.randn(128, K, device=DEV) * 0.05
            if args.const:
                A.fill_(1.0)
                W.fill_(0.05)
            out = torch.empty(M, 128, device=DEV)
            sc, sh = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1
            scp, shp = (None, None) if args.noact else (L.ptr(sc), L.ptr(sh))
            ms = timeit(lambda: L.call('gnx_conv1x1_bnrelu', L.ptr(A), ct, L.ptr(W), L.ptr(out), 128, M, 128, K,
                                       scp, shp, 0, 0, st), args.reps)
            fl = 2.0 * M * K * 128
            byts = 4.0 * M * (K + 128)
            print("conv1x1 S=%2d K=%4d M=%8d  %8.3f ms  %6.1f TFLOP/s  %5.2f TB/s" % (S, K, M, ms, fl / ms / 1e9, byts / ms / 1e9))
            del A, out
    if args.only == 'conv1x1split':
        # conv1 + norm2 / relu2 on the store: the fp32 instruction (gnx_conv1x1_bnrelu_act) beside the split-bf16 form
        for S, K, ct in shapes:
            M = n * S * S
            A = torch.randn(M, ct, device=DEV)
            W = torch.randn(128, K, device=DEV) * 0.05
            out = torch.empty(M, 128, device=DEV)
            sc, sh = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1
            osc, osh = torch.rand(128, device=DEV) + 0.5, torch.randn(128, device=DEV) * 0.1
            Wp = torch.empty(L.query('gnx_conv1x1_split_pack_halves', K), device=DEV, dtype=torch.bfloat16)
            L.call('gnx_conv1x1_split_pack', L.ptr(W), Wp.data_ptr(), K, st)
            ms0 = timeit(lambda: L.call('gnx_conv1x1_bnrelu_act', L.ptr(A), ct, L.ptr(W), L.ptr(out), 128, M, 128, K, L.ptr(sc),
                                        L.ptr(sh), L.ptr(osc), L.ptr(osh), st), args.reps)
            ms1 = timeit(lambda: L.call('gnx_conv1x1_bnrelu_act_split', L.ptr(A), ct, Wp.data_ptr(), L.ptr(out), 128, M, K, L.ptr(sc),
                                        L.ptr(sh), L.ptr(osc), L.ptr(osh), st), args.reps)
            fl = 2.0 * M * K * 128
            byts = 4.0 * M * (K + 128)
            print("conv1x1 S=%2d K=%4d M=%8d  fp32 mfma %8.3f ms %6.1f TFLOP/s %5.2f TB/s | split bf16 %8.3f ms %6.1f TFLOP/s %5.2f TB/s  (x%.2f)" %
                  (S, K, M, ms0, fl / ms0 / 1e9, byts / ms0 / 1e9, ms1, fl / ms1 / 1e9, byts / ms1 / 1e9, ms0 / ms1), flush=True)
            del A, out
    if args.only == 'wgrad1split':
        # conv1's weight gradient: the fp32-instruction kernel (gnx_wgrad_bnrelu) beside the split-bf16 form
        for S, K, ct in shapes:
            M = n * S * S
            X = torch.randn(M, ct, device=DEV)
            dY = torch.randn(M, 128, device=DEV)
            sc, sh = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1
            dW = torch.empty(128, K, device=DEV)
            ws0 = torch.empty(L.query('gnx_wgrad_workspace', M, 128, K, 1), device=DEV)
            ws1 = torch.empty(L.query('gnx_wgrad1x1_split_workspace', M, 128, K), device=DEV)
            ms0 = timeit(lambda: L.call('gnx_wgrad_bnrelu', L.ptr(dY), 128, L.ptr(X), ct, L.ptr(sc), L.ptr(sh), L.ptr(dW), L.ptr(ws0), M, 128,
                                        K, S, 1, 0, 0, st), args.reps)
            ms1 = timeit(lambda: L.call('gnx_wgrad1x1_split', L.ptr(dY), 128, L.ptr(X), ct, L.ptr(sc), L.ptr(sh), L.ptr(dW), L.ptr(ws1), M,
                                        128, K, 0, st), args.reps)
            fl = 2.0 * M * K * 128
            byts = 4.0 * M * (K + 128)
            print("wgrad1x1 S=%2d K=%4d M=%8d  fp32 mfma %8.3f ms %6.1f TFLOP/s %5.2f TB/s | split bf16 %8.3f ms %6.1f TFLOP/s %5.2f TB/s  (x%.2f)" %
                  (S, K, M, ms0, fl / ms0 / 1e9, byts / ms0 / 1e9, ms1, fl / ms1 / 1e9, byts / ms1 / 1e9, ms0 / ms1), flush=True)
            del X, dY
    if args.only == 'wgrad9split':
        # conv2's weight gradient: the fp32-instruction kernel (gnx_wgrad_bnrelu, taps = 9) beside the split-bf16 form
        for S in (32, 16, 8, 4):
            M = n * S * S
            A = torch.relu(torch.randn(M, 128, device=DEV))
            dY = torch.randn(M, 256, device=DEV)
            dW = torch.empty(32, 128, 3, 3, device=DEV)
            ws0 = torch.empty(L.query('gnx_wgrad_workspace', M, 32, 128, 9), device=DEV)
            ws1 = torch.empty(L.query('gnx_wgrad3x3_split_workspace', M), device=DEV)
            ms0 = timeit(lambda: L.call('gnx_wgrad_bnrelu', dY.data_ptr() + 4 * 64, 256, L.ptr(A), 128, None, None, L.ptr(dW), L.ptr(ws0), M, 32,
                                        128, S, 9, 0, 0, st), args.reps)
            ms1 = timeit(lambda: L.call('gnx_wgrad3x3_split', dY.data_ptr() + 4 * 64, 256, L.ptr(A), 128, L.ptr(dW), L.ptr(ws1), M, S, 0, st),
                         args.reps)
            fl = 2.0 * M * 1152 * 32
            byts = 4.0 * M * (128 + 32)
            print("wgrad3x3 S=%2d M=%8d  fp32 mfma %8.3f ms %6.1f TFLOP/s %5.2f TB/s | split bf16 %8.3f ms %6.1f TFLOP/s %5.2f TB/s  (x%.2f)" %
                  (S, M, ms0, fl / ms0 / 1e9, byts / ms0 / 1e9, ms1, fl / ms1 / 1e9, byts / ms1 / 1e9, ms0 / ms1), flush=True)
            del A, dY
    if args.only == 'conv3x3split':
        # conv2 on the ready (activated) bottleneck: Winograd F(2,3) on the fp32 instruction beside the split-bf16 direct form
        for S in (32, 16, 8, 4):
            M = n * S * S
            A = torch.relu(torch.randn(M, 128, device=DEV))
            ct = 256
            out = torch.empty(M, ct, device=DEV)
            Wt = torch.randn(32, 128, 3, 3, device=DEV) * 0.05
            Wu = torch.empty(12, 32, 128, device=DEV)
            L.call('gnx_winograd_conv3x3_weights', L.ptr(Wt), L.ptr(Wu), 32, 128, st)
            Wr = torch.randn(9, 32, 128, device=DEV) * 0.05
            Wp = torch.empty(L.query('gnx_conv3x3_split_pack_halves'), device=DEV, dtype=torch.bfloat16)
            L.call('gnx_conv3x3_split_pack', L.ptr(Wt), Wp.data_ptr(), st)
            if S >= 8:
                ms0 = timeit(lambda: L.call('gnx_conv3x3_winograd', L.ptr(A), 128, L.ptr(Wu), out.data_ptr() + 4 * 64, ct, M, 32, 128, S,
                                            st), args.reps)
            else:
                ms0 = timeit(lambda: L.call('gnx_conv3x3_bnrelu', L.ptr(A), 128, L.ptr(Wr), out.data_ptr() + 4 * 64, ct, M, 32, 128, S,
                                            None, None, st), args.reps)
            ms1 = timeit(lambda: L.call('gnx_conv3x3_split', L.ptr(A), 128, Wp.data_ptr(), out.data_ptr() + 4 * 64, ct, M, S, st), args.reps)
            fl = 2.0 * M * 1152 * 32
            byts = 4.0 * M * (128 + 32)
            print("conv3x3 S=%2d M=%8d  fp32 mfma %8.3f ms %6.1f TFLOP/s (direct-conv FLOPs) %5.2f TB/s | split bf16 %8.3f ms %6.1f TFLOP/s %5.2f TB/s  (x%.2f)" %
                  (S, M, ms0, fl / ms0 / 1e9, byts / ms0 / 1e9, ms1, fl / ms1 / 1e9, byts / ms1 / 1e9, ms0 / ms1), flush=True)
            del A, out
    if args.only == 'winowide':
        # conv2's Winograd kernel at the headline's S = 32 and S = 16 launches (K = 128, block buffer stride 256): the loaded
        # library, whose gnx_conv3x3_winograd runs the 8-wave 512-pixel form at these row counts, beside comparison builds of
        # csrc/conv3x3.hip given as --libs label=path,...: -DGNX_WINO_NARROW=1 (never wide: the 256-pixel form), -DGNX_WINO_DBG=1
        # (no input transform: what is left is DMA waits, barriers and the multiplies) and both.  --rounds: the whole table that
        # many times, the libraries taking turns; --reps at least 200 (short runs sit in the clock ramp).
        import ctypes
        libs = [('this', L.lib())]
        for item in filter(None, args.libs.split(',')):
            label, path = item.split('=', 1)
            h = ctypes.CDLL(os.path.abspath(path))
            for name in ('gnx_conv3x3_winograd', 'gnx_conv3x3_winograd_form'):
                getattr(h, name).restype, getattr(h, name).argtypes = L.SIGNATURES[name]
            libs.append((label, h))
        reps = max(args.reps, 200)
        Wt = torch.randn(32, 128, 3, 3, device=DEV) * 0.05
        Wu = torch.empty(12, 32, 128, device=DEV)
        L.call('gnx_winograd_conv3x3_weights', L.ptr(Wt), L.ptr(Wu), 32, 128, st)
        for rnd in range(args.rounds):
            for S in (32, 16):
                for spots in (4456, 4992):
                    M = spots * S * S
                    A = torch.relu(torch.randn(M, 128, device=DEV))
                    out = torch.empty(M, 256, device=DEV)
                    a = (L.ptr(A), 128, L.ptr(Wu), out.data_ptr() + 4 * 64, 256, M, 32, 128, S)
                    for label, h in libs:
                        wgs = ctypes.c_int(0)
                        code = h.gnx_conv3x3_winograd_form(*a, ctypes.addressof(wgs))

                        def launch():
                            assert h.gnx_conv3x3_winograd(*a, st) == 0
                        ms = timeit(launch, reps)
                        print("winowide round %d S=%2d spots=%4d M=%8d  %-20s form %2d x %3d wgs  %8.4f ms  %6.1f TFLOP/s "
                              "(direct-conv FLOPs)" % (rnd, S, spots, M, label, code, wgs.value, ms, 2.0 * M * 1152 * 32 / ms / 1e9),
                              flush=True)
                    del A, out
    if args.only in ('', 'conv3x3'):
        for S in (32, 16, 8, 4):
            M = n * S * S
            A = torch.randn(M, 128, device=DEV)
            Wr = torch.randn(9, 32, 128, device=DEV) * 0.05
            ct = 256
            out = torch.empty(M, ct, device=DEV)
            sc, sh = torch.rand(128, device=DEV) + 0.5, torch.randn(128, device=DEV) * 0.1
            scp, shp = (None, None) if args.noact else (L.ptr(sc), L.ptr(sh))
            if args.wino:
                Wt = torch.randn(32, 128, 3, 3, device=DEV) * 0.05
                Wu = torch.empty(12, 32, 128, device=DEV)
                L.call('gnx_winograd_conv3x3_weights', L.ptr(Wt), L.ptr(Wu), 32, 128, st)
                ms = timeit(lambda: L.call('gnx_conv3x3_winograd', L.ptr(A), 128, L.ptr(Wu), out.data_ptr() + 4 * 64, ct,
                                           M, 32, 128, S, st), args.reps)
            else:
                ms = timeit(lambda: L.call('gnx_conv3x3_bnrelu', L.ptr(A), 128, L.ptr(Wr), out.data_ptr() + 4 * 64, ct,
                                           M, 32, 128, S, scp, shp, st), args.reps)
            fl = 2.0 * M * 1152 * 32
            print("conv3x3 S=%2d M=%8d  %8.3f ms  %6.1f TFLOP/s (direct-conv FLOPs)" % (S, M, ms, fl / ms / 1e9))
            del A, out
    if args.only in ('', 'conv1x1h'):
        # config 5: conv1 on fp16 block buffers
        H = torch.float16
        for S, K, ct in shapes:
            M = n * S * S
            A = torch.randn(M, ct, device=DEV).to(H)
            W = (torch.randn(128, K, device=DEV) * 0.05).to(H)
            out = torch.empty(M, 128, device=DEV, dtype=H)
            sc, sh = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1
            osc, osh = torch.rand(128, device=DEV) + 0.5, torch.randn(128, device=DEV) * 0.1
            scp, shp = (None, None) if args.noact else (L.ptr(sc), L.ptr(sh))
            ms = timeit(lambda: L.call('gnx_conv1x1_bnrelu_h16', L.ptr(A, H), ct, L.ptr(W, H), L.ptr(out, H), 128, M, 128, K,
                                       scp, shp, L.ptr(osc), L.ptr(osh), st), args.reps)
            print("conv1x1_h16 S=%2d K=%4d M=%8d  %8.3f ms  %6.1f TFLOP/s  %5.2f TB/s (fp16 bytes)" %
                  (S, K, M, ms, 2.0 * M * K * 128 / ms / 1e9, 2.0 * M * (K + 128) / ms / 1e9))
            del A, out
    if args.only in ('fused', 'fusedcmp'):
        # config 5: one dense layer as ONE kernel (gnx_dense_layer_f16) on the 256-px shapes (--spots: images per launch);
        # 'fusedcmp' also times the two-kernel pair it replaces.  TB/s = algorithmic bytes of the fused layer (K columns in,
        # 32 out) over the time.
        H = torch.float16
        fshapes = [(64, 64, 256), (64, 128, 256), (64, 224, 256), (32, 128, 512), (32, 480, 512), (16, 256, 1024),
                   (16, 992, 1024), (8, 512, 1024), (8, 992, 1024)]
        for S, K, ct in fshapes:
            M = n * S * S
            X = torch.randn(ct // 32, M, 32, device=DEV).to(H)          # channel-blocked [ct / 32][rows][32]
            W1 = torch.randn(128, K, device=DEV) * (1.0 / K ** 0.5)
            W2 = torch.randn(32, 128, 3, 3, device=DEV) * 0.05
            sc, sh = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1
            osc, osh = torch.rand(128, device=DEV) + 0.5, torch.randn(128, device=DEV) * 0.1
            w1p = torch.empty(128 * K, device=DEV, dtype=H)
            w2p = torch.empty(9 * 8 * 512, device=DEV, dtype=H)
            L.call('gnx_dense_layer_f16_pack', L.ptr(W1), L.ptr(W2), L.ptr(w1p, H), L.ptr(w2p, H), K, st)
            ms = timeit(lambda: L.call('gnx_dense_layer_f16', L.ptr(X, H), M, n, S, K, L.ptr(w1p, H), L.ptr(w2p, H), L.ptr(sc),
                                       L.ptr(sh), L.ptr(osc), L.ptr(osh), st), args.reps)
            byts = M * (2.0 * K + 64)
            fl = 2.0 * M * 128 * (K + 9 * 32)
            line = "fused S=%2d K=%4d M=%8d  %8.3f ms  %5.2f TB/s  %6.1f TFLOP/s" % (S, K, M, ms, byts / ms / 1e9, fl / ms / 1e9)
            if args.only == 'fusedcmp' and M * ct < 2 ** 31:
                Xr = torch.randn(M, ct, device=DEV).to(H)                  # the pair works on a row-major buffer
                bott = torch.empty(M, 128, device=DEV, dtype=H)
                W16 = W1.to(H)
                Wr = torch.empty(9, 32, 128, device=DEV)
                L.call('gnx_repack_conv3x3', L.ptr(W2), L.ptr(Wr), 32, 128, st)
                Wr16 = Wr.to(H)

                def pair():
                    L.call('gnx_conv1x1_bnrelu_h16', L.ptr(Xr, H), ct, L.ptr(W16, H), L.ptr(bott, H), 128, M, 128, K, L.ptr(sc),
                           L.ptr(sh), L.ptr(osc), L.ptr(osh), st)
                    L.call('gnx_conv3x3_f16_dma_h', L.ptr(bott, H), 128, L.ptr(Wr16, H), Xr.data_ptr() + 2 * K, ct, M, 32, 128, S, st)
                ms2 = timeit(pair, args.reps)
                line += "   | pair %8.3f ms (x%.2f)" % (ms2, ms2 / ms)
                del bott, Xr
            print(line, flush=True)
            del X
    if args.only in ('', 'wgrad1'):
        # weight gradient of conv1 (taps = 1): dW[128][K] = dY^T act(X); GNX_WGRAD_R1=1 selects the round-1 kernels
        for S, K, ct in shapes:
            M = n * S * S
            X = torch.randn(M, ct, device=DEV)
            dY = torch.randn(M, 128, device=DEV)
            sc, sh = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1
            dW = torch.empty(128, K, device=DEV)
            ws = torch.empty(L.query('gnx_wgrad_workspace', M, 128, K, 1), device=DEV)
            ms = timeit(lambda: L.call('gnx_wgrad_bnrelu', L.ptr(dY), 128, L.ptr(X), ct, L.ptr(sc), L.ptr(sh), L.ptr(dW),
                                       L.ptr(ws), M, 128, K, 0, 1, 0, 0, st), args.reps)
            fl = 2.0 * M * K * 128
            print("wgrad1x1 S=%2d K=%4d M=%8d  %8.3f ms  %6.1f TFLOP/s  %5.2f TB/s" %
                  (S, K, M, ms, fl / ms / 1e9, 4.0 * M * (K + 128) / ms / 1e9))
            del X, dY, ws
    if args.only in ('', 'wgrad9'):
        for S in (32, 16, 8, 4):
            M = n * S * S
            X = torch.randn(M, 128, device=DEV)
            ct = 256
            dY = torch.randn(M, ct, device=DEV)
            dW = torch.empty(32, 128, 3, 3, device=DEV)
            sc, sh = torch.rand(128, device=DEV) + 0.5, torch.randn(128, device=DEV) * 0.1
            scp, shp = (None, None) if args.noact else (L.ptr(sc), L.ptr(sh))
            ws = torch.empty(L.query('gnx_wgrad_workspace', M, 32, 128, 9), device=DEV)
            ms = timeit(lambda: L.call('gnx_wgrad_bnrelu', dY.data_ptr() + 4 * 64, ct, L.ptr(X), 128, scp, shp, L.ptr(dW),
                                       L.ptr(ws), M, 32, 128, S, 9, 0, 0, st), args.reps)
            fl = 2.0 * M * 1152 * 32
            print("wgrad3x3 S=%2d M=%8d  %8.3f ms  %6.1f TFLOP/s" % (S, M, ms, fl / ms / 1e9))
            del X, dY, ws
    if args.only in ('', 'gemm'):
        # the count MLP's first Linear on one array: C[4992][500] = A^T W^T, A = the (genes, spots) count grid read in place
        M, N, K = 4992, 500, 2000
        A = torch.randn(K, M, device=DEV)
        W = torch.randn(N, K, device=DEV) * 0.05
        Wt = W.t().contiguous()
        bias = torch.randn(N, device=DEV)
        C = torch.empty(M, N, device=DEV)
        nws = L.query('gnx_gemm_f32_workspace', M, N, K)
        ws = torch.empty(nws, device=DEV) if nws else None
        print('gemm workspace floats', nws)
        for bk, Bm, ldb in ((0, W, K), (1, Wt, N)):
            ms = timeit(lambda: L.call('gnx_gemm_f32_ws', L.ptr(A), M, 1, L.ptr(Bm), ldb, bk, L.ptr(bias), L.ptr(C), N, M, N, K, 0, L.ptr(ws), st),
                        args.reps)
            print("gemm kmajor-A M=%d N=%d K=%d b_kmajor=%d  %8.3f ms  %6.1f TFLOP/s" % (M, N, K, bk, ms, 2.0 * M * N * K / ms / 1e9))
    if args.only in ('', 'stem'):
        x = torch.rand(n, 3, 128, 128, device=DEV)
        w = torch.randn(64, 3, 7, 7, device=DEV) * 0.05
        out = torch.empty(n * 64 * 64, 64, device=DEV)
        ms = timeit(lambda: L.call('gnx_conv_stem', L.ptr(x), L.ptr(w), L.ptr(out), 64, n, 3, 128, 128, 64, 7, 7, 2, 3,
                                   st), args.reps)
        fl = 2.0 * n * 64 * 64 * 147 * 64
        print("stem7x7 n=%d  %8.3f ms  %6.1f TFLOP/s  (in %.2f GB, out %.2f GB -> %.2f TB/s)" %
              (n, ms, fl / ms / 1e9, x.numel() * 4 / 1e9, out.numel() * 4 / 1e9, (x.numel() + out.numel()) * 4 / ms / 1e9))
        if args.only in ('', 'stem', 'pool'):
            sc, sh = torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV) * 0.1
            pooled = torch.empty(n * 32 * 32, 256, device=DEV)
            ms = timeit(lambda: L.call('gnx_bnrelu_maxpool', L.ptr(out), 64, L.ptr(pooled), 256, n, 64, 64, 64,
                                       L.ptr(sc), L.ptr(sh), st), args.reps)
            print("maxpool n=%d  %8.3f ms  %.2f TB/s" % (n, ms, (out.numel() + n * 32 * 32 * 64) * 4 / ms / 1e9))
    if args.only == 'dgrad0':
        # conv0's gradient with respect to the patches (gnx_conv0_dgrad): 128-px patches, O = 64; --spots 512 is the quoted run
        dS = torch.randn(n * 64 * 64, 64, device=DEV)
        w = torch.randn(64, 3, 7, 7, device=DEV) * 0.05
        dX = torch.empty(n, 3, 128, 128, device=DEV)
        ms = timeit(lambda: L.call('gnx_conv0_dgrad', L.ptr(dS), 64, L.ptr(w), L.ptr(dX), n, 128, 128, 64, 7, 7, 2, 3, st),
                    args.reps)
        fl = 2.0 * n * 64 * 64 * 147 * 64
        print("conv0_dgrad n=%d  %9.1f us  %6.2f TFLOP/s  %7.1f GB/s  (in %.3f GB, out %.3f GB)" %
              (n, ms * 1e3, fl / ms / 1e9, (dS.numel() + dX.numel()) * 4 / ms / 1e6, dS.numel() * 4 / 1e9, dX.numel() * 4 / 1e9))
    if args.only == 'resize':
        # the tutorials' Resize(256) + CenterCrop(224) on stored 260-px uint8 patches (gnx_resize_crop_u8, and its float form),
        # then 146 -> 128 px for the fused uint8 stem; GB/s = stored bytes in + window bytes out over the time
        from gridnext_amd.transforms import resize_crop
        for P0, rs, cr in ((260, 256, 224), (146, 128, 128)):
            x = torch.randint(0, 256, (n, 3, P0, P0), device=DEV, dtype=torch.uint8)
            for as_float in (False, True):
                ms = timeit(lambda: resize_crop(x, rs, cr, None, as_float), args.reps)
                byts = 3.0 * n * (P0 * P0 + cr * cr * (4 if as_float else 1))
                print("resize_crop %s n=%d %d -> %d -> %d px  %9.1f us  %7.1f GB/s  (in %.3f GB, out %.3f GB)" %
                      ('u8->f32' if as_float else 'u8->u8 ', n, P0, rs, cr, ms * 1e3, byts / ms / 1e6, 3.0 * n * P0 * P0 / 1e9,
                       3.0 * n * cr * cr * (4 if as_float else 1) / 1e9), flush=True)
            del x

    if args.only == 'wsi':
        # the patch grid of one Visium array cut out of a resident 20 000 x 20 000 slide (gnx_wsi_patch_grid_u8, and its float
        # form): 78 x 64 spots on Visium spacing (odd rows shifted by half a pitch); GB/s = window bytes in + patch bytes out
        import numpy as np
        from gridnext_amd.transforms import axis_ksize, axis_tables
        S, GH, GW = 20000, 78, 64
        slide = torch.randint(0, 256, (S, S, 3), device=DEV, dtype=torch.uint8)
        pitch = (S - 3000) / GW
        spots = np.array([(int(1500 + pitch * (c + 0.5 * (r % 2))), int(1500 + pitch * 0.866 * r), r, c)
                          for r in range(GH) for c in range(GW)], dtype=np.int32)[:n]
        # the plain rows first, as they always ran (their figures compare across commits); then per row the colour-cast table
        # folded into the gather (the _lut form) and what it replaces: gnx_rgb_lut_u8 of the whole slide into a second
        # slide-sized buffer + the plain gather, timed together
        corrected = lut = None
        for folded in (False, True):
            if folded:
                corrected = torch.empty_like(slide)
                lut = torch.randint(0, 256, (3, 256), device=DEV, dtype=torch.uint8)
            for P, w in ((256, 256), (256, 320), (128, 256)):
                coef, bnd = (torch.from_numpy(a).to(DEV) for a in axis_tables(w, P, filter='bicubic'))
                ks = axis_ksize(w, P, 'bicubic')
                for as_float in (False, True):
                    out = torch.zeros((GH, GW, 3, P, P), device=DEV, dtype=torch.float32 if as_float else torch.uint8)
                    a = (slide.data_ptr(), S, S, spots.ctypes.data, len(spots), w // 2, P, GH, GW, coef.data_ptr(),
                         bnd.data_ptr(), ks, out.data_ptr())
                    name = 'gnx_wsi_patch_grid_u8_f32' if as_float else 'gnx_wsi_patch_grid_u8'
                    tail = (None,) if as_float else ()
                    b_in, b_out = 3.0 * len(spots) * w * w, 3.0 * len(spots) * P * P * (4 if as_float else 1)
                    what = "%s n=%d window %d -> %d px (%s)" % ('u8->f32' if as_float else 'u8->u8 ', len(spots), w, P,
                                                                'copy' if w == P else 'bicubic ksize %d' % ks)
                    if not folded:
                        ms = timeit(lambda: L.call(name, *a, *tail, st), args.reps)
                        print("wsi_patch_grid %s  %9.1f us  %7.1f GB/s  (in %.3f GB, out %.3f GB)" %
                              (what, ms * 1e3, (b_in + b_out) / ms / 1e6, b_in / 1e9, b_out / 1e9), flush=True)
                    else:
                        ms = timeit(lambda: L.call(name + '_lut', *a, *tail, lut.data_ptr(), st), args.reps)
                        a2 = (corrected.data_ptr(),) + a[1:]

                        def lookup_then_gather():
                            L.call('gnx_rgb_lut_u8', slide.data_ptr(), corrected.data_ptr(), S * S, lut.data_ptr(), st)
                            L.call(name, *a2, *tail, st)
                        ms2 = timeit(lookup_then_gather, args.reps)
                        print("wsi_patch_grid_lut %s  folded %9.1f us  %7.1f GB/s | lookup of the slide (+ %.1f GB) + gather "
                              "%9.1f us" % (what, ms * 1e3, (b_in + b_out) / ms / 1e6, 3.0 * S * S / 1e9, ms2 * 1e3), flush=True)
                    del out

    if args.only == 'colorcast':
        # the two passes of remove_color_cast over a resident 20 000 x 20 000 slide (gnx_rgb_hist_u8: read-only; gnx_rgb_lut_u8:
        # one read, one write), a random slide and a constant one (the background of a real slide: every add on one counter);
        # to be read beside tools/ubench/stream_mix.hip's read-only and copy figures of the same session
        S = 20000
        n = S * S
        slide = torch.empty((S, S, 3), device=DEV, dtype=torch.uint8)
        out = torch.empty_like(slide)
        hist = torch.empty(768, device=DEV, dtype=torch.int64)
        ws = torch.empty(L.query('gnx_rgb_hist_u8_workspace', n) // 8, device=DEV, dtype=torch.int64)
        lut = torch.randint(0, 256, (3, 256), device=DEV, dtype=torch.uint8)
        reps = max(args.reps, 20)
        for kind in ('random', 'constant'):
            if kind == 'random':
                for y0 in range(0, S, 2000):
                    slide[y0:y0 + 2000] = torch.randint(0, 256, (2000, S, 3), device=DEV, dtype=torch.uint8)
            else:
                slide.copy_(torch.tensor([228, 190, 241], device=DEV, dtype=torch.uint8).expand(S, S, 3))
            for _ in range(3):
                L.call('gnx_rgb_hist_u8', slide.data_ptr(), n, hist.data_ptr(), ws.data_ptr(), st)
                L.call('gnx_rgb_lut_u8', slide.data_ptr(), out.data_ptr(), n, lut.data_ptr(), st)
            ms = timeit(lambda: L.call('gnx_rgb_hist_u8', slide.data_ptr(), n, hist.data_ptr(), ws.data_ptr(), st), reps)
            assert int(hist.sum()) == 3 * n
            print("colorcast hist   %-8s slide %d x %d  %9.1f us  %7.1f GB/s  (in %.3f GB)" %
                  (kind, S, S, ms * 1e3, 3.0 * n / ms / 1e6, 3.0 * n / 1e9), flush=True)
            ms = timeit(lambda: L.call('gnx_rgb_lut_u8', slide.data_ptr(), out.data_ptr(), n, lut.data_ptr(), st), reps)
            print("colorcast lookup %-8s slide %d x %d  %9.1f us  %7.1f GB/s  (in %.3f GB, out %.3f GB)" %
                  (kind, S, S, ms * 1e3, 6.0 * n / ms / 1e6, 3.0 * n / 1e9, 3.0 * n / 1e9), flush=True)
            ms = timeit(lambda: L.call('gnx_rgb_lut_u8', out.data_ptr(), out.data_ptr(), n, lut.data_ptr(), st), reps)
            print("colorcast lookup %-8s in place           %9.1f us  %7.1f GB/s" % (kind, ms * 1e3, 6.0 * n / ms / 1e6), flush=True)

    if args.only == 'augment':
        # train-time augmentation of one array's patches (gnx_patch_augment_u8 and its float form): every patch the same code
        # class - identity, a flip within the rows, a transposing turn - or all eight mixed; with and without per-patch tables;
        # then the grey sums.  GB/s = patch bytes in + patch bytes (or floats) out; to be read beside gnx_rgb_lut_u8's
        # out-of-place figure over the same number of bytes (last line of a size) and tools/ubench/stream_mix.hip's copy rate
        reps = max(args.reps, 20)
        for P in (128, 256):
            x = torch.randint(0, 256, (n, 3, P, P), device=DEV, dtype=torch.uint8)
            luts = torch.randint(0, 256, (n, 3, 256), device=DEV, dtype=torch.uint8)
            classes = (('identity', torch.zeros(n, dtype=torch.uint8)), ('fliplr', torch.full((n,), 4, dtype=torch.uint8)),
                       ('flipud', torch.full((n,), 6, dtype=torch.uint8)), ('rot90', torch.ones(n, dtype=torch.uint8)),
                       ('mixed', torch.arange(n, dtype=torch.int64).remainder(8).to(torch.uint8)))
            for as_float in (False, True):
                out = torch.empty((n, 3, P, P), device=DEV, dtype=torch.float32 if as_float else torch.uint8)
                name = 'gnx_patch_augment_u8_f32' if as_float else 'gnx_patch_augment_u8'
                tail = (None,) if as_float else ()
                byts = 3.0 * n * P * P * (5 if as_float else 2)
                for label, codes in classes:
                    codes = codes.to(DEV)
                    for tab in (None, luts):
                        ms = timeit(lambda: L.call(name, x.data_ptr(), out.data_ptr(), n, P, n, codes.data_ptr(),
                                                   None if tab is None else tab.data_ptr(), None, *tail, st), reps)
                        print("augment %s n=%d %d px %-8s %-9s %9.1f us  %7.1f GB/s" %
                              ('u8->f32' if as_float else 'u8->u8 ', n, P, label, 'tables' if tab is not None else 'no tables',
                               ms * 1e3, byts / ms / 1e6), flush=True)
                del out
            sums = torch.empty(n, device=DEV, dtype=torch.int64)
            ms = timeit(lambda: L.call('gnx_patch_grey_sum_u8', x.data_ptr(), n, P, sums.data_ptr(), st), reps)
            print("augment grey sums n=%d %d px  %9.1f us  %7.1f GB/s  (in %.3f GB)" %
                  (n, P, ms * 1e3, 3.0 * n * P * P / ms / 1e6, 3.0 * n * P * P / 1e9), flush=True)
            out = torch.empty_like(x)
            ms = timeit(lambda: L.call('gnx_rgb_lut_u8', x.data_ptr(), out.data_ptr(), n * P * P, luts.data_ptr(), st), reps)
            print("gnx_rgb_lut_u8 out of place over the same %.3f GB  %9.1f us  %7.1f GB/s" %
                  (3.0 * n * P * P / 1e9, ms * 1e3, 6.0 * n * P * P / ms / 1e6), flush=True)
            del x, out, luts

    if args.only == 'augment_hs':
        # saturation / hue jitter of one array's patches (gnx_patch_augment_hs_u8 and its float form): mixed codes, per-patch
        # tables, random factors in [0, 2] and random shifts; saturation only, hue only and both.  Every time stands next to the
        # yardsticks of the same run over the same bytes: gnx_patch_augment_u8[_f32] with tables (the same traffic without the
        # colour arithmetic) and gnx_rgb_lut_u8 out of place.  GB/s = patch bytes in + patch bytes (or floats) out
        reps = max(args.reps, 20)
        for P in (128, 256):
            g = torch.Generator(device=DEV).manual_seed(P)
            x = torch.randint(0, 256, (n, 3, P, P), device=DEV, dtype=torch.uint8, generator=g)
            luts = torch.randint(0, 256, (n, 3, 256), device=DEV, dtype=torch.uint8, generator=g)
            codes = torch.arange(n, dtype=torch.int64).remainder(8).to(torch.uint8).to(DEV)
            sat = 2.0 * torch.rand(n, device=DEV, generator=g)
            hue = torch.randint(0, 256, (n,), device=DEV, dtype=torch.uint8, generator=g)
            for as_float in (False, True):
                out = torch.empty((n, 3, P, P), device=DEV, dtype=torch.float32 if as_float else torch.uint8)
                sfx = '_f32' if as_float else ''
                tail = (None,) if as_float else ()
                byts = 3.0 * n * P * P * (5 if as_float else 2)
                form = 'u8->f32' if as_float else 'u8->u8 '
                base = timeit(lambda: L.call('gnx_patch_augment_u8' + sfx, x.data_ptr(), out.data_ptr(), n, P, n, codes.data_ptr(),
                                             luts.data_ptr(), None, *tail, st), reps)
                print("augment_hs %s n=%d %d px %-15s %9.1f us  %7.1f GB/s" %
                      (form, n, P, 'augment_u8%s' % sfx, base * 1e3, byts / base / 1e6), flush=True)
                for label, s, h in (('no stage', None, None), ('saturation', sat, None), ('hue', None, hue), ('both', sat, hue)):
                    ms = timeit(lambda: L.call('gnx_patch_augment_hs_u8' + sfx, x.data_ptr(), out.data_ptr(), n, P, n,
                                               codes.data_ptr(), luts.data_ptr(), None if s is None else s.data_ptr(),
                                               None if h is None else h.data_ptr(), None, *tail, st), reps)
                    print("augment_hs %s n=%d %d px %-15s %9.1f us  %7.1f GB/s  %5.2f x augment_u8%s" %
                          (form, n, P, label, ms * 1e3, byts / ms / 1e6, ms / base, sfx), flush=True)
                del out
            out = torch.empty_like(x)
            ms = timeit(lambda: L.call('gnx_rgb_lut_u8', x.data_ptr(), out.data_ptr(), n * P * P, luts.data_ptr(), st), reps)
            print("gnx_rgb_lut_u8 out of place over the same %.3f GB  %9.1f us  %7.1f GB/s" %
                  (3.0 * n * P * P / 1e9, ms * 1e3, 6.0 * n * P * P / ms / 1e6), flush=True)
            del x, out, luts

    if args.only == 'metrics':
        # the evaluation stage: gnx_clf_curve (curves + areas, and areas alone) and gnx_confusion_counts over one run's
        # predictions (12 arrays of 4 992 spots) and over 2^22 spots, 7 classes.  "moved" is what the curve's kernels read and
        # write by their code, per score: the key build 4 + 8 (+ 8 / C for the label), four passes of histogram read (8), scatter
        # read (8) and write (8), the count pass (8) and the compaction's read (8) = 4 + 8 + 4 * 24 + 8 + 8 = 124 bytes; per
        # threshold: the compaction's 8 + 4, the integration's 8, and 16 more with the curve outputs.  GB/s is that figure over
        # the time
        reps = max(args.reps, 20)
        C = 7
        for n in (12 * 4992, 1 << 22):
            for kind in ('softmax', 'q64'):
                g = torch.Generator(device=DEV).manual_seed(n % 1000)
                s = torch.softmax(3 * torch.randn((n, C), device=DEV, generator=g), 1)
                if kind == 'q64':
                    s = torch.round(s * 64) / 64
                y = torch.randint(0, C, (n,), device=DEV, generator=g)
                pred = s.argmax(1)
                ws = torch.empty(L.query('gnx_clf_curve_workspace', n, C) // 8, device=DEV, dtype=torch.int64)
                thr = torch.empty((C, n), device=DEV)
                tps, fps = (torch.empty((C, n), device=DEV, dtype=torch.int64) for _ in range(2))
                n_thr, bad = torch.empty(C, device=DEV, dtype=torch.int64), torch.empty(1, device=DEV, dtype=torch.int64)
                auroc, auprc = (torch.empty(C, device=DEV, dtype=torch.float64) for _ in range(2))
                counts = torch.empty((C, C), device=DEV, dtype=torch.int64)

                def curve(full):
                    L.call('gnx_clf_curve', s.data_ptr(), C, y.data_ptr(), n, C, thr.data_ptr() if full else None,
                           tps.data_ptr() if full else None, fps.data_ptr() if full else None, n_thr.data_ptr(),
                           auroc.data_ptr(), auprc.data_ptr(), bad.data_ptr(), ws.data_ptr(), st)
                for full in (True, False):
                    ms = timeit(lambda: curve(full), reps)
                    moved = (124.0 * C + 8) * n + float(n_thr.sum()) * (36 if full else 20)
                    print("metrics clf_curve %-7s n=%d C=%d %-11s %9.1f us  %6.2f ns/score  ~%6.1f GB/s moved (workspace %.1f MB, "
                          "T of class 0: %d)" % (kind, n, C, 'curves+aucs' if full else 'aucs only', ms * 1e3,
                                                 ms * 1e6 / (n * C), moved / ms / 1e6, ws.numel() * 8 / 1e6, int(n_thr[0])),
                          flush=True)
                assert int(bad) == 0
                ms = timeit(lambda: L.call('gnx_confusion_counts', y.data_ptr(), pred.data_ptr(), n, C, counts.data_ptr(),
                                           bad.data_ptr(), st), reps)
                assert int(counts.sum()) == n
                print("metrics confusion %-7s n=%d K=%d             %9.1f us  %7.1f GB/s  (in %.4f GB)" %
                      (kind, n, C, ms * 1e3, 16.0 * n / ms / 1e6, 16.0 * n / 1e9), flush=True)
            one = torch.zeros(n, device=DEV, dtype=torch.int64)
            ms = timeit(lambda: L.call('gnx_confusion_counts', one.data_ptr(), one.data_ptr(), n, C, counts.data_ptr(),
                                       bad.data_ptr(), st), reps)
            print("metrics confusion one cell n=%d K=%d            %9.1f us  %7.1f GB/s" % (n, C, ms * 1e3, 16.0 * n / ms / 1e6),
                  flush=True)

    if args.only == 'counts':
        # csrc/sparse_counts.hip over one array of 4 992 spots: the selected 2 000 genes at 10 % non-zeros and the whole
        # transcriptome of 33 000 genes at 3 %.  Expand in both uses (rows of spots from the CSR; the channel-first 78 x 64 grid
        # from the CSC), "written" being the dense output; the moments, divisions and log1p over all entries, "moved" being the
        # idx / val bytes their code reads and writes per entry.  To be read beside tools/ubench/stream_mix.hip's figures of
        # the same session
        reps = max(args.reps, 20)
        S, H, W = 4992, 78, 64

        def lines_of(mask):
            at = mask.nonzero()                                      # row-major: indices ascending within a line
            ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mask.sum(1).cumsum(0)])
            val = torch.randint(1, 50, (at.shape[0],), device=DEV).float()
            return ptr, at[:, 1].int().contiguous(), val
        for rnd in range(args.rounds):
            for G, density in ((2000, 0.10), (33000, 0.03)):
                g = torch.Generator(device=DEV).manual_seed(G)
                mask = torch.rand((S, G), device=DEV, generator=g) < density
                rptr, ridx, rval = lines_of(mask)
                cptr, cidx, cval = lines_of(mask.t().contiguous())
                del mask
                nnz = rval.numel()
                cells = torch.randperm(H * W, device=DEV, generator=g)[:S].int()
                one_s = torch.ones(S, device=DEV)
                rows, grid = torch.empty((S, G), device=DEV), torch.empty((G, H * W), device=DEV)
                mom = torch.empty((max(S, G), 2), device=DEV, dtype=torch.float64)
                tag = "round %d counts G=%5d nnz=%9d" % (rnd, G, nnz)
                ms = timeit(lambda: L.call('gnx_sparse_expand_f32', rptr.data_ptr(), ridx.data_ptr(), rval.data_ptr(), None, S,
                                           None, rows.data_ptr(), G, G, st), reps)
                assert float(rows.sum(dtype=torch.float64)) == float(rval.sum(dtype=torch.float64))
                print("%s expand rows (S, G)      %9.1f us  %7.1f GB/s written (%.3f GB) + %.3f GB read" %
                      (tag, ms * 1e3, 4.0 * S * G / ms / 1e6, 4.0 * S * G / 1e9, 8.0 * nnz / 1e9), flush=True)
                ms = timeit(lambda: L.call('gnx_sparse_expand_f32', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None, G,
                                           cells.data_ptr(), grid.data_ptr(), H * W, H * W, st), reps)
                assert float(grid.sum(dtype=torch.float64)) == float(cval.sum(dtype=torch.float64))
                print("%s expand grid (G, 78, 64) %9.1f us  %7.1f GB/s written (%.3f GB) + %.3f GB read" %
                      (tag, ms * 1e3, 4.0 * G * H * W / ms / 1e6, 4.0 * G * H * W / 1e9, 8.0 * nnz / 1e9), flush=True)
                for what, (ptr, idx, val, n) in (('genes (CSC)', (cptr, cidx, cval, G)), ('spots (CSR)', (rptr, ridx, rval, S))):
                    ms = timeit(lambda: L.call('gnx_sparse_line_moments_f64', ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), None,
                                               n, None, mom.data_ptr(), st), reps)
                    print("%s moments %-14s %9.1f us  %7.1f GB/s moved (val only: %.3f GB)" %
                          (tag, what, ms * 1e3, 4.0 * nnz / ms / 1e6, 4.0 * nnz / 1e9), flush=True)
                ms = timeit(lambda: L.call('gnx_sparse_div_by_line_f32', rptr.data_ptr(), rval.data_ptr(), S, one_s.data_ptr(), st),
                            reps)
                print("%s div by line (CSR)      %9.1f us  %7.1f GB/s moved (val in + out)" %
                      (tag, ms * 1e3, 8.0 * nnz / ms / 1e6), flush=True)
                ms = timeit(lambda: L.call('gnx_sparse_div_by_idx_f32', cidx.data_ptr(), cval.data_ptr(), nnz, one_s.data_ptr(), st),
                            reps)
                print("%s div by idx (CSC)       %9.1f us  %7.1f GB/s moved (idx + val in + out)" %
                      (tag, ms * 1e3, 12.0 * nnz / ms / 1e6), flush=True)
                ms = timeit(lambda: L.call('gnx_log1p_f32', rval.data_ptr(), nnz, st), reps)
                print("%s log1p                  %9.1f us  %7.1f GB/s moved (val in + out)" %
                      (tag, ms * 1e3, 8.0 * nnz / ms / 1e6), flush=True)
                del rows, grid, rptr, ridx, rval, cptr, cidx, cval

    if args.only == 'sparse_linear':
        # csrc/sparse_linear.hip over the two matrices of --only counts, F = 500, batches of 128 rows and of the whole array:
        # the sparse forward beside expand + gnx_gemm_f32_ws, the sparse weight gradient beside the dense _Linear backward's
        # (functional.py: gnx_gemm_f32 below 2 048 rows, gnx_wgrad_bnrelu from there; expand not counted: the dense tape holds
        # the operand).  "gathered" = nnz of the batch x 4 F bytes of W (forward) or dY (gradient) rows.  Medians and the
        # spread over --rounds at the end
        import statistics
        reps = max(args.reps, 20)
        S, F = 4992, 500
        table = {}

        def lines_of(mask, values):
            at = mask.nonzero()
            ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mask.sum(1).cumsum(0)])
            return ptr, at[:, 1].int().contiguous(), values[mask]                    # row-major: the order of `at`

        def note(key, ms, text):
            table.setdefault(key, []).append(ms * 1e3)
            print("%-58s %9.1f us  %s" % (key, ms * 1e3, text), flush=True)
        for rnd in range(args.rounds):
            for G, density in ((2000, 0.10), (33000, 0.03)):
                g = torch.Generator(device=DEV).manual_seed(G)
                mask = torch.rand((S, G), device=DEV, generator=g) < density
                values = torch.rand((S, G), device=DEV, generator=g) * 5 + 0.1          # one matrix, both orientations
                rptr, ridx, rval = lines_of(mask, values)
                cptr, cidx, cval = lines_of(mask.t().contiguous(), values.t().contiguous())
                del mask, values
                Wg = torch.randn(G, F, device=DEV, generator=g) * 0.02                 # gene-major
                Wd = Wg.t().contiguous()                                               # nn.Linear's layout
                bias = torch.randn(F, device=DEV, generator=g)
                for B in (128, S):
                    batch = torch.randperm(S, device=DEV, generator=g)[:B].int()
                    pos = torch.full((S,), -1, device=DEV, dtype=torch.int32)
                    pos[batch.long()] = torch.arange(B, device=DEV, dtype=torch.int32)
                    nnz_b = int((rptr[batch.long() + 1] - rptr[batch.long()]).sum())
                    x = torch.empty((B, G), device=DEV)
                    y, y2 = torch.empty((B, F), device=DEV), torch.empty((B, F), device=DEV)
                    dY = torch.randn(B, F, device=DEV, generator=g)
                    dWg, dWd = torch.empty((G, F), device=DEV), torch.empty((F, G), device=DEV)
                    nws = L.query('gnx_gemm_f32_workspace', B, F, G)
                    ws = torch.empty(max(nws, 1), device=DEV)
                    tag = "G=%5d B=%4d" % (G, B)
                    ms = timeit(lambda: L.call('gnx_sparse_linear_fwd_f32', rptr.data_ptr(), ridx.data_ptr(), rval.data_ptr(),
                                               batch.data_ptr(), B, None, L.ptr(Wg), F, L.ptr(bias), L.ptr(y), F, F, st), reps)
                    note(tag + " forward sparse", ms, "%7.1f GB/s gathered (%.3f GB)" % (4.0 * F * nnz_b / ms / 1e6, 4.0 * F * nnz_b / 1e9))

                    def dense_fwd():
                        L.call('gnx_sparse_expand_f32', rptr.data_ptr(), ridx.data_ptr(), rval.data_ptr(), batch.data_ptr(), B, None,
                               L.ptr(x), G, G, st)
                        L.call('gnx_gemm_f32_ws', L.ptr(x), G, 0, L.ptr(Wd), G, 0, L.ptr(bias), L.ptr(y2), F, B, F, G, 0,
                               L.ptr(ws) if nws else None, st)
                    ms = timeit(dense_fwd, reps)
                    note(tag + " forward expand + gnx_gemm_f32_ws", ms, "%6.1f TFLOP/s dense" % (2.0 * B * G * F / ms / 1e9))
                    assert torch.allclose(y, y2, rtol=1e-3, atol=1e-3)
                    ms = timeit(lambda: L.call('gnx_sparse_linear_wgrad_f32', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None, G,
                                               pos.data_ptr(), L.ptr(dY), F, L.ptr(dWg), F, F, 0, st), reps)
                    note(tag + " weight gradient sparse", ms, "%7.1f GB/s gathered (%.3f GB) + %.3f GB of idx read" %
                         (4.0 * F * nnz_b / ms / 1e6, 4.0 * F * nnz_b / 1e9, 4.0 * cval.numel() / 1e9))
                    if B >= 2048:
                        wws = torch.empty(L.query('gnx_wgrad_workspace', B, F, G, 1), device=DEV)
                        dense_wg = lambda: L.call('gnx_wgrad_bnrelu', L.ptr(dY), F, L.ptr(x), G, None, None, L.ptr(dWd), L.ptr(wws),   # noqa: E731
                                                  B, F, G, 0, 1, 0, 0, st)
                    else:
                        dense_wg = lambda: L.call('gnx_gemm_f32', L.ptr(dY), F, 1, L.ptr(x), G, 1, None, L.ptr(dWd), G, F, G, B, 0, st)   # noqa: E731
                    ms = timeit(dense_wg, reps)
                    note(tag + " weight gradient dense (_Linear backward)", ms, "%6.1f TFLOP/s dense" % (2.0 * B * G * F / ms / 1e9))
                    assert torch.allclose(dWg, dWd.t(), rtol=1e-3, atol=1e-3 * float(dWd.abs().max()))
                    del x, dWg, dWd
                del rptr, ridx, rval, cptr, cidx, cval, Wg, Wd
        print("\nmedian [min .. max] over %d rounds, us" % args.rounds)
        for key, v in table.items():
            print("%-58s %9.1f [%9.1f .. %9.1f]" % (key, statistics.median(v), min(v), max(v)))

    if args.only == 'gram':
        # csrc/sparse_gram.hip over one array of 4 992 spots: the 2 000 selected genes at 10 % non-zeros of --only counts and,
        # as wide as fit_pca's max_genes allows, 8 192 genes at 3 %.  Beside it, in the same session, torch's float64
        # X.T @ X on the expanded (S, G) array (the expand and the cast not counted: the dense route would hold that operand).
        # "pairs" = the products the sparse walk adds, sum over the spots of (row length)^2.  Medians and the spread over
        # --rounds at the end
        import statistics
        reps = max(args.reps, 10)
        S = 4992
        table = {}

        def lines_of(mask, values):
            at = mask.nonzero()
            ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mask.sum(1).cumsum(0)])
            return ptr, at[:, 1].int().contiguous(), values[mask]

        def note(key, ms, text):
            table.setdefault(key, []).append(ms * 1e3)
            print("%-44s %10.1f us  %s" % (key, ms * 1e3, text), flush=True)
        for rnd in range(args.rounds):
            for G, density in ((2000, 0.10), (8192, 0.03)):
                g = torch.Generator(device=DEV).manual_seed(G)
                mask = torch.rand((S, G), device=DEV, generator=g) < density
                values = torch.rand((S, G), device=DEV, generator=g) * 5 + 0.1
                rptr, ridx, rval = lines_of(mask, values)
                cptr, cidx, cval = lines_of(mask.t().contiguous(), values.t().contiguous())
                X = (values * mask).double()
                del mask, values
                pairs = float(((rptr[1:] - rptr[:-1]).double() ** 2).sum())
                C, Cd = torch.empty((G, G), device=DEV, dtype=torch.float64), torch.empty((G, G), device=DEV, dtype=torch.float64)
                tag = "round %d G=%4d nnz=%8d" % (rnd, G, rval.numel())
                ms = timeit(lambda: L.call('gnx_sparse_gram_f64', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None, G,
                                           rptr.data_ptr(), ridx.data_ptr(), rval.data_ptr(), 0, None, C.data_ptr(), G, 0, st), reps)
                note("G=%4d gram sparse" % G, ms, "%s  %6.1f G pairs/s (%.3f G pairs), C %.3f GB written" %
                     (tag, pairs / ms / 1e6, pairs / 1e9, 8.0 * G * G / 1e9))
                ms = timeit(lambda: torch.matmul(X.t(), X, out=Cd), reps)
                note("G=%4d gram dense float64 X.T @ X" % G, ms, "%s  %6.1f TFLOP/s fp64, operand %.3f GB" %
                     (tag, 2.0 * S * G * G / ms / 1e9, 8.0 * S * G / 1e9))
                worst = float(((C - Cd).abs() / Cd.abs().clamp_min(1e-300)).max())
                assert worst < 1e-12, worst
                del X, C, Cd, rptr, ridx, rval, cptr, cidx, cval
        print("\nmedian [min .. max] over %d rounds, us" % args.rounds)
        for key, v in table.items():
            print("%-44s %10.1f [%10.1f .. %10.1f]" % (key, statistics.median(v), min(v), max(v)))

    if args.only == 'exprmetrics':
        # csrc/expr_moments.hip at a user's size: one array of 4 992 spots x 2 000 genes at about 25 % non-zeros, the whole array
        # as one batch (pos = a permutation of the spots).  "implied" bytes: the dense half reads z once (4 S G) and writes 16 G;
        # the sparse half reads idx and val (8 nnz), one map entry and one gathered z per entry (8 nnz), the line pointers and
        # the scale (12 G) and writes 24 G.  Beside them, in the same session and alternating per round, the torch
        # composition on the device: gnx_sparse_expand_f32 to a dense (S, G) target, then the five sums in float64.
        # Medians and the spread over --rounds at the end
        import statistics
        reps = max(args.reps, 20)
        S, G, density = 4992, 2000, 0.25
        table = {}

        def lines_of(mask, values):
            at = mask.nonzero()
            ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mask.sum(1).cumsum(0)])
            return ptr, at[:, 1].int().contiguous(), values[mask]

        def note(key, ms, text):
            table.setdefault(key, []).append(ms * 1e3)
            print("%-46s %9.1f us  %s" % (key, ms * 1e3, text), flush=True)
        g = torch.Generator(device=DEV).manual_seed(G)
        mask = torch.rand((S, G), device=DEV, generator=g) < density
        values = torch.rand((S, G), device=DEV, generator=g) * 5 + 0.1
        rptr, ridx, rval = lines_of(mask, values)
        cptr, cidx, cval = lines_of(mask.t().contiguous(), values.t().contiguous())
        del mask, values
        nnz = rval.numel()
        z = torch.randn((S, G), device=DEV, generator=g) * 2
        scale = torch.rand(G, device=DEV, generator=g) * 0.19 + 0.001
        batch = torch.randperm(S, device=DEV, generator=g).int()
        pos = torch.empty(S, device=DEV, dtype=torch.int32)
        pos[batch.long()] = torch.arange(S, device=DEV, dtype=torch.int32)
        M = torch.empty((G, 5), device=DEV, dtype=torch.float64)
        x = torch.empty((S, G), device=DEV)
        act = L.CONSTANTS['GNX_ACT_SIGMOID']
        want = [None]

        def dense_half():
            L.call('gnx_act_col_moments_f64', L.ptr(z), G, S, G, act, M.data_ptr(), 5, 0, st)

        def sparse_half():
            L.call('gnx_sparse_pred_moments_f64', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None, G, pos.data_ptr(),
                   L.ptr(scale), L.ptr(z), G, act, M.data_ptr(), 5, 0, st)

        def both():
            dense_half()
            sparse_half()

        def composition():
            L.call('gnx_sparse_expand_f32', rptr.data_ptr(), ridx.data_ptr(), rval.data_ptr(), batch.data_ptr(), S, None, L.ptr(x), G, G, st)
            p, t = torch.sigmoid(z.double()), (x * scale).double()
            want[0] = torch.stack([p.sum(0), (p * p).sum(0), t.sum(0), (t * t).sum(0), (p * t).sum(0)], dim=1)
        db, sb = 4.0 * S * G + 16.0 * G, 16.0 * nnz + 36.0 * G
        for rnd in range(args.rounds):
            tag = "round %d nnz=%d" % (rnd, nnz)
            ms = timeit(dense_half, reps)
            note("dense half  gnx_act_col_moments_f64", ms, "%s  %7.1f GB/s implied (%.4f GB)" % (tag, db / ms / 1e6, db / 1e9))
            ms = timeit(sparse_half, reps)
            note("sparse half gnx_sparse_pred_moments_f64", ms, "%s  %7.1f GB/s implied (%.4f GB)" % (tag, sb / ms / 1e6, sb / 1e9))
            ms = timeit(both, reps)
            note("both halves (one update)", ms, tag)
            ms = timeit(composition, reps)
            note("torch composition: expand + float64 sums", ms, "%s  dense target %.3f GB fp32, %.3f GB as float64" %
                 (tag, 4.0 * S * G / 1e9, 8.0 * S * G / 1e9))
            worst = float(((M - want[0]).abs() / want[0].abs().clamp_min(1e-300)).max())
            assert worst < 1e-11, worst
        print("\nmedian [min .. max] over %d rounds, us" % args.rounds)
        for key, v in table.items():
            print("%-46s %9.1f [%9.1f .. %9.1f]" % (key, statistics.median(v), min(v), max(v)))

    if args.only == 'hvg':
        # The two launches of SpotCounts.highly_variable_genes at a whole transcriptome: one array of 4 992 spots x 33 000 genes
        # at 3 % non-zeros.  gnx_sparse_line_clip_moments_f64 over the array's CSC beside gnx_sparse_line_moments_f64 of the same
        # session, alternating per round ("moved": the val bytes, 4 per entry, plus 8 per line for the bound); gnx_loess_fit_f64
        # at n = 33 000, span 0.3 ("terms": the weighted terms, the sum of the windows' lengths; 8 sums of one term each),
        # and once, in round 0, the host path's numpy loess on the same windows.  Medians and the spread over --rounds at the end
        import statistics
        import time
        import numpy as np
        from gridnext_amd import hvg
        reps = max(args.reps, 20)
        S, G, density = 4992, 33000, 0.03
        table = {}

        def note(key, ms, text):
            table.setdefault(key, []).append(ms * 1e3)
            print("%-44s %10.1f us  %s" % (key, ms * 1e3, text), flush=True)
        g = torch.Generator(device=DEV).manual_seed(G)
        mask = (torch.rand((S, G), device=DEV, generator=g) < density).t().contiguous()
        at = mask.nonzero()
        cptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mask.sum(1).cumsum(0)])
        cidx = at[:, 1].int().contiguous()
        cval = torch.randint(1, 50, (at.shape[0],), device=DEV, generator=g).float()
        del mask, at
        nnz = cval.numel()
        bound = torch.rand(G, device=DEV, generator=g, dtype=torch.float64) * 40 + 5         # cuts about half of the entries
        mom, clipped = (torch.empty((G, 2), device=DEV, dtype=torch.float64) for _ in range(2))
        rng = np.random.default_rng(G)
        xs = np.sort(rng.normal(-0.5, 0.9, G))                                                # log10(mean) of a transcriptome
        ys = 1.1 * xs + 0.15 * xs * xs + rng.normal(0, 0.2, G)
        lo, cnt, inv_h, degree = hvg.loess_windows(xs, 0.3)
        terms = float(cnt.sum())
        dx, dy, dlo, dcnt, dih, ddeg = (torch.from_numpy(a).to(DEV) for a in (xs, ys, lo, cnt, inv_h, degree))
        fit = torch.empty(G, device=DEV, dtype=torch.float64)
        for rnd in range(args.rounds):
            tag = "round %d nnz=%d" % (rnd, nnz)
            ms = timeit(lambda: L.call('gnx_sparse_line_moments_f64', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None, G,
                                       None, mom.data_ptr(), st), reps)
            note("moments      gnx_sparse_line_moments_f64", ms, "%s  %7.1f GB/s moved (val: %.3f GB)" % (tag, 4.0 * nnz / ms / 1e6, 4.0 * nnz / 1e9))
            ms = timeit(lambda: L.call('gnx_sparse_line_clip_moments_f64', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None,
                                       G, None, bound.data_ptr(), clipped.data_ptr(), st), reps)
            note("clip moments gnx_sparse_line_clip_moments_f64", ms, "%s  %7.1f GB/s moved (val + bounds: %.3f GB)" %
                 (tag, (4.0 * nnz + 8.0 * G) / ms / 1e6, (4.0 * nnz + 8.0 * G) / 1e9))
            assert bool((clipped <= mom).all()) and bool((clipped[:, 0] < mom[:, 0]).any())
            ms = timeit(lambda: L.call('gnx_loess_fit_f64', dx.data_ptr(), dy.data_ptr(), G, dlo.data_ptr(), dcnt.data_ptr(),
                                       dih.data_ptr(), ddeg.data_ptr(), fit.data_ptr(), G, st), max(args.reps, 5))
            note("loess        gnx_loess_fit_f64 n=%d" % G, ms, "%s  %7.2f G terms/s (%.3f G terms, window %d)" %
                 (tag, terms / ms / 1e6, terms / 1e9, int(cnt.max())))
            if rnd == 0:
                t0 = time.perf_counter()
                host = hvg.fit_windows(xs, ys, lo, cnt, inv_h, degree)
                sec = time.perf_counter() - t0
                print("%-44s %10.2f s   numpy float64 on the host, the same windows, once" % ("loess        host path n=%d" % G, sec), flush=True)
                worst = float(np.abs(fit.cpu().numpy() - host).max())
                assert worst < 1e-9, worst
                print("largest |device - host| of the fit: %.2e on |y| <= %.1f" % (worst, float(np.abs(ys).max())), flush=True)
        print("\nmedian [min .. max] over %d rounds, us" % args.rounds)
        for key, v in table.items():
            print("%-44s %10.1f [%10.1f .. %10.1f]" % (key, statistics.median(v), min(v), max(v)))


    if args.only == 'spatial':
        # The launches of SpotCounts.spatial_autocorr at a whole transcriptome, the workload of --only hvg on a hexagonal tissue:
        # one array of 4 992 spots (the full 78 x 64 pseudo-hex grid) x 33 000 genes at 3 % non-zeros.  gnx_sparse_line_spatial_f64
        # at K = 6 with 1 table and with 101 (the table and 100 permutations), at K = 18 with 1 table; in the same rounds
        # gnx_sparse_line_moments_f64 over the same CSC - the same values read: the floor of this walk ("gathers": entries x K x
        # tables LDS reads) - and once, in round 0, the host path's scipy A @ X for one table.  Medians and the spread at the end
        import statistics
        import time
        import numpy as np
        from gridnext_amd import spatial
        reps = max(args.reps, 20)
        S, G, density = 4992, 33000, 0.03
        table = {}

        def note(key, ms, text):
            table.setdefault(key, []).append(ms * 1e3)
            print("%-44s %10.1f us  %s" % (key, ms * 1e3, text), flush=True)
        g = torch.Generator(device=DEV).manual_seed(G)
        mask = (torch.rand((S, G), device=DEV, generator=g) < density).t().contiguous()
        at = mask.nonzero()
        cptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mask.sum(1).cumsum(0)])
        cidx = at[:, 1].int().contiguous()
        cval = torch.rand(at.shape[0], device=DEV, generator=g) * 3 + 0.1                     # log-normalised sizes
        del mask, at
        nnz = cval.numel()
        rows, cols = np.divmod(np.arange(S), 64)
        rng = np.random.default_rng(G)
        t6, t18 = (spatial.neighbor_table(2 * cols + rows % 2, rows, r) for r in (1, 2))
        many = np.stack([t6] + [spatial.permuted_table(t6, rng.permutation(S)) for _ in range(100)])
        d6, d18, dmany = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (t6[None], t18[None], many))
        mom = torch.empty((G, 2), device=DEV, dtype=torch.float64)
        outs = {k: torch.empty((n_t, G, 3), device=DEV, dtype=torch.float64) for k, n_t in (('one', 1), ('many', 101))}

        def launch(tab, out):
            n_t, _, K = tab.shape
            L.call('gnx_sparse_line_spatial_f64', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None, G, S, tab.data_ptr(), K,
                   n_t, out.data_ptr(), st)
        for rnd in range(args.rounds):
            tag = "round %d nnz=%d" % (rnd, nnz)
            ms = timeit(lambda: L.call('gnx_sparse_line_moments_f64', cptr.data_ptr(), cidx.data_ptr(), cval.data_ptr(), None, G,
                                       None, mom.data_ptr(), st), reps)
            note("floor        gnx_sparse_line_moments_f64", ms, "%s  %7.1f GB/s moved (val: %.3f GB)" % (tag, 4.0 * nnz / ms / 1e6, 4.0 * nnz / 1e9))
            for key, tab, out, r in (("spatial K=6  1 table", d6, outs['one'], reps), ("spatial K=18 1 table", d18, outs['one'], reps),
                                     ("spatial K=6  101 tables", dmany, outs['many'], max(args.reps, 3))):
                ms = timeit(lambda: launch(tab, out), r)
                gathers = float(nnz) * tab.shape[2] * tab.shape[0]
                note(key, ms, "%s  %7.2f G gathers/s  %7.1f us per table" % (tag, gathers / ms / 1e6, ms * 1e3 / tab.shape[0]))
            if rnd == 0:
                launch(d6, outs['one'])
                dev = outs['one'][0].cpu().numpy()
                trio = tuple(t.cpu() for t in (cptr, cidx, cval))
                t0 = time.perf_counter()
                host = spatial.line_spatial(trio, None, G, S, t6[None], None)[0]
                sec = time.perf_counter() - t0
                print("%-44s %10.2f s   scipy float64 A @ X on the host, one table, once" % ("spatial      host path K=6", sec), flush=True)
                worst = float((np.abs(dev - host) / np.maximum(np.abs(host), 1e-300)).max())
                assert worst < 1e-12, worst
                print("largest relative |device - host| of P, D, Q: %.2e" % worst, flush=True)
                first = outs['many'][0].cpu().numpy()
                assert np.array_equal(first.view(np.int64), dev.view(np.int64))              # table 0 of 101: the same bits
        print("\nmedian [min .. max] over %d rounds, us" % args.rounds)
        for key, v in table.items():
            print("%-44s %10.1f [%10.1f .. %10.1f]" % (key, statistics.median(v), min(v), max(v)))


if __name__ == '__main__':
    main()
