"""DenseNet-BC forward-with-tape and backward on the HIP kernels (training / gradient path).

Used by `DenseNet.forward` whenever the module is in training mode or a gradient is required - i.e.
`train_spotwise` on an image classifier (BatchNorm batch statistics, /root/reference/gridnext/training.py:60-67)
and `train_gridwise` with `f_opt` (f kept in eval mode by training.py:126, but its parameters trained).

MI355X-first: a 128-px array's full tape is ~55 GB of the 288 GB HBM, so by default one tape covers the whole batch and
nothing is recomputed.  Where the reference saves memory (`efficient=True`, densenet.py:36-40; `atonce_patch_limit` chunks
under `cp.checkpoint`, gridnet_models.py:88-104) or where the tape would exceed `DenseNet.tape_budget` (256-px arrays), the
batch goes through in chunks whose forward keeps no tape and whose backward rebuilds it (`_RecomputeFn`).
The tape holds the raw (pre-BN) tensors only: stem output, the dense-block buffers and each layer's 1x1-conv output (stored
activated under running statistics); every other BN+ReLU is re-evaluated inside the consuming kernel's operand load, forward
and backward.  One autograd node covers the whole network; gradients are returned for every parameter that requires one.
`DenseNet.mfma = 'f16'` under running statistics takes the fp16 tape and the fp16-MFMA backward of densenet_train_f16.
An input that requires a gradient gets one (`gnx_conv0_dgrad`, conv0's adjoint in its input, after the stem's backward); a call
whose input requires none launches nothing for it.
"""
import ctypes
import os
import struct
from collections import namedtuple

import torch
from torch.autograd import Function

from . import _lib as L
from .densenet import dense_layer_f32_act
from .functional import _bn_sync


F32 = torch.float32

# One weight gradient dW[N][K][taps] of dY[M][N] (ld lddy) against X[M][K] (ld ldx; device addresses), X under the folded BN
# `stats` + ReLU when given; S: map size, pool: X is the unpooled input of a transition (gnx_wgrad_bnrelu)
_Wgrad = namedtuple('_Wgrad', 'w dy lddy x ldx stats M N K S taps pool')
# One dense layer on the fp32 tape: bottleneck, norm1 / norm2 stats, bottleneck stored activated?, dropout keep-mask or None
_LayerTape = namedtuple('_LayerTape', 'bott s1 s2 activated keep')


def _cols(t, c0):
    """Device address of column c0 of a row-major [M, ld] matrix."""
    return t.data_ptr() + 4 * c0


class _Tape:
    pass


def _bn(model_bn, X_ptr, ld, M, training, dev, st):
    """Fold one BatchNorm over rows of X[M][C]: returns stats[4][Cpad] = scale, shift, mean, invstd."""
    C = model_bn.num_features
    cp = (C + 3) // 4 * 4
    stats = torch.empty((4, cp), device=dev, dtype=F32)
    if training:
        ws = torch.empty(L.query('gnx_bn_workspace', M, C), device=dev, dtype=F32)
        sync = _bn_sync(model_bn, torch.device(dev))           # (the layer's persistent sync words: no memset node per call)
        L.call('gnx_bn_train_stats_sync', X_ptr, ld, M, C, L.ptr(model_bn.weight), L.ptr(model_bn.bias),
               L.ptr(model_bn.running_mean), L.ptr(model_bn.running_var),
               L.ptr(model_bn.num_batches_tracked, torch.int64), float(model_bn.momentum), float(model_bn.eps),
               L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(stats[2]), L.ptr(stats[3]), L.ptr(ws),
               sync.data_ptr() if sync is not None else None, st)
    else:
        L.call('gnx_bn_fold_eval', C, L.ptr(model_bn.weight), L.ptr(model_bn.bias), L.ptr(model_bn.running_mean),
               L.ptr(model_bn.running_var), float(model_bn.eps), L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(stats[2]),
               L.ptr(stats[3]), st)
    return stats


def relayout_weights(model, kind, dev, st):
    """{weight: re-laid-out copy} for every conv weight of one kind (0: conv2 -> [tap][N][K], 1: conv2 -> [8 - tap][K][N] for
    the data gradient, 2: conv1 / transition conv -> [K][N]) in ONE launch (`gnx_relayout_weights_batch`; a training step
    needs all three after every optimizer step - 3 x 58 small launches otherwise).  Destinations and the device-side pointer
    table persist with the model (rebuilt when a weight's storage moves); the CONTENT is refreshed by every call."""
    if kind == 2:
        weights = [l.conv1.weight for l in model._layers] + [t.conv.weight for t in model._transitions]
    else:
        weights = [l.conv2.weight for l in model._layers]
    key = (str(dev),) + tuple(w.data_ptr() for w in weights)
    plans = model.__dict__.setdefault('_relayout_plans', {})
    hit = plans.get(kind)
    if hit is None or hit[0] != key:
        dsts, rows = {}, []
        for w in weights:
            # the device table holds RAW pointers read as dense fp32 [N][K][taps]: anything else (channels_last weights
            # after model.to(memory_format=...), half weights) would be re-laid-out silently wrong
            if not (w.is_contiguous() and w.dtype == F32):
                raise TypeError("gridnext_amd.DenseNet: conv weights must be contiguous float32 (got %s, strides %s)"
                                % (w.dtype, tuple(w.stride())))
            n, k = w.shape[0], w.shape[1]
            shape = (9, n, k) if kind == 0 else ((9, k, n) if kind == 1 else (k, n))
            d = torch.empty(shape, device=dev, dtype=F32)
            dsts[w] = d
            rows.append(struct.pack('<QQii', w.data_ptr(), d.data_ptr(), n, k))
        table = torch.frombuffer(bytearray(b''.join(rows)), dtype=torch.uint8).to(dev)
        hit = plans[kind] = (key, dsts, table, len(weights))
    L.call('gnx_relayout_weights_batch', hit[2].data_ptr(), hit[3], kind, st)
    return hit[1]


def gammas_nonzero(model):
    """True when no norm2 (and norm0) weight of the network is exactly zero (the activated-bottleneck form of the training
    forward cannot recover x_hat where gamma == 0).  One device reduction and one host read per change of those weights: the
    answer is cached with the model's other derived tensors, keyed on the weights' versions."""
    ws = [l.norm2.weight for l in model._layers]
    if hasattr(model.features, 'norm0'):
        ws.append(model.features.norm0.weight)       # pool0's adjoint reads norm0's mask and x_hat off the pooled map
    return model._cached('g2nz', model._key(ws), lambda: bool((torch.cat([t.detach().reshape(-1) for t in ws]) != 0).all().item()))


def _dropout_keep(model, index, rows, cols, dev):
    """Keep-mask [rows][cols] (bool) of dense layer `index`'s dropout: Bernoulli(1 - p) from torch's device generator (Philox;
    graph-capture safe), or whatever the test hook `model._dropout_mask` returns."""
    if model._dropout_mask is not None:
        return model._dropout_mask(index, rows, cols, dev)
    return torch.rand((rows, cols), device=dev) >= model.drop_rate


# ------------------------------------------------------------------ shared by both taped forwards and all three backwards
def _versions(params):
    return [(p, p._version, p.data_ptr()) for p in params]


def _check_tape(tape, consequence):
    """A backward's guard: its forward's `tape` (None once a backward consumed it) must still match the live parameters,
    whose values the backward re-reads."""
    if tape is None:
        raise RuntimeError("gridnext_amd.DenseNet: the tape of this forward was already consumed (a second backward / "
                           "retain_graph=True is not supported: run the forward again)")
    for p, ver, addr in tape.versions:
        if p._version != ver or p.data_ptr() != addr:
            raise RuntimeError("gridnext_amd.DenseNet: a parameter was modified between forward and backward "
                               "(optimizer.step() or load_state_dict before loss.backward()); " + consequence)


def _finish_forward(ctx, model, tape, feats, params, st):
    """Last step of a taped forward: the tape keeps the pooled features and which parameter values were used; returns the
    fp32 classifier's logits (a copy of the features where the network has no classifier)."""
    tape.feats = feats
    tape.versions = _versions(params)
    ctx.tape, ctx.model = tape, model
    if not model.classify:
        return feats.clone()
    N, c, nc = feats.shape[0], model.num_features, model.classifier.out_features
    out = torch.empty((N, nc), device=feats.device, dtype=F32)
    L.call('gnx_gemm_f32', L.ptr(feats), c, 0, L.ptr(model.classifier.weight), c, 0, L.ptr(model.classifier.bias),
           L.ptr(out), nc, N, nc, c, 0, st)
    return out


class _Grads:
    """The parameter gradients of one backward, in the order it makes them.  Data-parallel runs: `bucket()` after each stage
    hands what was made since the last one to a distributed.BackwardReducer, whose all-reduce overlaps the rest of the
    backward; what autograd receives is already the average over ranks."""

    def __init__(self, input_only=False):
        from . import distributed as gdist
        self.made, self.sent = {}, 0
        # input_only (utils.patch_saliency): no parameter wants a gradient, whatever its requires_grad says - none is formed,
        # none is handed to a reducer, and the step's delivery mode is not decided by this backward
        self.input_only = input_only
        self.reducer = None
        if input_only:
            return
        self.reducer = gdist.BackwardReducer() if gdist.BackwardReducer.wanted() else None
        if gdist.is_active():
            gdist.note_backward(self.reducer is not None)     # (all backwards of one optimizer step must deliver alike)

    def want(self, p):
        return p is not None and p.requires_grad and not self.input_only

    def new(self, p):
        t = self.made[p] = torch.empty_like(p, memory_format=torch.contiguous_format)
        return t

    def bn(self, bn):
        """(dgamma, dbeta) of a BatchNorm, None for a frozen one."""
        return tuple(self.new(p) if self.want(p) else None for p in (bn.weight, bn.bias))

    def bucket(self):
        if self.reducer is not None:
            ps = list(self.made)[self.sent:]
            self.sent += len(ps)
            self.reducer.bucket([self.made[p] for p in ps], ps)

    def result(self, model, dx=None):
        """autograd's tuple: None for the model, the input's gradient `dx` (None where it asked for none), then one gradient
        (or None) per parameter."""
        if self.reducer is not None:
            self.bucket()
            self.reducer.finish()
        return (None, dx) + tuple(self.made.get(p) for p in model.parameters())


def _classifier_backward(model, grads, dout, feats, st):
    """The fp32 classifier's parameter gradients; returns the gradient of the pooled features (dout without a classifier)."""
    if not model.classify:
        return dout
    cls, c = model.classifier, model.num_features
    N, nc = dout.shape[0], cls.out_features
    dfeats = torch.empty((N, c), device=dout.device, dtype=F32)
    L.call('gnx_gemm_f32', L.ptr(dout), nc, 0, L.ptr(cls.weight), c, 1, None, L.ptr(dfeats), c, N, c, nc, 0, st)
    if grads.want(cls.weight):
        L.call('gnx_gemm_f32', L.ptr(dout), nc, 1, L.ptr(feats), c, 1, None, L.ptr(grads.new(cls.weight)), c, nc, c, N, 0, st)
    if grads.want(cls.bias):
        db = grads.new(cls.bias)
        ws = torch.empty(L.query('gnx_bn_workspace', N, nc), device=dout.device, dtype=F32)
        L.call('gnx_colsum', L.ptr(dout), nc, N, nc, L.ptr(db), 0, L.ptr(ws), st)
    return dfeats


# ------------------------------------------------------------------ fp32 taped forward
def _stem_taped(model, tape, x, buf, st):
    """conv0 (-> norm0 -> relu0 -> pool0) of the taped forward into the first block buffer `buf`.  The tape gets norm0's
    folded stats0, pool_idx - which window element won, one byte per pooled element: pool0's adjoint routes by it, ties
    exactly as torch's max_pool2d - and stem_out, the conv0 map, kept only where the backward needs it."""
    N, _, P, _ = x.shape
    dev, hs, training = x.device, tape.hs, tape.training
    conv0 = model.features.conv0
    c0, ld = conv0.out_channels, buf.shape[1]
    w0 = conv0.weight.detach().contiguous()
    tape.stats0 = tape.pool_idx = tape.stem_out = None
    if model.small_inputs:
        L.call('gnx_conv_stem', L.ptr(x), L.ptr(w0), L.ptr(buf), ld, N, 3, P, P, c0, 3, 3, 1, 1, st)
        return
    norm0, M0, hp = model.features.norm0, N * hs * hs, (hs + 2 - 3) // 2 + 1
    # Running statistics (training.py:126 keeps f in eval mode) and window indices: the backward reads mask and x_hat off the
    # pooled map in block 1's buffer, and the conv0 map (5.2 GB for a 128-px array) is not kept
    pooled_bwd = not training and c0 % 4 == 0 and ld % 4 == 0 and gammas_nonzero(model)
    if pooled_bwd:
        # norm0's map is known before conv0 runs, so stem, norm0, relu0 and pool0 are the eval forward's ONE kernel, which also
        # records the window indices: the conv0 map is never written
        s0 = tape.stats0 = _bn(norm0, None, c0, M0, False, dev, st)
        tape.pool_idx = torch.empty((N * hp * hp, c0), device=dev, dtype=torch.uint8)
        if L.try_call('gnx_conv_stem_bnrelu_maxpool_argmax', L.ptr(x), L.ptr(w0), L.ptr(buf), ld, tape.pool_idx.data_ptr(),
                      N, 3, P, P, c0, 7, 7, 2, 3, L.ptr(s0[0]), L.ptr(s0[1]), st):
            return
    stem_out = torch.empty((M0, c0), device=dev, dtype=F32)
    L.call('gnx_conv_stem', L.ptr(x), L.ptr(w0), L.ptr(stem_out), c0, N, 3, P, P, c0, 7, 7, 2, 3, st)
    s0 = tape.stats0 = _bn(norm0, L.ptr(stem_out), c0, M0, training, dev, st)
    if c0 % 4 == 0:
        if tape.pool_idx is None:                          # (a fused stem that declined the shapes left one)
            tape.pool_idx = torch.empty((N * hp * hp, c0), device=dev, dtype=torch.uint8)
        L.call('gnx_bnrelu_maxpool_argmax', L.ptr(stem_out), c0, L.ptr(buf), ld, tape.pool_idx.data_ptr(), N, c0, hs, hs,
               L.ptr(s0[0]), L.ptr(s0[1]), st)
    else:
        L.call('gnx_bnrelu_maxpool', L.ptr(stem_out), c0, L.ptr(buf), ld, N, c0, hs, hs, L.ptr(s0[0]), L.ptr(s0[1]), st)
    if not pooled_bwd:
        tape.stem_out = stem_out


class _DenseNetFn(Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        x = model._unit_floats(x)       # uint8 patches: ToTensor (+ Normalize) as one pass (conv0's wgrad re-reads floats)
        N, _, P, _ = x.shape
        dev = x.device
        st = L.stream()
        training = model.training
        hs, sizes = model._geometry(P)
        mid = model.bn_size * model.growth_rate
        g = model.growth_rate
        tape = _Tape()
        tape.x, tape.N, tape.P, tape.hs, tape.sizes, tape.training = x, N, P, hs, sizes, training
        bufs = [torch.empty((N * s * s, c_total), device=dev, dtype=F32)
                for (_, _, _, c_total), s in zip(model._blocks, sizes)]
        tape.bufs = bufs
        _stem_taped(model, tape, x, bufs[0], st)
        w2r = relayout_weights(model, 0, dev, st)            # conv2 weights tap-major, all layers, one launch
        tape.layers = []          # per block: one _LayerTape per layer
        act_ok = (not training) and gammas_nonzero(model)
        w2u = model._winograd_conv2() if (act_ok and model.winograd and model.mfma == 'f32') else None
        split_ok = act_ok and model.mfma == 'f32' and mid == 128
        w1s = model._split_conv1() if (split_ok and model.split_conv1) else None
        w2s = model._split_conv2() if (split_ok and model.split_conv2 and g == 32) else None
        tape.trans = []           # per block: stats of the transition BN (or None)
        n_drop = 0
        for bi, ((c_in, layers, trans, c_total), s) in enumerate(zip(model._blocks, sizes)):
            buf = bufs[bi]
            M = N * s * s
            recs = []
            for li, layer in enumerate(layers):
                cin = c_in + li * g
                s1 = _bn(layer.norm1, L.ptr(buf), c_total, M, training, dev, st)
                bott = torch.empty((M, mid), device=dev, dtype=F32)
                # Eval statistics (training.py:126 puts f in eval mode even when it is trained): norm2's affine map is known
                # before conv1 runs, so the bottleneck is stored ACTIVATED - conv2 then runs its prologue-free LDS-DMA
                # form and its weight gradient needs no prologue; the BN adjoint recovers mask and
                # x_hat from the activated values (needs scale != 0, i.e. gamma != 0, checked once per layer).
                activated = act_ok
                if activated:
                    s2 = _bn(layer.norm2, None, mid, M, False, dev, st)
                    # conv1 and conv2 as in the eval forward, the (opt-in) split and Winograd forms included.  The backward
                    # differentiates the same function on the fp32 instruction, the adjoint of whichever conv2 ran (masks and
                    # x_hat come from the stored activations).  Against a direct-form reference the outputs differ at rounding
                    # level; only a pre-activation that a reference computes as EXACTLY 0 (closed-form nets with integer
                    # weights) can flip a ReLU mask of the next layer - such tests set `model.winograd = False`.
                    dense_layer_f32_act(model, layer, buf, c_total, cin, bott, M, s, s1, s2, w2r[layer.conv2.weight], w1s, w2s,
                                        w2u, st)
                else:
                    nws = L.query('gnx_conv1x1_workspace', M, mid, cin)       # small batches: K split over workgroups
                    ws1 = torch.empty(nws, device=dev, dtype=F32) if nws else None
                    L.call('gnx_conv1x1_bnrelu_ws', L.ptr(buf), c_total, L.ptr(layer.conv1.weight), L.ptr(bott), mid, M, mid,
                           cin, L.ptr(s1[0]), L.ptr(s1[1]), L.ptr(ws1), st)
                    s2 = _bn(layer.norm2, L.ptr(bott), mid, M, training, dev, st)
                    L.call('gnx_conv3x3_bnrelu', L.ptr(bott), mid, L.ptr(w2r[layer.conv2.weight]), _cols(buf, cin), c_total, M,
                           g, mid, s, L.ptr(s2[0]), L.ptr(s2[1]), st)
                keep = None
                if training and model.drop_rate > 0:
                    # F.dropout(new_features, p, training) (densenet.py:42-43): the layer's 32 new columns times a keep-mask
                    # / (1 - p), in place in the block buffer - later layers read the dropped features, as after the
                    # reference's concatenation; the backward applies the same factor to the columns' gradient
                    keep = _dropout_keep(model, n_drop, M, g, dev)
                    n_drop += 1
                    buf[:, cin:cin + g].mul_(keep.to(F32).mul_(1.0 / (1.0 - model.drop_rate)))
                recs.append(_LayerTape(bott, s1, s2, activated, keep))
            tape.layers.append(recs)
            if trans is not None:
                nxt = bufs[bi + 1]
                so = s // 2
                stt = _bn(trans.norm, L.ptr(buf), c_total, M, training, dev, st)
                L.call('gnx_conv1x1_bnrelu', L.ptr(buf), c_total, L.ptr(trans.conv.weight), L.ptr(nxt), nxt.shape[1],
                       N * so * so, trans.conv.out_channels, c_total, L.ptr(stt[0]), L.ptr(stt[1]), 1, s, st)
                tape.trans.append(stt)
            else:
                tape.trans.append(None)
        s_last = sizes[-1]
        c_last = model.num_features
        sf = _bn(model.features.norm_final, L.ptr(bufs[-1]), bufs[-1].shape[1], N * s_last * s_last, training, dev, st)
        tape.statsf = sf
        feats = torch.empty((N, c_last), device=dev, dtype=F32)
        L.call('gnx_bnrelu_avgpool', L.ptr(bufs[-1]), bufs[-1].shape[1], L.ptr(feats), c_last, N, c_last,
               s_last * s_last, L.ptr(sf[0]), L.ptr(sf[1]), st)
        if training:
            model.invalidate_cache()      # running statistics were updated through raw pointers (no _version bump)
        ctx.x_needs_grad = ctx.needs_input_grad[1]            # (not x.requires_grad: `x` may be _unit_floats' copy by now)
        return _finish_forward(ctx, model, tape, feats, params, st)

    @staticmethod
    def backward(ctx, dout):
        tape = ctx.tape
        _check_tape(tape, "its gradient would be computed from the new value")
        model = ctx.model
        dout = dout.contiguous()
        b = _Backward(model, tape, dout.device)
        grads, N = b.grads, tape.N
        bufs, dbufs = tape.bufs, [None] * len(tape.bufs)
        dbufs[-1] = b.tail(_classifier_backward(model, grads, dout, tape.feats, b.st))
        for bi in range(len(model._blocks) - 1, -1, -1):
            _, layers, _, c_total = model._blocks[bi]
            M = N * tape.sizes[bi] ** 2
            tA = torch.empty((M, b.mid), device=b.dev, dtype=F32)
            tB = torch.empty((M, b.mid), device=b.dev, dtype=F32) if b.defer is None else None    # (deferred: one per layer)
            tC = torch.empty((M, c_total), device=b.dev, dtype=F32)
            for li in range(len(layers) - 1, -1, -1):
                b.layer(bi, li, dbufs[bi], tA, tB, tC)
                tape.layers[bi][li] = None
            if b.defer is not None:
                b.defer.flush(b.wgrad_batch)                   # this block's weight gradients: one branch on the side stream
            del tA, tB, tC
            if bi > 0:
                dbufs[bi - 1] = b.transition(bi, dbufs[bi])
                dbufs[bi] = None
                bufs[bi] = None
            grads.bucket()                                         # this block (+ the transition below it): final
        dX = b.stem(dbufs[0], ctx.x_needs_grad)
        if b.defer is not None:
            b.defer.join()
        ctx.tape = None
        return grads.result(model, dX)


class _DeferredWgrads:
    """Under hipGraph capture (the spot loop's small-batch steps, graphs.py) a dense block's weight gradients are DEFERRED to
    the end of the block and launched on a side stream as ONE parallel branch of the step graph: they are off the critical
    path (the data-gradient chain), and at a batch of 32 patches every kernel leaves most of the chip idle, so the branch
    runs beside the next block's chain.  One fork per block, one join at the end: 2 514 -> 2 577 spots/s in the same run
    (a fork / join per LAYER cost more than it gave: 2 369 against 2 505; branches of 2, 4 or 8 layers: the same +2 %).
    Each layer then keeps its own gradient-of-bottleneck buffer until the join."""

    def __init__(self, model, dev):
        side = model.__dict__.get('_wgrad_stream')
        if side is None or side.device != dev:
            side = model.__dict__['_wgrad_stream'] = torch.cuda.Stream(device=dev)
        self.side, self.cur = side, torch.cuda.current_stream(dev)
        self.items = []           # this block's _Wgrad items
        self.held = []            # what their kernels read, alive until the join: per layer bottleneck, stats, tB, buffers
        self.done = []            # one event per flushed block

    def flush(self, run):
        """Fork after everything launched so far: `run(items)` launches the block's weight gradients on the side stream."""
        if not self.items:
            return
        ev = torch.cuda.Event()
        ev.record(self.cur)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            run(self.items)
        self.items = []
        done = torch.cuda.Event()
        done.record(self.side)
        self.done.append(done)

    def join(self):
        for ev in self.done:
            self.cur.wait_event(ev)
        self.held.clear()


class _Backward:
    """The stages of one fp32 backward on the tape of its forward: tail, dense layer, transition, stem.  Weight gradients run
    on the current stream (`L.stream()`: the side stream inside a flush of `defer`), everything else on `st`."""

    def __init__(self, model, tape, dev):
        self.model, self.tape, self.dev, self.st = model, tape, dev, L.stream()
        self.training, self.g, self.mid = tape.training, model.growth_rate, model.bn_size * model.growth_rate
        self.defer = _DeferredWgrads(model, dev) if torch.cuda.is_current_stream_capturing() else None
        self.grads = _Grads(model.__dict__.get('_input_grad_only', False))
        self.w2b = relayout_weights(model, 1, dev, self.st)   # conv2 weights for the data gradient, all layers, one launch
        self.w1t = relayout_weights(model, 2, dev, self.st)   # conv1 / transition weights transposed, one launch

    def bn_bwd(self, bn, stats, dy_ptr, lddy, x_ptr, ldx, dx_ptr, lddx, M, C, dx_acc, relu=1):
        dg, db = self.grads.bn(bn)
        ws = torch.empty(L.query('gnx_bn_workspace', M, C), device=self.dev, dtype=F32)
        sync = _bn_sync(bn, torch.device(self.dev))
        L.call('gnx_bn_relu_bwd_sync', dy_ptr, lddy, x_ptr, ldx, dx_ptr, lddx, M, C, L.ptr(stats[0]), L.ptr(stats[1]),
               L.ptr(stats[2]), L.ptr(stats[3]), L.ptr(dg), L.ptr(db), relu, 1 if self.training else 0, 0, dx_acc,
               L.ptr(ws), sync.data_ptr() if sync is not None else None, self.st)

    def wgrad(self, c):
        model = self.model
        w, dy_ptr, lddy, x_ptr, ldx, stats, M, Nn, K, S, taps, pool = c
        if not self.grads.want(w):
            return
        dw = self.grads.new(w)
        sc, sh = (L.ptr(stats[0]), L.ptr(stats[1])) if stats is not None else (None, None)
        if model.split_wgrad and taps == 1 and not pool and Nn % 4 == 0 and K % 4 == 0:
            # (opt-in) the same contraction on split bf16 operands: HBM-bound instead of bound by the fp32 matrix instruction
            t0 = model._probe_begin()
            ws = torch.empty(L.query('gnx_wgrad1x1_split_workspace', M, Nn, K), device=self.dev, dtype=F32)
            if L.try_call('gnx_wgrad1x1_split', dy_ptr, lddy, x_ptr, ldx, sc, sh, L.ptr(dw), L.ptr(ws), M, Nn, K, 0, L.stream()):
                model._probe_mark('wgrad1x1', t0, 2 * M * Nn * K, 4 * M * (Nn + K))
                return
        if model.split_wgrad and taps == 9 and stats is None and Nn == 32 and K == 128 and S >= 8:
            # (opt-in) conv2's weight gradient from the activated bottleneck, same arithmetic (4 x 4 maps: the fp32 kernel is faster)
            t0 = model._probe_begin()
            ws = torch.empty(L.query('gnx_wgrad3x3_split_workspace', M), device=self.dev, dtype=F32)
            if L.try_call('gnx_wgrad3x3_split', dy_ptr, lddy, x_ptr, ldx, L.ptr(dw), L.ptr(ws), M, S, 0, L.stream()):
                model._probe_mark('wgrad3x3', t0, 2 * M * 9 * Nn * K, 4 * M * (Nn + K))
                return
        ws = torch.empty(L.query('gnx_wgrad_workspace', M, Nn, K, taps), device=self.dev, dtype=F32)
        t0 = model._probe_begin()
        L.call('gnx_wgrad_bnrelu', dy_ptr, lddy, x_ptr, ldx, sc, sh, L.ptr(dw), L.ptr(ws), M, Nn, K, S, taps, pool, 0,
               L.stream())
        model._probe_mark('wgrad3x3' if taps == 9 else ('wgrad_trans' if pool else 'wgrad1x1'), t0, 2 * M * taps * Nn * K,
                          4 * M * (Nn + K * (4 if pool else 1)))

    def wgrad_or_defer(self, c):
        if self.defer is None:
            self.wgrad(c)
        else:
            self.defer.items.append(c)

    def wgrad_batch(self, items):
        """A dense block's deferred weight gradients.  Items of one kind go out as ONE launch per 24 layers plus one batched
        reduce (gnx_wgrad_bnrelu_batch: the same kernel bodies, slab layout and reduce order - bit-identical to the single
        calls); whatever that entry point does not take is made one by one."""
        grads = self.grads
        for taps in (9, 1):
            batch = [c for c in items if c.taps == taps and c.pool == 0 and grads.want(c.w) and
                     (taps == 9 or (c.K > 128 and c.K % 4 == 0 and c.N % 128 == 0))]    # (K <= 128 runs another kernel: singly)
            if len(batch) < 2:
                continue
            arr = (L.struct('gnx_wgrad_item') * len(batch))()      # one weight gradient of the batch each
            outs = []
            for a, c in zip(arr, batch):
                dw = torch.empty_like(c.w, memory_format=torch.contiguous_format)
                ws = torch.empty(L.query('gnx_wgrad_workspace', c.M, c.N, c.K, taps), device=self.dev, dtype=F32)
                outs.append((dw, ws))
                a.dY, a.lddy, a.X, a.ldx = c.dy, c.lddy, c.x, c.ldx
                a.scale, a.shift = (L.ptr(c.stats[0]), L.ptr(c.stats[1])) if c.stats is not None else (None, None)
                a.dW, a.workspace, a.M, a.N, a.K, a.S, a.accumulate = L.ptr(dw), L.ptr(ws), c.M, c.N, c.K, c.S, 0
            # batched items never take the opt-in split_wgrad kernels, so a captured step ignores that flag
            if L.try_call('gnx_wgrad_bnrelu_batch', ctypes.addressof(arr), len(batch), taps, L.stream()):
                for c, (dw, _) in zip(batch, outs):
                    grads.made[c.w] = dw
                batched = {id(c) for c in batch}
                items = [c for c in items if id(c) not in batched]
        for c in items:
            self.wgrad(c)

    def tail(self, dfeats):
        """norm_final -> relu -> global average; returns the last block's gradient."""
        model, tape = self.model, self.tape
        x, c, s = tape.bufs[-1], model.num_features, tape.sizes[-1]
        M = tape.N * s * s
        dY = torch.empty((M, c), device=self.dev, dtype=F32)
        L.call('gnx_rows_broadcast', L.ptr(dfeats), c, L.ptr(dY), c, tape.N, c, s * s, 1.0 / (s * s), self.st)
        dx = torch.empty_like(x)
        self.bn_bwd(model.features.norm_final, tape.statsf, L.ptr(dY), c, L.ptr(x), x.shape[1], L.ptr(dx), x.shape[1], M, c, 0)
        return dx

    def layer(self, bi, li, dbuf, tA, tB, tC):
        """Dense layer li of block bi: its parameter gradients, and its input's gradient accumulated into the block gradient
        `dbuf`.  tA, tB, tC: the block's scratch, [M][mid], [M][mid] (None under capture) and [M][c_total]."""
        model, st = self.model, self.st
        c_in, layers, _, c_total = model._blocks[bi]
        layer, buf, s = layers[li], self.tape.bufs[bi], self.tape.sizes[bi]
        M, g, mid = self.tape.N * s * s, self.g, self.mid
        cin = c_in + li * g
        bott, s1, s2, activated, keep = self.tape.layers[bi][li]
        if keep is not None:                                   # dropout's adjoint on this layer's gradient columns
            dbuf[:, cin:cin + g].mul_(keep.to(F32).mul_(1.0 / (1.0 - model.drop_rate)))
        dy2 = _cols(dbuf, cin)
        if self.defer is not None:
            tB = torch.empty((M, mid), device=self.dev, dtype=F32)      # this layer's own: read by its deferred wgrad
            self.defer.held.append((bott, s1, s2, tB, buf, dbuf))
        # conv2: weight gradient (no prologue when the bottleneck was stored activated), then data gradient (adjoint conv with
        # flipped taps) and norm2 -> relu2's adjoint: ONE kernel where the bottleneck was stored activated (eval statistics)
        # and the shape is the LDS-DMA kernel's; otherwise the product, then the adjoint pass
        self.wgrad_or_defer(_Wgrad(layer.conv2.weight, dy2, c_total, L.ptr(bott), mid, None if activated else s2, M, g, mid, s,
                                   9, 0))
        wb = self.w2b[layer.conv2.weight]
        if not (activated and self.dgrad3x3_bn2(layer, dy2, c_total, wb, bott, tB, M, s, s2)):
            t0 = model._probe_begin()
            L.call('gnx_conv3x3_bnrelu', dy2, c_total, L.ptr(wb), L.ptr(tA), mid, M, mid, g, s, None, None, st)
            t0 = model._probe_mark('dgrad3x3', t0, 2 * M * 9 * mid * g, 4 * M * (g + mid))
            self.bn_bwd(layer.norm2, s2, L.ptr(tA), mid, L.ptr(bott), mid, L.ptr(tB), mid, M, mid, 0, relu=2 if activated else 1)
            model._probe_mark('bn2_bwd', t0, 0, 4 * M * 3 * mid)
        # conv1: the opt-in one-pass form, else its weight gradient and then the data gradient + norm1 -> relu1 adjoint into
        # the block gradient (one kernel under running statistics where the tiles are whole: 3 passes over [M][cin] instead
        # of 5), else the product and the adjoint pass
        w1t = self.w1t[layer.conv1.weight]
        fused = (not self.training and self.defer is None and mid == 128 and cin % 32 == 0 and M % 32 == 0 and
                 self.grads.want(layer.conv1.weight) and model.__dict__.get('fused_conv1_backward', False))
        if not (fused and self.conv1_dgrad_wgrad_bn1(layer, tB, w1t, buf, dbuf, c_total, M, cin, s1)):
            self.wgrad_or_defer(_Wgrad(layer.conv1.weight, L.ptr(tB), mid, L.ptr(buf), c_total, s1, M, mid, cin, s, 1, 0))
            if self.training or not self.conv1_dgrad_bn1(layer, tB, w1t, buf, dbuf, c_total, M, cin, s1):
                L.call('gnx_conv1x1_bnrelu', L.ptr(tB), mid, L.ptr(w1t), L.ptr(tC), c_total, M, cin, mid, None, None, 0, 0, st)
                self.bn_bwd(layer.norm1, s1, L.ptr(tC), c_total, L.ptr(buf), c_total, L.ptr(dbuf), c_total, M, cin, 1)

    def dgrad3x3_bn2(self, layer, dy2, lddy, wb, bott, dB, M, s, s2):
        """conv2's data gradient and norm2 -> relu2's adjoint in one kernel; False where it declines the shapes."""
        model, mid, g = self.model, self.mid, self.g
        dg, db = self.grads.bn(layer.norm2)
        ws = torch.empty(L.query('gnx_conv3x3_dgrad_bn_workspace', M, mid), device=self.dev, dtype=F32)
        t0 = model._probe_begin()
        if not L.try_call('gnx_conv3x3_dgrad_bnrelu_bwd', dy2, lddy, L.ptr(wb), L.ptr(bott), mid, L.ptr(dB), mid, M, mid, g, s,
                          L.ptr(s2[0]), L.ptr(s2[1]), L.ptr(s2[2]), L.ptr(s2[3]), L.ptr(dg), L.ptr(db), 0, L.ptr(ws), self.st):
            return False
        model._probe_mark('dgrad3x3_bn2', t0, 2 * M * 9 * mid * g, 4 * M * (g + 2 * mid))
        return True

    def conv1_dgrad_wgrad_bn1(self, layer, dB, w1t, buf, dbuf, ld, M, cin, s1):
        """Optional (`model.fused_conv1_backward = True`): data gradient + norm1/relu1 adjoint into the block gradient AND the
        weight gradient from the same staged tiles, ONE pass over dB, X and G (gnx_conv1x1_dgrad_wgrad_bnrelu_bwd).  Not the
        default: with both products the fp32 pass is bound by the matrix pipe at ~100 TFLOP/s (93 ms per 128-px array) - the
        same time as the two separate passes it replaces (50 + 42 ms); on the fp16 path, where the matrix
        work is 16x cheaper, the same fusion is the default (densenet_train_f16)."""
        model, mid = self.model, self.mid
        dg, db = self.grads.bn(layer.norm1)
        ws = torch.empty(L.query('gnx_conv1x1_dgrad_wgrad_workspace', M, cin), device=self.dev, dtype=F32)
        dw = self.grads.new(layer.conv1.weight)
        t0 = model._probe_begin()
        if not L.try_call('gnx_conv1x1_dgrad_wgrad_bnrelu_bwd', L.ptr(dB), mid, L.ptr(w1t), L.ptr(buf), ld, L.ptr(dbuf), ld, M,
                          cin, L.ptr(s1[0]), L.ptr(s1[1]), L.ptr(s1[2]), L.ptr(s1[3]), L.ptr(dg), L.ptr(db), L.ptr(dw),
                          L.ptr(ws), 0, self.st):
            return False
        model._probe_mark('dgrad_wgrad1x1_bn1', t0, 4 * M * cin * mid, 4 * M * (mid + 3 * cin))
        return True

    def conv1_dgrad_bn1(self, layer, dB, w1t, buf, dbuf, ld, M, cin, s1):
        """conv1's data gradient and norm1 -> relu1's adjoint (running statistics) in one kernel, or False."""
        model, mid = self.model, self.mid
        dg, db = self.grads.bn(layer.norm1)
        ws = torch.empty(L.query('gnx_conv1x1_dgrad_bn_workspace', M, cin), device=self.dev, dtype=F32)
        t0 = model._probe_begin()
        if not L.try_call('gnx_conv1x1_dgrad_bnrelu_bwd', L.ptr(dB), mid, L.ptr(w1t), L.ptr(buf), ld, L.ptr(dbuf), ld, M, cin,
                          mid, L.ptr(s1[0]), L.ptr(s1[1]), L.ptr(s1[2]), L.ptr(s1[3]), L.ptr(dg), L.ptr(db), 0, L.ptr(ws),
                          self.st):
            return False
        model._probe_mark('dgrad1x1_bn1', t0, 2 * M * cin * mid, 4 * M * (mid + 3 * cin))
        return True

    def transition(self, bi, dbuf):
        """Transition bi-1 -> bi from block bi's gradient `dbuf` (its columns [0, c_out)); returns block bi-1's gradient."""
        model, tape, st = self.model, self.tape, self.st
        _, _, trans, ld = model._blocks[bi - 1]
        c_total = model._blocks[bi][3]
        N, ps, c_out = tape.N, tape.sizes[bi - 1], trans.conv.out_channels
        M, Mp = N * tape.sizes[bi] ** 2, N * ps * ps
        x, stt, w = tape.bufs[bi - 1], tape.trans[bi - 1], trans.conv.weight
        # weight gradient: with eval statistics the pooled, activated input is built once (one 16-B pass) and the plain 1x1
        # weight-gradient kernel runs on a quarter of the rows; the in-kernel pooling form otherwise
        if not (self.grads.want(w) and not self.training and self.wgrad_pooled(w, dbuf, c_total, x, stt, M, c_out, ps)):
            self.wgrad(_Wgrad(w, L.ptr(dbuf), c_total, L.ptr(x), ld, stt, M, c_out, ld, ps, 1, 1))
        dPool = torch.empty((M, ld), device=self.dev, dtype=F32)
        L.call('gnx_conv1x1_bnrelu', L.ptr(dbuf), c_total, L.ptr(self.w1t[w]), L.ptr(dPool), ld, M, ld, c_out, None, None, 0, 0,
               st)
        dx = torch.empty_like(x)
        # norm -> relu adjoint straight from the POOLED gradient (eval statistics): the unpooled map - a full-size write and
        # read - is never built
        if self.training or not self.bn_bwd_pooled(trans.norm, stt, dPool, x, dx, ps):
            dAct = torch.empty((Mp, ld), device=self.dev, dtype=F32)
            L.call('gnx_avgpool2_bwd', L.ptr(dPool), ld, L.ptr(dAct), ld, N, ld, ps, st)
            self.bn_bwd(trans.norm, stt, L.ptr(dAct), ld, L.ptr(x), ld, L.ptr(dx), ld, Mp, ld, 0)
            del dAct
        del dPool
        return dx

    def wgrad_pooled(self, w, dbuf, lddy, x, stt, M, c_out, s):
        """A transition's weight gradient from its pooled activated input (running statistics), or False."""
        ld = x.shape[1]
        pooled = torch.empty((M, ld), device=self.dev, dtype=F32)
        if not L.try_call('gnx_bnrelu_avgpool2', L.ptr(x), ld, L.ptr(pooled), ld, self.tape.N, ld, s, L.ptr(stt[0]),
                          L.ptr(stt[1]), self.st):
            return False
        self.wgrad(_Wgrad(w, L.ptr(dbuf), lddy, L.ptr(pooled), ld, None, M, c_out, ld, 0, 1, 0))
        return True

    def bn_bwd_pooled(self, bn, stt, dPool, x, dx, s):
        """A transition's norm -> relu adjoint from the gradient of its pooled map (running statistics), or False."""
        N, ld = self.tape.N, x.shape[1]
        dg, db = self.grads.bn(bn)
        ws = torch.empty(L.query('gnx_bn_workspace', N * s * s, ld), device=self.dev, dtype=F32)
        return L.try_call('gnx_bn_relu_bwd_pooled', L.ptr(dPool), ld, L.ptr(x), ld, L.ptr(dx), ld, N, s, ld, L.ptr(stt[0]),
                          L.ptr(stt[1]), L.ptr(stt[2]), L.ptr(stt[3]), L.ptr(dg), L.ptr(db), 0, L.ptr(ws), self.st)

    def conv0_dgrad(self, dS_ptr, ldd, k, stride, pad):
        """The gradient of the float patches from the conv0 map's gradient (rows [N*hs*hs][c0], leading dimension ldd):
        conv0's adjoint in its input (gnx_conv0_dgrad), a fresh [N, 3, P, P] tensor, every element written."""
        model, tape = self.model, self.tape
        conv0 = model.features.conv0
        N, P, c0 = tape.N, tape.P, conv0.out_channels
        dX = torch.empty((N, 3, P, P), device=self.dev, dtype=F32)
        t0 = model._probe_begin()
        L.call('gnx_conv0_dgrad', dS_ptr, ldd, L.ptr(conv0.weight.detach().contiguous()), L.ptr(dX), N, P, P, c0, k, k, stride,
               pad, self.st)
        ho = (P + 2 * pad - k) // stride + 1
        model._probe_mark('conv0_dgrad', t0, 2 * N * ho * ho * c0 * 3 * k * k, 4 * N * (ho * ho * c0 + 3 * P * P))
        return dX

    def stem(self, dx, want_dx=False):
        """conv0 (-> norm0 -> relu0 -> pool0) from block 1's gradient `dx`: pool0's output gradient is its first c0 columns.
        `want_dx`: the input patches asked for a gradient - returns it (None otherwise, and nothing more is launched)."""
        model, tape, grads, st = self.model, self.tape, self.grads, self.st
        conv0 = model.features.conv0
        N, P, hs, c0, ld = tape.N, tape.P, tape.hs, conv0.out_channels, dx.shape[1]
        dw0 = grads.new(conv0.weight) if grads.want(conv0.weight) else None
        if model.small_inputs:
            if dw0 is not None:
                ws = torch.empty(L.query('gnx_conv0_wgrad_workspace', N, P, P, c0, 3, 3, 1, 1), device=self.dev, dtype=F32)
                L.call('gnx_conv0_wgrad', L.ptr(tape.x), L.ptr(dx), ld, L.ptr(dw0), L.ptr(ws), N, P, P, c0, 3, 3, 1, 1, 0, st)
            # no norm0 / pool0 here: block 1's first c0 gradient columns ARE the conv0 map's gradient
            return self.conv0_dgrad(L.ptr(dx), ld, 3, 1, 1) if want_dx else None
        norm0 = model.features.norm0
        want_norm0 = grads.want(norm0.weight) or grads.want(norm0.bias)
        if dw0 is None and not want_norm0 and not want_dx:
            return None
        s0, x0, M0 = tape.stats0, tape.bufs[0], N * hs * hs
        dS = torch.empty((M0, c0), device=self.dev, dtype=F32)
        # running statistics: pool0's adjoint carries norm0 -> relu0 with it (mask and x_hat from the pooled activated map in
        # block 1's buffer), the conv0 map is not read again
        if (tape.pool_idx is not None and not self.training and gammas_nonzero(model) and
                L.try_call('gnx_maxpool_bwd_argmax_bnrelu', tape.pool_idx.data_ptr(), L.ptr(dx), ld, L.ptr(x0), ld,
                           L.ptr(s0[0]), L.ptr(dS), c0, N, c0, hs, hs, st)):
            hp = (hs + 2 - 3) // 2 + 1
            # this launch only sums dgamma / dbeta (no dx).  Without an input gradient it is kept exactly as it was, also for
            # a frozen norm0 under a trained conv0 (launch parity with earlier versions); with one it runs where it has a taker
            if want_norm0 or not want_dx:
                self.bn_bwd(norm0, s0, L.ptr(dx), ld, L.ptr(x0), ld, None, c0, N * hp * hp, c0, 0, relu=2)
        else:
            if tape.stem_out is None:
                raise RuntimeError("the conv0 map was not kept and gnx_maxpool_bwd_argmax_bnrelu refused the shapes")
            dAct = torch.empty((M0, c0), device=self.dev, dtype=F32)
            if tape.pool_idx is not None:
                L.call('gnx_maxpool_bwd_argmax', tape.pool_idx.data_ptr(), L.ptr(dx), ld, L.ptr(dAct), c0, N, c0, hs, hs, st)
            else:
                L.call('gnx_maxpool_bwd', L.ptr(tape.stem_out), c0, L.ptr(x0), ld, L.ptr(dx), ld, L.ptr(dAct), c0, N, c0, hs, hs,
                       L.ptr(s0[0]), L.ptr(s0[1]), st)
            self.bn_bwd(norm0, s0, L.ptr(dAct), c0, L.ptr(tape.stem_out), c0, L.ptr(dS), c0, M0, c0, 0)
            del dAct
        if dw0 is not None:
            ws = torch.empty(L.query('gnx_conv0_wgrad_workspace', N, P, P, c0, 7, 7, 2, 3), device=self.dev, dtype=F32)
            L.call('gnx_conv0_wgrad', L.ptr(tape.x), L.ptr(dS), c0, L.ptr(dw0), L.ptr(ws), N, P, P, c0, 7, 7, 2, 3, 0, st)
        return self.conv0_dgrad(L.ptr(dS), c0, 7, 2, 3) if want_dx else None


def _taped(model, x):
    """The autograd node that runs this call: the fp16-MFMA tape + backward (densenet_train_f16) where `DenseNet.mfma = 'f16'`
    and the shapes / mode are the ones it takes, the fp32 one otherwise."""
    if model.mfma == 'f16':
        from . import densenet_train_f16 as f16
        if f16.eligible(model, x):
            return f16._DenseNetF16Fn
    return _DenseNetFn


class _RecomputeFn(Function):
    """The same forward WITHOUT a tape; the backward runs the taped forward again on the saved input chunk and then its
    backward - what `cp.checkpoint` around a chunk (/root/reference/gridnext/gridnet_models.py:88-104) and `efficient=True`
    (/root/reference/gridnext/densenet.py:12-18, :36-40) do in the reference.  Memory: only the chunk's INPUT lives between
    forward and backward; one tape exists at a time, inside backward.
    BatchNorm running statistics (train mode only): updated exactly ONCE per chunk - the recompute starts from the
    statistics the first forward started from, so it reproduces that forward bit for bit (the reference's reentrant
    checkpoint runs the update twice).  Parameter gradients are accumulated straight into `.grad` by the inner backward, as
    a reentrant checkpoint does; nothing is returned for them.  An input chunk that requires a gradient is recomputed as a
    leaf of its own, and that leaf's gradient is what the backward returns for it."""

    @staticmethod
    def forward(ctx, model, x, *params):
        ctx.x_needs_grad = ctx.needs_input_grad[1]
        tape = _Tape()            # (no tape proper: the chunk's input and what its recompute must start from)
        tape.x, tape.versions = x, _versions(params)
        # train-mode dropout: the recompute must draw the masks the first forward drew
        tape.rng = torch.cuda.get_rng_state(x.device) if (model.training and model.drop_rate > 0) else None
        tape.bn_state = _running_stats(model) if model.training else None
        ctx.tape, ctx.model = tape, model
        with torch.no_grad():
            out = _taped(model, x).apply(model, x, *params)     # its tape dies with this call
        return out

    @staticmethod
    def backward(ctx, dout):
        model, tape = ctx.model, ctx.tape
        _check_tape(tape, "the recomputed forward would differ from the one whose output the loss was computed from")
        x = tape.x
        after = None
        if tape.bn_state is not None:
            after = _running_stats(model)
            _running_stats(model, tape.bn_state)
        rng_now = None
        if tape.rng is not None:
            rng_now = torch.cuda.get_rng_state(x.device)
            torch.cuda.set_rng_state(tape.rng, x.device)
        leaf = x.detach().requires_grad_(ctx.x_needs_grad)
        with torch.enable_grad():
            out = _taped(model, leaf).apply(model, leaf, *list(model.parameters()))
        if rng_now is not None:
            torch.cuda.set_rng_state(rng_now, x.device)
        if after is not None:                                    # later chunks may have moved the statistics on: keep theirs
            _running_stats(model, after)
        torch.autograd.backward(out, dout)
        ctx.tape = None
        return (None, leaf.grad) + (None,) * len(list(model.parameters()))


def _running_stats(model, restore=None):
    """Copies of every BatchNorm's running statistics, [(bn, mean, var, count)]; given such a list, writes it back instead."""
    if restore is None:
        return [(m, m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()) for m in model._bn_modules()]
    for m, rm, rv, nb in restore:
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
        m.num_batches_tracked.copy_(nb)
    model.invalidate_cache()


def tape_bytes_per_spot(model, P):
    """HBM one spot holds on the tape of the f-trained forward, plus its share of the backward's scratch (bytes): block
    buffers, one bottleneck per dense layer, the largest block's gradient buffers, the float patch."""
    hs, sizes = model._geometry(P)
    mid = model.bn_size * model.growth_rate
    total, biggest = 0, 0
    for (c_in, layers, trans, c_total), s in zip(model._blocks, sizes):
        block = s * s * c_total
        total += block + len(layers) * s * s * mid
        biggest = max(biggest, 2 * block + 2 * s * s * mid)
    return 4 * (total + biggest + 3 * P * P)


def densenet_autograd(model, x):
    """Differentiable DenseNet forward (training-mode BN when model.training, running-stat BN otherwise).
    Memory control (the reference's `efficient=True` and chunk checkpointing): with `model.efficient`, or when the tape of
    the whole batch would exceed `model.tape_budget` bytes under running statistics (where chunks are independent), the
    batch goes through in chunks whose forward keeps no tape and whose backward recomputes it (`_RecomputeFn`)."""
    params = list(model.parameters())
    n = x.shape[0]
    fn = _taped(model, x)
    if fn is _DenseNetFn:
        per = tape_bytes_per_spot(model, x.shape[2])
    else:
        from .densenet_train_f16 import tape_bytes_per_spot as per_f16
        per = per_f16(model, x.shape[2])
    chunk = n
    budget = getattr(model, 'tape_budget', None)
    if not model.training and budget and per * n > budget:
        chunk = max(8, int(budget // per) // 8 * 8)
    if chunk >= n:
        if getattr(model, 'efficient', False):
            return _RecomputeFn.apply(model, x, *params)
        return fn.apply(model, x, *params)
    return torch.cat([_RecomputeFn.apply(model, x.narrow(0, s0, min(chunk, n - s0)), *params) for s0 in range(0, n, chunk)], 0)


def densenet_recompute(model, x):
    """One chunk, forward without tape, recompute in backward (GridNet.atonce_patch_limit on the gradient path).  With
    `input_resize` / `input_crop` set the chunk arrives as stored uint8 patches and is resized here, chunk by chunk."""
    if not x.is_cuda:
        raise RuntimeError("gridnext_amd.DenseNet runs on a HIP device only (input is on %s)" % x.device)
    if model._input_transform_set():
        x = model._transformed_input(x, True)
    return _RecomputeFn.apply(model, x.contiguous(), *list(model.parameters()))
