"""DenseNet-BC gradient path on the fp16-MFMA kernels (BASELINE config 5 with f trained).

`DenseNet.mfma = 'f16'` on the gradient path under running statistics - `train_gridwise` with `f_opt`
(/root/reference/gridnext/training.py:126 keeps f in eval mode, :164-171 steps it) - runs here: the taped forward of
/root/reference/gridnext/densenet.py:35-54 IS the eval forward of config 5, block by block the same function
(`DenseNet._block_f16`) - every dense layer ONE kernel on channel-blocked fp16 block buffers [c_total / 32][rows][32]
(gnx_dense_layer_f16_tape: the same kernel, bit for bit, which also copies the activated bottleneck tile it holds in the LDS
out as the tape, [4][rows][32] halves) - and the backward of csrc/dense_bwd_f16.hip runs on the SAME buffers (`_lb` entry
points: (ld, bs) addressing) - fp16 matrix operands and fp16 gradient tensors, fp32 accumulation, fp32 parameter gradients.
`_DenseNetF16Fn.backward` is a skeleton over the stages of `_BackwardF16`, as the fp32 node's over `densenet_train._Backward`.

Every fp16 gradient tensor holds s x the true gradient, s the power-of-two loss scale of `_LossScale` (chosen per backward on
the device, re-centred at every transition); every fp32 result is multiplied by 1/s (exact) where its partial sums are reduced.

The stem (conv0 .. pool0, 64 channels) runs on fp16 matrix operands too: the forward is the inference kernel writing block 1's
first channel blocks, the backward (gnx_stem_bwd_f16) one pass over the patches - no window indices, no fp32 conv0-map
gradient in HBM.  Other stem widths (and `model.f16_stem = False`) keep the fp32 stem with recorded window indices
(`_stem_f32_taped`) and its fp32 adjoints.  The classifier is fp32.
"""
import torch
from torch.autograd import Function

from . import _lib as L
from .densenet_train import _Grads, _Tape, _bn, _check_tape, _classifier_backward, _finish_forward, gammas_nonzero

F32, H16 = torch.float32, torch.float16


def eligible(model, x):
    """Shapes / modes the fp16 gradient path takes (else the fp32 path): the limits of gnx_dense_layer_f16_tape.  Not asked, unlike
    `DenseNet._eval_plan`: f16_buffers, f16_fused (no other form here), f16_stem and conv0's width (`_stem_f32_taped` serves those).
    An input that requires a gradient is declined: the fp16 stem backward never forms the conv0 map's gradient, so such a call
    takes the fp32 tape (densenet_train._DenseNetFn), whose stem backward ends in gnx_conv0_dgrad."""
    N, P = x.shape[0], x.shape[2]
    return (model.mfma == 'f16' and not model.training and not x.requires_grad and not model.drop_rate > 0 and   # (no dropout here)
            N % 8 == 0 and N != 0 and model._f16_fused_shapes_ok(P) and gammas_nonzero(model))       # N: whole 128-row tiles


def tape_bytes_per_spot(model, P):
    """HBM one spot holds on the fp16 tape plus its share of the backward's scratch: block buffers and their gradients (2 B),
    one activated bottleneck per layer (2 B), the pooled transition operands, the float patch and the fp32 pooled stem map."""
    hs, sizes = model._geometry(P)
    total, biggest = 0, 0
    for (c_in, layers, trans, c_total), s in zip(model._blocks, sizes):
        block = s * s * c_total
        total += block + len(layers) * s * s * 128 + (block // 4 if trans is not None else 0)
        biggest = max(biggest, 2 * block + 2 * s * s * 128)
    c0 = model.features.conv0.out_channels
    return 2 * (total + biggest) + 4 * 3 * P * P + 4 * 3 * sizes[0] * sizes[0] * c0


def _f32(n, dev):
    return torch.empty(max(int(n), 1), device=dev, dtype=F32)


def _rows_of_blocks(t, nblocks):
    """The first `nblocks` channel blocks of a channel-blocked buffer [C / 32][rows][32] as a row-major [rows][32 nblocks]
    matrix (one copy; for the few narrow operands whose consumers read rows: a transition's output gradient, the stem's)."""
    return t[:nblocks].permute(1, 0, 2).reshape(t.shape[1], 32 * nblocks).contiguous()


def _stem_f32_taped(tape, x, conv0, s0, st):
    """The stem in fp32 with window indices (running statistics; stem widths other than 64, `f16_stem = False`), then into
    block 1's first channel blocks as fp16.  The tape keeps norm0's stats `s0`, the fp32 pooled map and the indices."""
    N, P, c0, w0 = tape.N, tape.P, conv0.out_channels, conv0.weight.detach().contiguous()
    M1 = N * ((tape.hs + 2 - 3) // 2 + 1) ** 2
    tape.stats0 = s0
    tape.stem32 = torch.empty((M1, c0), device=x.device, dtype=F32)
    tape.pool_idx = torch.empty((M1, c0), device=x.device, dtype=torch.uint8)
    L.call('gnx_conv_stem_bnrelu_maxpool_argmax', L.ptr(x), L.ptr(w0), L.ptr(tape.stem32), c0, tape.pool_idx.data_ptr(), N, 3, P, P,
           c0, 7, 7, 2, 3, L.ptr(s0[0]), L.ptr(s0[1]), st)
    tape.bufs[0][:c0 // 32].copy_(tape.stem32.view(M1, c0 // 32, 32).permute(1, 0, 2))


class _DenseNetF16Fn(Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        x = model._unit_floats(x)
        N, _, P, _ = x.shape
        dev, st = x.device, L.stream()
        hs, sizes = model._geometry(P)
        tape = _Tape()
        tape.x, tape.N, tape.P, tape.hs, tape.sizes = x, N, P, hs, sizes
        # channel-blocked block buffers [c_total / 32][rows][32] (include/gridnext_hip.h: gnx_dense_layer_f16): the buffers the
        # eval forward of config 5 runs on - the taped forward IS that forward (DenseNet._block_f16 with a tape)
        bufs = tape.bufs = [torch.empty((c_total // 32, N * s * s, 32), device=dev, dtype=H16)
                            for (_, _, _, c_total), s in zip(model._blocks, sizes)]
        tape.stats0 = tape.stem32 = tape.pool_idx = None
        tape.layers, tape.trans = [], []          # per block: [(a, s1, s2) per layer]; (stt, pooled) or None
        conv0 = model.features.conv0
        def fold(bn):      # ONE launch per BatchNorm, just before the kernel that reads it (not the eval forward's cached table:
            return _bn(bn, None, bn.num_features, 0, False, dev, st)       # the backward needs mean and invstd as well)
        f16_stem = conv0.out_channels == 64 and model.f16_stem
        if not f16_stem:
            _stem_f32_taped(tape, x, conv0, fold(model.features.norm0), st)
        dlp = None                                # (the packed weights: built by block 0, after the stem)
        for bi, s in enumerate(sizes):
            dlp = model._block_f16(bi, bufs[bi], bufs[bi + 1] if bi + 1 < len(bufs) else None, x if f16_stem else None, N, s, P,
                                   fold, dlp, st, tape)
        tape.statsf = fold(model.features.norm_final)
        feats = torch.empty((N, model.num_features), device=dev, dtype=F32)
        model._tail_eval(bufs[-1], feats, N, sizes[-1], True, True, tape.statsf, st)
        return _finish_forward(ctx, model, tape, feats, params, st)

    @staticmethod
    def backward(ctx, dout):
        model, tape = ctx.model, ctx.tape
        _check_tape(tape, "its gradient would be computed from the new value")
        dout = dout.contiguous()
        b = _BackwardF16(model, tape, dout.device)
        grads, N = b.grads, tape.N
        bufs, dbufs = tape.bufs, [None] * len(tape.bufs)
        dbufs[-1] = b.tail(_classifier_backward(model, grads, dout, tape.feats, b.st))
        for bi in range(len(model._blocks) - 1, -1, -1):
            M = N * tape.sizes[bi] ** 2      # the block's scratch: dB [M][mid] (row-major), the workspaces of conv2's three kernels
            scratch = (torch.empty((M, b.mid), device=b.dev, dtype=H16), _f32(L.query('gnx_wgrad3x3_f16_workspace', M), b.dev),
                       _f32(L.query('gnx_conv3x3_dgrad_bnrelu_bwd_f16_workspace', M), b.dev),
                       _f32(L.query('gnx_conv3x3_bwd_f16_workspace', M), b.dev))
            for li in range(len(model._blocks[bi][1]) - 1, -1, -1):
                b.layer(bi, li, dbufs[bi], scratch)
                tape.layers[bi][li] = None
            del scratch
            if bi > 0:
                dbufs[bi - 1] = b.transition(bi, dbufs[bi])
                dbufs[bi] = None
                bufs[bi] = None
            grads.bucket()                                         # this block (+ the transition below it): final
        b.stem(dbufs)
        ctx.tape = None
        return grads.result(model)


class _LossScale:
    """The scaling policy of the fp16 gradients: ONE power-of-two loss scale `s` per backward, chosen on the device
    from the gradient that enters the network, s = 2^floor(tgt - log2(max |dfeats| * max |scale_final| / S^2)), tgt =
    `model.f16_grad_target` = 12, and re-centred at every transition for the block in front.  Published on the model for
    `training._F16StepGuard`: `f16_grad_overflow` (device int32, `flag_ptr`: OR-ed with 1 by any kernel that reduces a non-finite
    value, STICKY across backwards), `f16_grad_scale` ({s, 1/s} of the last backward), `f16_grad_block_scales` (last block first)."""

    def __init__(self, model, dev):
        pub = self.pub = model.__dict__
        flag = pub.get('f16_grad_overflow')
        if flag is None or flag.device != dev:
            flag = pub['f16_grad_overflow'] = torch.zeros(1, device=dev, dtype=torch.int32)
        self.flag_ptr, self.tgt = flag.data_ptr(), float(pub.get('f16_grad_target', 12.0))

    def start(self, dfeats, scale_final, S2):
        top = dfeats.abs().max() * scale_final.abs().max() / S2
        e = torch.where(top > 0, torch.floor(self.tgt - torch.log2(top.clamp_min(1e-38))), torch.zeros_like(top)).clamp(-24.0, 60.0)
        s_val = torch.exp2(e)
        self.cur = self.pub['f16_grad_scale'] = torch.stack([s_val, 1.0 / s_val]).to(F32).contiguous()
        self.ptr = L.ptr(self.cur)
        self.blocks = self.pub['f16_grad_block_scales'] = [self.cur]

    def recentre(self, dPool):
        """The power of two f that puts the largest element of the pooled gradient `dPool` back at 2^tgt (x 4-16 per block measured)."""
        mn, mx = torch.aminmax(dPool)                   # (one pass; abs() would write a copy of the tensor first)
        amax = torch.maximum(mx, -mn).to(F32)
        f_e = torch.where(amax > 0, torch.floor(self.tgt - torch.log2(amax.clamp_min(1e-30))), torch.zeros_like(amax))
        f_e = torch.minimum(torch.maximum(f_e, -24.0 - torch.log2(self.cur[0])), 60.0 - torch.log2(self.cur[0])).clamp(-12.0, 12.0)
        return torch.exp2(f_e)

    def advance(self, f_val):
        """s <- s f for the block in front, once the transition's kernel has been launched with the old scale."""
        s_new = self.cur[0] * f_val
        self.cur = torch.stack([s_new, 1.0 / s_new]).to(F32).contiguous()
        self.blocks.append(self.cur)
        self.ptr = L.ptr(self.cur)


class _BackwardF16:
    """The stages of one fp16 backward on the tape of its forward: tail, dense layer, transition, stem.  Every block buffer,
    block gradient and taped bottleneck is channel-blocked: (ld, bs) = (32, rows * 32) in the `_lb` entry points."""

    def __init__(self, model, tape, dev):
        self.model, self.tape, self.dev, self.st = model, tape, dev, L.stream()
        self.g, self.mid, self.grads = model.growth_rate, model.bn_size * model.growth_rate, _Grads()
        self.scale = _LossScale(model, dev)

    def tail(self, dfeats):
        """norm_final -> relu -> global average, under the loss scale chosen from `dfeats`; returns the last block's gradient."""
        model, tape, sc = self.model, self.tape, self.scale
        N, c, S2, sf, x = tape.N, model.num_features, tape.sizes[-1] ** 2, tape.statsf, tape.bufs[-1]
        sc.start(dfeats, sf[0][:c], S2)
        dx, bs = torch.empty_like(x), x.shape[1] * 32
        dg, db = self.grads.bn(model.features.norm_final)
        ws = _f32(L.query('gnx_tail_bwd_f16_workspace', N, c), self.dev)
        L.call('gnx_tail_bwd_f16_lb', L.ptr(dfeats), c, x.data_ptr(), 32, bs, dx.data_ptr(), 32, bs, N, c, S2, L.ptr(sf[0]),
               L.ptr(sf[1]), L.ptr(sf[2]), L.ptr(sf[3]), L.ptr(dg), L.ptr(db), L.ptr(ws), sc.ptr, 0, sc.flag_ptr, self.st)
        return dx

    def layer(self, bi, li, G, scratch):
        """Dense layer li of block bi: its parameter gradients, and its input's gradient accumulated into the block gradient G."""
        model, tape, grads, sc, st, g, mid = self.model, self.tape, self.grads, self.scale, self.st, self.g, self.mid
        layer, X, s = model._blocks[bi][1][li], tape.bufs[bi], tape.sizes[bi]
        M, cin = tape.N * s * s, model._blocks[bi][0] + li * g
        bs = M * 32                                          # halves between two channel blocks of X, G and the taped A
        (dB, ws3, wsd3, wsc3), (a, s1, s2) = scratch, tape.layers[bi][li]
        dy = G.data_ptr() + 2 * (cin // 32) * bs             # the layer's 32 gradient columns: ONE contiguous [M][32] matrix
        w1, w2 = layer.conv1.weight, layer.conv2.weight
        # both fp16 operands of the layer's backward in one launch: W2b [tap][m][n], W1t [cin][128]
        w2b, w1t = torch.empty((9, mid, g), device=self.dev, dtype=H16), torch.empty((cin, mid), device=self.dev, dtype=H16)
        L.call('gnx_dense_bwd_f16_pack', L.ptr(w1.detach().contiguous()), L.ptr(w2.detach().contiguous()), w1t.data_ptr(),
               w2b.data_ptr(), cin, st)                       # (mid = 128, g = 32: `eligible`)
        dgb2 = grads.bn(layer.norm2)
        if grads.want(w2) and model.f16_fused_conv2_backward:
            self.conv2_one_pass((layer, s, M, a, s2), dy, w2b, dgb2, dB, wsc3)
        else:
            self.conv2_two_passes((layer, s, M, a, s2), dy, w2b, dgb2, dB, ws3, wsd3)
        # conv1: data gradient + norm1 -> relu1's adjoint into the block gradient, and - from the same staged tiles - the
        # weight gradient (ONE pass over dB, X and G)
        dg1, db1 = grads.bn(layer.norm1)
        t0 = model._probe_begin()
        wg = grads.want(w1)
        ws = _f32(L.query('gnx_conv1x1_dgrad_wgrad_f16_workspace' if wg else 'gnx_conv1x1_dgrad_bnrelu_bwd_f16_workspace', M, cin),
                  self.dev)
        L.call('gnx_conv1x1_dgrad_wgrad_bnrelu_bwd_f16_lb', dB.data_ptr(), w1t.data_ptr(), X.data_ptr(), 32, bs, G.data_ptr(),
               32, bs, M, cin, L.ptr(s1[0]), L.ptr(s1[1]), L.ptr(s1[2]), L.ptr(s1[3]), L.ptr(dg1), L.ptr(db1),
               L.ptr(grads.new(w1)) if wg else None, L.ptr(ws), sc.ptr, 0, sc.flag_ptr, st)
        model._probe_mark('dgrad_wgrad1x1_bn1_f16' if wg else 'dgrad1x1_bn1_f16', t0, (4 if wg else 2) * M * cin * mid,
                          2 * M * (mid + 3 * cin))

    def conv2_one_pass(self, op, dy, w2b, dgb2, dB, ws):
        """conv2's whole backward - data gradient + norm2 adjoint AND weight gradient - in ONE pass over dY and A.
        `op`: the layer, its map size, rows M, taped bottleneck A and norm2 stats."""
        (layer, s, M, a, s2), model, sc, g, mid = op, self.model, self.scale, self.g, self.mid
        n2, bs = layer.norm2, M * 32
        t0 = model._probe_begin()
        L.call('gnx_conv3x3_bwd_f16_lb', dy, 32, w2b.data_ptr(), a.data_ptr(), 32, bs, dB.data_ptr(),
               L.ptr(self.grads.new(layer.conv2.weight)), M, s, L.ptr(s2[0]), L.ptr(n2.weight), L.ptr(n2.bias), L.ptr(dgb2[0]),
               L.ptr(dgb2[1]), L.ptr(ws), sc.ptr, 0, sc.flag_ptr, self.st)
        model._probe_mark('conv3x3_bwd_f16', t0, 4 * M * 9 * mid * g, 2 * M * (g + 2 * mid))

    def conv2_two_passes(self, op, dy, w2b, dgb2, dB, ws_w, ws_d):
        """conv2's weight gradient where it is wanted, then its data gradient + norm2 adjoint, a pass over dY and A each."""
        (layer, s, M, a, s2), model, sc, g, mid = op, self.model, self.scale, self.g, self.mid
        n2, w2, bs = layer.norm2, layer.conv2.weight, M * 32
        if self.grads.want(w2):
            t0 = model._probe_begin()
            L.call('gnx_wgrad3x3_f16_lb', dy, 32, a.data_ptr(), 32, bs, L.ptr(self.grads.new(w2)), L.ptr(ws_w), M, s, sc.ptr, 0,
                   sc.flag_ptr, self.st)
            model._probe_mark('wgrad3x3_f16', t0, 2 * M * 9 * mid * g, 2 * M * (mid + g))
        t0 = model._probe_begin()
        L.call('gnx_conv3x3_dgrad_bnrelu_bwd_f16_lb', dy, 32, w2b.data_ptr(), a.data_ptr(), 32, bs, dB.data_ptr(), M, s,
               L.ptr(s2[0]), L.ptr(n2.weight), L.ptr(n2.bias), L.ptr(dgb2[0]), L.ptr(dgb2[1]), L.ptr(ws_d), sc.ptr, 0, sc.flag_ptr,
               self.st)
        model._probe_mark('dgrad3x3_bn2_f16', t0, 2 * M * 9 * mid * g, 2 * M * (g + 2 * mid))

    def transition(self, bi, G):
        """Transition bi-1 -> bi from block bi's gradient G; returns block bi-1's, under the scale re-centred for that block."""
        model, tape, grads, sc, st, dev = self.model, self.tape, self.grads, self.scale, self.st, self.dev
        _, _, trans, p_total = model._blocks[bi - 1]
        N, ps, M, c_out, wt = tape.N, tape.sizes[bi - 1], G.shape[1], trans.conv.out_channels, trans.conv.weight
        X, (stt, pooled) = tape.bufs[bi - 1], tape.trans[bi - 1]
        # its output gradient is G's first c_out / 32 channel blocks; the two GEMMs that consume it read rows: one copy
        Gn = _rows_of_blocks(G, c_out // 32)                                                       # [M][c_out]
        if grads.want(wt):
            wsw = _f32(L.query('gnx_wgrad1x1_f16_workspace', M, c_out, p_total), dev)
            L.call('gnx_wgrad1x1_f16', Gn.data_ptr(), c_out, pooled.data_ptr(), p_total, None, None, L.ptr(grads.new(wt)),
                   L.ptr(wsw), M, c_out, p_total, sc.ptr, 0, sc.flag_ptr, st)
            del wsw
        tape.trans[bi - 1] = None
        del pooled
        wtt = wt.detach().reshape(c_out, p_total).t().to(H16).contiguous()                        # [p_total][c_out]
        dPool = torch.empty((p_total // 32, M, 32), device=dev, dtype=H16)                         # (channel-blocked)
        L.call('gnx_conv1x1_bnrelu_h16_cb', Gn.data_ptr(), c_out, wtt.data_ptr(), dPool.data_ptr(), M, M, p_total, c_out,
               None, None, None, None, st)
        del Gn
        dX, pbs = torch.empty_like(X), X.shape[1] * 32
        dgt, dbt = grads.bn(trans.norm)
        wst = _f32(L.query('gnx_trans_bwd_f16_workspace', N, p_total, ps), dev)
        # The re-centring factor f rides on the transition norm's folded (scale, shift) - the ReLU mask's sign test is
        # unchanged by a positive factor, the BatchNorm sums do not use them - so the kernel writes f x its block gradient
        # while its own sums still carry the old scale.
        f_val = sc.recentre(dPool)
        sc_f, sh_f = (stt[0] * f_val).contiguous(), (stt[1] * f_val).contiguous()          # (kept alive across the call)
        L.call('gnx_trans_bwd_f16_lb', dPool.data_ptr(), 32, M * 32, X.data_ptr(), 32, pbs, dX.data_ptr(), 32, pbs, N, p_total,
               ps, L.ptr(sc_f), L.ptr(sh_f), L.ptr(stt[2]), L.ptr(stt[3]), L.ptr(dgt), L.ptr(dbt), L.ptr(wst), sc.ptr, 0,
               sc.flag_ptr, st)
        sc.advance(f_val)
        return dX

    def stem(self, dbufs):
        """conv0 .. pool0 from block 1's gradient dbufs[0], released here: its first c0 / 32 channel blocks, copied out as rows."""
        grads, conv0, norm0 = self.grads, self.model.features.conv0, self.model.features.norm0
        need = grads.want(conv0.weight) or grads.want(norm0.weight) or grads.want(norm0.bias)
        Gs = _rows_of_blocks(dbufs[0], conv0.out_channels // 32) if need else None                 # [M1][c0]
        dbufs[0] = None
        if need and self.tape.pool_idx is None:
            self.stem_f16(conv0, norm0, Gs)
        elif need:
            self.stem_f32(conv0, norm0, Gs)

    def stem_f16(self, conv0, norm0, Gs):
        """One pass over the patches: conv0 rows recomputed, pool0's winners found, gradient routed and contracted."""
        model, tape, grads, sc = self.model, self.tape, self.grads, self.scale
        N, P, hs, c0, s0 = tape.N, tape.P, tape.hs, conv0.out_channels, tape.stats0
        t0 = model._probe_begin()
        ws = _f32(L.query('gnx_stem_bwd_f16_workspace', N, P), self.dev)
        dg0, db0 = grads.bn(norm0)
        L.call('gnx_stem_bwd_f16', L.ptr(tape.x), L.ptr(conv0.weight.detach().contiguous()), L.ptr(s0[0]), L.ptr(s0[1]),
               L.ptr(norm0.weight), L.ptr(norm0.bias), Gs.data_ptr(), c0,
               L.ptr(grads.new(conv0.weight)) if grads.want(conv0.weight) else None, L.ptr(dg0), L.ptr(db0), L.ptr(ws), N, P, c0,
               sc.ptr, 0, sc.flag_ptr, self.st)
        model._probe_mark('stem_bwd_f16', t0, 4 * N * hs * hs * c0 * 147, 4 * N * 3 * P * P + 2 * N * (hs // 2) ** 2 * c0)

    def stem_f32(self, conv0, norm0, Gs):
        """The fp32 stem's adjoints (`_stem_f32_taped`) on the gradient unscaled to fp32 (gnx_h16_cols_to_f32)."""
        tape, grads, sc, st, dev = self.tape, self.grads, self.scale, self.st, self.dev
        N, P, hs, c0, s0 = tape.N, tape.P, tape.hs, conv0.out_channels, tape.stats0
        M1, M0 = Gs.shape[0], N * hs * hs
        dO = torch.empty((M1, c0), device=dev, dtype=F32)
        L.call('gnx_h16_cols_to_f32', Gs.data_ptr(), c0, L.ptr(dO), c0, M1, c0, sc.ptr, sc.flag_ptr, st)
        dS = torch.empty((M0, c0), device=dev, dtype=F32)
        L.call('gnx_maxpool_bwd_argmax_bnrelu', tape.pool_idx.data_ptr(), L.ptr(dO), c0, L.ptr(tape.stem32), c0, L.ptr(s0[0]),
               L.ptr(dS), c0, N, c0, hs, hs, st)
        dg0, db0 = grads.bn(norm0)
        ws = _f32(L.query('gnx_bn_workspace', M1, c0), dev)
        L.call('gnx_bn_relu_bwd', L.ptr(dO), c0, L.ptr(tape.stem32), c0, None, c0, M1, c0, L.ptr(s0[0]), L.ptr(s0[1]),
               L.ptr(s0[2]), L.ptr(s0[3]), L.ptr(dg0), L.ptr(db0), 2, 0, 0, 0, L.ptr(ws), st)
        if grads.want(conv0.weight):
            ws = _f32(L.query('gnx_conv0_wgrad_workspace', N, P, P, c0, 7, 7, 2, 3), dev)
            L.call('gnx_conv0_wgrad', L.ptr(tape.x), L.ptr(dS), c0, L.ptr(grads.new(conv0.weight)), L.ptr(ws), N, P, P, c0, 7, 7,
                   2, 3, 0, st)
