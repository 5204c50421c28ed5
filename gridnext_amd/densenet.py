"""DenseNet-BC image spot classifier, MI355X-native.

Drop-in for `gridnext.densenet.DenseNet` (/root/reference/gridnext/densenet.py:78-159): same constructor
(:93-95), same parameter/buffer names (state_dict keys `features.conv0.weight`,
`features.denseblock{b}.denselayer{l}.{norm1,conv1,norm2,conv2}.*`, `features.transition{t}.{norm,conv}.*`,
`features.norm_final.*`, `classifier.*`), same initialisation (:141-150), same output.

The module tree below holds PARAMETERS ONLY (stock torch containers, so `.to()`, `.train()`, `state_dict()`
and optimizers behave as for the reference).  `forward` does not call them: it drives the hand-written gfx950
kernels of csrc/conv1x1.hip, conv3x3.hip and stem_pool.hip through the C ABI:
  * activations are channels-last matrices [spots*S*S, C]; a dense block is ONE buffer, each layer writes its
    `growth_rate` columns in place, so the reference's `torch.cat` (:14, :75) never happens;
  * BN+ReLU are folded into the operand load of the following conv; the transition averages 2x2 first;
  * a whole array's spots go through each kernel together (chunks only when activations would exceed ~40 GB,
    or when the caller sets `atonce` / GridNet.atonce_patch_limit).
`efficient=True` (checkpointing, :36-40): on the gradient path the forward keeps no tape and the backward recomputes it
(densenet_train._RecomputeFn); independently of the flag, a batch whose tape would exceed `tape_budget` bytes goes through in
recomputed chunks when BatchNorm runs on running statistics (train_gridwise always: training.py:126).
"""
import ctypes
import math
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import _lib as L
from . import functional as GF

F32 = torch.float32

EMPTY_GRANULE = 8      # spots: 8 spots of a 4 x 4 map are one 128-row tile, the unit every fast kernel of the chain takes


def compacted_spots(N, n_fg, chunk, granule=EMPTY_GRANULE):
    """Host arithmetic of the empty-spot compaction (DenseNet.skip_empty): how many spots the eval forward runs when `n_fg`
    of an array's `N` spots are non-empty and the uncompacted plan takes `chunk` spots at a time - or None: run all N.

    The compacted batch is the non-empty spots, ONE empty spot (the source of every empty spot's row) and copies of that
    empty spot up to a count that leaves the same remainder modulo `granule` as N.  Every launch of the chain picks its
    kernel by whether its rows are whole 128-row tiles (8 | spots on the 4 x 4 maps); a row's sums do not depend on its
    position, only on that choice, so keeping the remainder keeps the results bit for bit.  For the same reason the
    compaction is declined where the uncompacted call mixes the two classes of launches (chunks of whole tiles and a ragged
    last chunk, or chunks that are not whole tiles).  It is also declined where it would not run fewer spots."""
    if n_fg >= N:
        return None                                            # no empty spot
    n_c = n_fg + 1
    n_c += (N - n_c) % granule                                 # the smallest count >= n_fg + 1 congruent to N
    if n_c >= N:
        return None                                            # padding eats the saving
    if not (chunk >= N or (chunk % granule == 0 and N % granule == 0)):
        return None
    return n_c


RANGE_ROWS = 32768     # rows: one 128-row tile on each of the 256 CUs - the unit the two-range blocks count their rounds in


def block_ranges(n, s, min_rows=RANGE_ROWS):
    """Host arithmetic of the two-range dense blocks (DenseNet.two_ranges; gnx_dense_block_ranges): the rows M0 of the first
    range when a block of `n` spots on an s x s map runs as rows [0, M0) and [M0, n s s) on two streams, or 0: one range.

    Taken on the 8 x 8 and 4 x 4 maps, whose persistent kernels end every launch on a round of tiles that leaves most CUs
    empty.  The first range is WHOLE ROUNDS, as many as fit into half the rows: on the 8 x 8 map a round is 2 `min_rows`
    (512 conv1 workgroups of 128 rows = 256 Winograd workgroups of 256 pixels = 65 536 rows), on the 4 x 4 map `min_rows`
    (256 direct-conv2 workgroups of 128 rows = 32 768).  Its launches then end together, and only the second range ends on a
    partial round - which the first range's next launch fills (measured against plain halves: DESIGN 4.2).  A round is taken in
    whole groups of 8 spots (128-row tiles on the 4 x 4 map, 256-pixel Winograd tiles on the 8 x 8 one) and the second range
    must come out in whole 128-row tiles too; below two rounds the block stays one range.  Depends on s and n alone."""
    if s not in (4, 8):
        return 0
    M = n * s * s
    unit = math.lcm(min_rows * (2 if s == 8 else 1), EMPTY_GRANULE * s * s)
    r0 = M // 2 // unit * unit
    if r0 == 0 or (M - r0) % 128 != 0:
        return 0
    return r0


def empty_spot_lists(x):
    """(fg_idx, bg_idx, counts) of gnx_spot_compact for a contiguous patch batch x [N, ...] on a HIP device, or None where
    the kernel does not take the layout (16 | bytes per spot, 16-B aligned): int32 device tensors, fg_idx [N] = the spots
    with any non-zero byte, ascending, then the first all-zero spot repeated; bg_idx [N] = the all-zero spots, ascending,
    in [0, counts[1]); counts = [n_fg, n_bg]."""
    N = x.shape[0]
    ws = torch.empty(3 * N + 2, device=x.device, dtype=torch.int32)
    flags, fg, bg, counts = ws[:N], ws[N:2 * N], ws[2 * N:3 * N], ws[3 * N:]
    I32 = torch.int32
    if not L.try_call('gnx_spot_compact', x.data_ptr(), x[0].numel() * x.element_size() if N else 16, N, L.ptr(flags, I32),
                      L.ptr(fg, I32), L.ptr(bg, I32), L.ptr(counts, I32), L.stream()):
        return None
    return fg, bg, counts


class _DenseLayer(nn.Module):
    def __init__(self, c_in, growth_rate, bn_size, drop_rate):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(c_in)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = nn.Conv2d(c_in, bn_size * growth_rate, kernel_size=1, stride=1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth_rate)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False)
        self.drop_rate = drop_rate


class _Transition(nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.norm = nn.BatchNorm2d(c_in)
        self.relu = nn.ReLU(inplace=True)
        self.conv = nn.Conv2d(c_in, c_out, kernel_size=1, stride=1, bias=False)
        self.pool = nn.AvgPool2d(kernel_size=2, stride=2)


class DenseNet(nn.Module):
    def __init__(self, growth_rate=12, block_config=(16, 16, 16), compression=0.5,
                 num_init_features=24, bn_size=4, drop_rate=0,
                 num_classes=10, small_inputs=True, efficient=False, classify=True):
        super().__init__()
        assert 0 < compression <= 1, 'compression of densenet should be between 0 and 1'
        self.drop_rate = float(drop_rate or 0)      # dropout after conv2 (:42-43): a keep-mask on the layer's 32 new columns in
                                                    # training mode (densenet_train), identity otherwise
        self.growth_rate, self.block_config = growth_rate, tuple(block_config)
        self.bn_size, self.small_inputs, self.classify = bn_size, small_inputs, classify
        self.efficient = bool(efficient)      # gradient path: no tape in the forward, recompute in the backward (:12-18, :36-40)
        self.tape_budget = 150 * 1024 ** 3    # bytes of tape one backward may hold (eval-statistics gradient path): beyond
                                              # it the batch is cut into recomputed chunks (a 256-px array: 3 chunks)
        self.atonce = None          # spots per chunk in eval mode (None = auto)
        self.mfma = 'f32'           # 'f16': fp16 matrix-core operands in the eval forward (BASELINE config 5)
        self.split_conv1 = False    # eval forward, fp32 path: conv1 on SPLIT bf16 operands (three 16-bit matrix instructions per
                                    # product, fp32 tensors and accumulation: csrc/conv1x1_split.hip; opt-in, fp32-grade results)
        self.split_conv2 = False    # ... and conv2 as nine shifted products of split bf16 operands (csrc/conv3x3_split.hip)
        self.split_wgrad = False    # fp32 gradient path: conv1's weight gradient on split bf16 operands (csrc/wgrad_split.hip)
        self.winograd = True        # eval forward: conv2 as Winograd F(2,3) along x where the shape allows (fp32 path;
                                    # same arithmetic type, 1.5x fewer matrix operations, rounding-level differences)
        self.skip_empty = True      # eval forward, fp32 path with the fused stem: all-zero patches (the background of an array)
                                    # are evaluated ONCE per call and that row copied to every one of them - bit for bit the
                                    # rows f gives them anyway (compacted_spots); False: every spot goes through every kernel
        self.two_ranges = False     # eval forward, fp32 path: the dense blocks on 8 x 8 and 4 x 4 maps as two row ranges on two
                                    # streams from two rounds of tiles on (block_ranges; gnx_dense_block_ranges): a range's launch
                                    # takes the CUs the other's last round of tiles leaves empty - the same kernels, the same bits.
                                    # Opt-in: 1.0 - 1.4 ms of the 56-ms step in every session, but within twice the run-to-run
                                    # spread in two sessions of three
        self.range_rows = RANGE_ROWS    # ... the rows of a round's unit (tests lower it to reach the path with a few spots)
        self.f16_buffers = True     # mfma = 'f16' only: the block buffers themselves in fp16 where the shapes allow
        self.f16_stem = True        # ... and, with fp16 block buffers, conv0's matrix operands in fp16 too
        self.f16_fused = True       # ... and every dense layer as ONE kernel, the bottleneck in LDS only (gnx_dense_layer_f16)
        self.f16_fused_transitions = True   # ... and every transition as ONE kernel, the pooled operand in LDS only (gnx_transition_f16)
        self.f16_fused_conv2_backward = True    # fp16 gradient path: conv2's data + weight gradient in one pass (gnx_conv3x3_bwd_f16_lb)
        self.input_norm = None      # (mean[3], std[3]) of a torchvision Normalize to apply to UINT8 input patches after the
                                    # u8 / 255 of ToTensor (fused into the stem's operand load); float inputs are taken as
                                    # already transformed by the dataset, as in the reference
        self.input_resize = None    # int (short edge), (h, w) or None: torchvision's Resize of UINT8 input patches, on the device,
        self.input_crop = None      # int or None: ... and its CenterCrop, in front of everything else (gnx_resize_crop_u8: Pillow's
                                    # bytes bit for bit; transforms.py).  `set_input_transform(compose)` sets all three

        feats = OrderedDict()
        if small_inputs:
            feats['conv0'] = nn.Conv2d(3, num_init_features, kernel_size=3, stride=1, padding=1, bias=False)
        else:
            feats['conv0'] = nn.Conv2d(3, num_init_features, kernel_size=7, stride=2, padding=3, bias=False)
            feats['norm0'] = nn.BatchNorm2d(num_init_features)
            feats['relu0'] = nn.ReLU(inplace=True)
            feats['pool0'] = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, ceil_mode=False)
        c = num_init_features
        self._blocks = []           # [(c_in, [layers], transition|None, c_total)]
        for bi, n_layers in enumerate(self.block_config):
            block = nn.Module()
            layers = []
            for li in range(n_layers):
                layer = _DenseLayer(c + li * growth_rate, growth_rate, bn_size, drop_rate)
                block.add_module('denselayer%d' % (li + 1), layer)
                layers.append(layer)
            feats['denseblock%d' % (bi + 1)] = block
            c_total = c + n_layers * growth_rate
            trans = None
            if bi != len(self.block_config) - 1:
                trans = _Transition(c_total, int(c_total * compression))
                feats['transition%d' % (bi + 1)] = trans
            self._blocks.append((c, layers, trans, c_total))
            c = int(c_total * compression) if trans is not None else c_total
        feats['norm_final'] = nn.BatchNorm2d(c)
        self._layers = [l for _, ls, _, _ in self._blocks for l in ls]
        self._transitions = [t for _, _, t, _ in self._blocks if t is not None]
        self.features = nn.Sequential(feats)
        self.num_features = c
        self.classifier = nn.Linear(c, num_classes)

        for name, param in self.named_parameters():          # densenet.py:141-150
            if 'conv' in name and 'weight' in name:
                n = param.size(0) * param.size(2) * param.size(3)
                param.data.normal_().mul_(math.sqrt(2. / n))
            elif 'norm' in name and 'weight' in name:
                param.data.fill_(1)
            elif 'norm' in name and 'bias' in name:
                param.data.fill_(0)
            elif 'classifier' in name and 'bias' in name:
                param.data.fill_(0)
        self._dropout_mask = None   # test hook: callable (layer index, rows, columns, device) -> bool keep-mask [rows][columns]
        self._cache = {}
        self._cache_epoch = 0       # part of every cache key; bumped by invalidate_cache()
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_cache())

    # ------------------------------------------------------------------ cached, derived device tensors
    def invalidate_cache(self):
        """Drop the derived device tensors of the eval forward (folded BN scale/shift, repacked / Winograd / fp16 conv
        weights).  They are keyed on each source tensor's (`_version`, `data_ptr()`), which catches optimizer steps and
        `.to()`; writes that bump neither - kernels updating running statistics through raw pointers, `p.data` writes,
        collectives into `.data` - must call this.  Called by the training forward, `load_state_dict`, `_apply`
        (`.to()`, `.float()`, ...) and `distributed.broadcast_module`."""
        self._cache = {}
        self._cache_epoch += 1

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_cache()
        return out

    def _key(self, tensors):
        return (self._cache_epoch, bool(self.two_ranges)) + tuple(v for t in tensors for v in (t._version, t.data_ptr()))

    def _bn_modules(self):
        mods = []
        if not self.small_inputs:
            mods.append(self.features.norm0)
        for _, layers, trans, _ in self._blocks:
            for l in layers:
                mods += [l.norm1, l.norm2]
            if trans is not None:
                mods.append(trans.norm)
        mods.append(self.features.norm_final)
        return mods

    def _cached(self, name, key, build):
        """Cache entry `name`: its value while the stored key equals `key` (normally `_key(sources)`), else `build()`."""
        hit = self._cache.get(name)
        if hit is None or hit[0] != key:
            hit = self._cache[name] = (key, build())
        return hit[1]

    def _folded_eval(self):
        """{bn module: (scale, shift)} for running-stat BN; refreshed when any BN tensor changed."""
        mods = self._bn_modules()

        def build():
            total = sum((m.num_features + 3) // 4 * 4 for m in mods)   # every slice starts 16-B aligned (float4 loads)
            buf = torch.empty((2, total), device=mods[0].weight.device, dtype=F32)   # (the table's views keep it alive)
            table, off = {}, 0
            st = L.stream()
            for m in mods:
                c = m.num_features
                sc, sh = buf[0, off:off + c], buf[1, off:off + c]
                L.call('gnx_bn_fold_eval', c, L.ptr(m.weight), L.ptr(m.bias), L.ptr(m.running_mean),
                       L.ptr(m.running_var), float(m.eps), L.ptr(sc), L.ptr(sh), None, None, st)
                table[m] = (sc, sh)
                off += (c + 3) // 4 * 4
            return table
        return self._cached('fold', self._key([t for m in mods for t in (m.weight, m.bias, m.running_mean, m.running_var)]),
                            build)

    def _conv2_key(self):
        return self._key([l.conv2.weight for l in self._layers])

    def _conv1_key(self):
        return self._key([l.conv1.weight for l in self._layers])

    def _repacked_conv2(self):
        """{layer: conv2 weight as [tap][growth][mid]} refreshed when a conv2 weight changed."""
        def build():
            table, st = {}, L.stream()
            for l in self._layers:
                w = l.conv2.weight
                table[l] = torch.empty((9,) + w.shape[:2], device=w.device, dtype=F32)
                L.call('gnx_repack_conv3x3', L.ptr(w.detach().contiguous()), L.ptr(table[l]), w.shape[0], w.shape[1], st)
            return table
        return self._cached('w2', self._conv2_key(), build)

    def _repacked_conv2_f16(self):
        """{layer: the tap-major conv2 weight rounded to fp16} (config 5's DMA conv2), refreshed with the weights."""
        return self._cached('w2h', self._conv2_key(),
                            lambda: {l: w.to(torch.float16) for l, w in self._repacked_conv2().items()})

    def _conv1_f16(self):
        """{layer: conv1 weight [mid][cin] rounded to fp16} (config 5 on fp16 block buffers), refreshed with the weights."""
        return self._cached('w1h', self._conv1_key(), lambda: {
            l: l.conv1.weight.detach().reshape(l.conv1.weight.shape[0], -1).to(torch.float16).contiguous() for l in self._layers})

    def _dense_f16_packed(self):
        """{layer: (w1p, w2p)}: conv1 / conv2 weights rounded to fp16 once, in the MFMA-fragment order gnx_dense_layer_f16
        streams (csrc/dense_layer_f16.hip); refreshed with the weights."""
        def build():
            table, st = {}, L.stream()
            for l in self._layers:
                w1, w2 = l.conv1.weight.detach().contiguous(), l.conv2.weight.detach().contiguous()
                w1p = torch.empty(w1.numel(), device=w1.device, dtype=torch.float16)
                w2p = torch.empty(w2.numel(), device=w1.device, dtype=torch.float16)
                L.call('gnx_dense_layer_f16_pack', L.ptr(w1), L.ptr(w2), L.ptr(w1p, torch.float16), L.ptr(w2p, torch.float16),
                       w1.shape[1], st)
                table[l] = (w1p, w2p)
            return table
        return self._cached('dlp', self._key([w for l in self._layers for w in (l.conv1.weight, l.conv2.weight)]), build)

    def _trans_f16(self):
        """{transition: conv weight [c_out][c_in] rounded to fp16} (config 5's two-step transitions), refreshed with the weights."""
        return self._cached('wth', self._key([t.conv.weight for t in self._transitions]), lambda: {
            t: t.conv.weight.detach().reshape(t.conv.weight.shape[0], -1).to(torch.float16).contiguous() for t in self._transitions})

    def _trans_f16_packed(self):
        """{transition: conv weight in gnx_transition_f16's fragment order (fp16)} - the fused transitions of config 5 -,
        refreshed with the weights."""
        def build():
            table, st = {}, L.stream()
            for t in self._transitions:
                w = t.conv.weight.detach().reshape(t.conv.weight.shape[0], -1).contiguous()
                table[t] = torch.empty(w.numel(), device=w.device, dtype=torch.float16)
                L.call('gnx_transition_f16_pack', L.ptr(w), L.ptr(table[t], torch.float16), w.shape[0], w.shape[1], st)
            return table
        return self._cached('wtp', self._key([t.conv.weight for t in self._transitions]), build)

    def _f16_dma_ok(self, M, s, mid, c_total):
        """Shapes gnx_conv3x3_f16_dma takes (conv3x3.hip): growth 32, 128 | mid, power-of-two maps 4..64, whole 128-row
        tiles, 32-bit element offsets."""
        return (self.growth_rate == 32 and mid % 128 == 0 and s in (4, 8, 16, 32, 64) and M % 128 == 0
                and M * max(mid, c_total) < 2 ** 31)

    # ---- the shape rules of the fp16 paths, each term once; combined by `_eval_plan`, `forward` (padding) and densenet_train_f16.eligible
    def _f16_patches_ok(self, P):        # the 7 x 7 stem on 128- / 256-px patches: what the fp16-output stem kernels take
        return not self.small_inputs and P in (128, 256)

    def _f16_maps_ok(self, P):           # every map a power of two in 4 .. 64: the tiles of the fp16 conv2 kernels, fused or not
        return all(s in (4, 8, 16, 32, 64) for s in self._geometry(P)[1])

    def _f16_growth_ok(self, one_tile=False):
        mid = self.bn_size * self.growth_rate   # whole 128-channel tiles (`_f16_dma_ok`); the fused kernels, fwd / bwd, hold ONE in the LDS
        return self.growth_rate == 32 and (mid == 128 if one_tile else mid % 128 == 0)

    def _f16_fused_shapes_ok(self, P):
        """Networks and patches gnx_dense_layer_f16 (and its `_tape` twin) takes: the terms above, and every block's input -
        conv0's width, each transition's output - in whole 32-channel blocks, at least two, at most 1024 + 32 channels in all."""
        return self._f16_patches_ok(P) and self._f16_growth_ok(one_tile=True) and self._f16_maps_ok(P) and \
            self.num_features % 32 == 0 and all(c_in % 32 == 0 and c_in >= 64 and c_total <= 1024 + 32
                                                for c_in, _, _, c_total in self._blocks)

    def _winograd_conv2(self):
        """{layer: conv2 weight as Winograd F(2,3)-along-x factors [3][4][growth][mid]} refreshed with the weights."""
        def build():
            table, st = {}, L.stream()
            for l in self._layers:
                w = l.conv2.weight
                table[l] = torch.empty((12,) + w.shape[:2], device=w.device, dtype=F32)
                L.call('gnx_winograd_conv3x3_weights', L.ptr(w.detach().contiguous()), L.ptr(table[l]), w.shape[0], w.shape[1], st)
            return table
        return self._cached('w2u', self._conv2_key(), build)

    def _split_conv1(self):
        """{layer: conv1 weight split into bf16 hi / lo planes by 64-wide K chunks (gnx_conv1x1_split_pack)} refreshed with the
        weights."""
        def build():
            table, st = {}, L.stream()
            for l in self._layers:
                w = l.conv1.weight
                table[l] = torch.empty(L.query('gnx_conv1x1_split_pack_halves', w.shape[1]), device=w.device, dtype=torch.bfloat16)
                L.call('gnx_conv1x1_split_pack', L.ptr(w.detach().contiguous()), table[l].data_ptr(), w.shape[1], st)
            return table
        return self._cached('w1s', self._conv1_key(), build)

    def _split_conv2(self):
        """{layer: conv2 weight split into bf16 hi / lo planes by 32-channel chunks and taps (gnx_conv3x3_split_pack)}."""
        def build():
            table, st = {}, L.stream()
            for l in self._layers:
                w = l.conv2.weight
                table[l] = torch.empty(L.query('gnx_conv3x3_split_pack_halves'), device=w.device, dtype=torch.bfloat16)
                L.call('gnx_conv3x3_split_pack', L.ptr(w.detach().contiguous()), table[l].data_ptr(), st)
            return table
        return self._cached('w2s', self._conv2_key(), build)

    def _norm_vector(self, dev):
        """Device floats {mean[3], std[3], 1/std[3]} for the uint8 entry points, or None (ToTensor only)."""
        if self.input_norm is None:
            return None
        mean, std = self.input_norm
        key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), str(dev), self._cache_epoch)

        def build():
            m, sd = torch.tensor(key[0], dtype=F32), torch.tensor(key[1], dtype=F32)
            assert m.numel() == 3 and sd.numel() == 3, "input_norm = (mean[3], std[3])"
            return torch.cat([m, sd, 1.0 / sd]).to(dev)              # 1 / std: one correctly rounded fp32 division
        return self._cached('nrm', key, build)

    def set_input_transform(self, compose):
        """Run the dataset's transform (`gridnext_amd.transforms.Compose`, e.g. `dataset.device_transform`) on the device, on
        the uint8 patches the dataset then delivers at their stored size: sets `input_resize`, `input_crop` and `input_norm`
        from its device plan.  None switches all three off."""
        if compose is None:
            self.input_resize = self.input_crop = self.input_norm = None
            return self
        plan = compose.device_plan()
        if plan is None:
            raise ValueError("this transform cannot run on the device: %s" % compose.device_plan_refusal())
        self.input_resize, self.input_crop, self.input_norm = plan
        return self

    def _input_transform_set(self):
        return self.input_resize is not None or self.input_crop is not None

    def _transformed_input(self, x, as_float):
        """`input_resize` / `input_crop` of the stored patches `x` (N, 3, H0, W0), which must be uint8 (the transform is
        defined on bytes): uint8 (N, 3, Ph, Pw) for the stems that take bytes, or with `as_float` the floats `_unit_floats`
        would make of those bytes, in the same pass (gnx_resize_crop_u8_f32)."""
        if x.dtype != torch.uint8:
            raise ValueError("input_resize / input_crop are defined on uint8 patches (Pillow's byte arithmetic); got %s - "
                             "pass the stored bytes, or clear the switches for patches the dataset already transformed" % x.dtype)
        from .transforms import resize_crop
        return resize_crop(x, self.input_resize, self.input_crop, self._norm_vector(x.device) if as_float else None, as_float)

    def _float_patches(self, x):
        """The float32 patches the network sees for the patches `x` as they arrive: `input_resize` / `input_crop` where set,
        then ToTensor (+ Normalize) of uint8 patches; float input passes through."""
        if self._input_transform_set():
            return self._transformed_input(x, True)
        return self._unit_floats(x)

    def _unit_floats(self, x):
        """ToTensor (+ Normalize) of uint8 patches (N, 3, P, P) as its own pass -> float32, the floats torch would produce
        (gnx_u8_to_f32); float input passes through."""
        if x.dtype != torch.uint8:
            return x.contiguous().float()
        x = x.contiguous()
        out = torch.empty(x.shape, device=x.device, dtype=F32)
        if x.numel():
            L.call('gnx_u8_to_f32', x.data_ptr(), L.ptr(out), x.shape[0], x.shape[1], x.shape[2], x.shape[3],
                   L.ptr(self._norm_vector(x.device)), L.stream())
        return out

    def _geometry(self, P):
        if self.small_inputs:
            hs, s = None, P
        else:
            hs = (P + 6 - 7) // 2 + 1
            s = (hs + 2 - 3) // 2 + 1
        sizes = []
        for _ in self._blocks:
            sizes.append(s)
            s = s // 2
        return hs, sizes

    def _auto_chunk(self, P, n, elem_bytes=4):
        if self.atonce is not None:
            return max(1, min(int(self.atonce), n))
        hs, sizes = self._geometry(P)
        per_spot = 0
        if hs is not None:
            per_spot += hs * hs * self.features.conv0.out_channels
        for (c_in, layers, trans, c_total), s in zip(self._blocks, sizes):
            per_spot += s * s * c_total
        per_spot += sizes[0] * sizes[0] * self.bn_size * self.growth_rate
        # Later blocks have few positions per spot (S=4: 16), so a launch only fills 256 CUs when thousands of
        # spots go through together: size chunks by HBM (288 GB), not by cache - a whole 128-px array is 17 GB.
        budget = 40 * 1024 ** 3 // elem_bytes      # elements
        return max(1, min(n, max(32, budget // max(per_spot, 1))))

    # ------------------------------------------------------------------ optional per-kernel timing (bench.py)
    _probe = None      # when a list: (kind, start_event, end_event, flops, bytes) per dense-layer launch, on the launch stream
                       # (flops / bytes: the ALGORITHMIC work of that launch - bench.py credits a kernel kind with exactly the
                       # launches it timed)

    def _probe_begin(self):
        if self._probe is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _probe_mark(self, kind, start, flops=None, nbytes=None):
        if self._probe is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self._probe.append((kind, start, ev, flops, nbytes))
        return ev

    # ------------------------------------------------------------------ stem of the eval forward
    def _stem_eval(self, xu, rows, c_total, P, hs, use_h, fold, w0, stem_out, chunk, st, src=None, n_src=0):
        """conv0 (-> norm0 -> relu0 -> pool0) of `xu` (float or uint8 patches) into the first block buffer `rows`.
        `src` (int32 device list, `n_src` entries): image i of `rows` is patch src[i] of `xu` instead of patch i.
        Returns the conv0-map scratch buffer (allocated on first need by the two-kernel path)."""
        nu = xu.shape[0]
        dev = xu.device
        c0 = self.features.conv0.out_channels
        if src is not None:                 # (the caller checked _skip_empty_shapes: the fused fp32-output stem takes the call)
            sc, sh = fold[self.features.norm0]
            if xu.dtype == torch.uint8:
                L.call('gnx_conv_stem_bnrelu_maxpool_u8_idx', xu.data_ptr(), L.ptr(w0), L.ptr(rows), c_total, n_src, 3, P, P, c0,
                       7, 7, 2, 3, L.ptr(sc), L.ptr(sh), L.ptr(self._norm_vector(dev)), L.ptr(src, torch.int32), nu, st)
            else:
                L.call('gnx_conv_stem_bnrelu_maxpool_idx', L.ptr(xu), L.ptr(w0), L.ptr(rows), c_total, n_src, 3, P, P, c0, 7, 7,
                       2, 3, L.ptr(sc), L.ptr(sh), L.ptr(src, torch.int32), nu, st)
            return stem_out
        if self.small_inputs:
            xu = self._unit_floats(xu)
            L.call('gnx_conv_stem', L.ptr(xu), L.ptr(w0), L.ptr(rows), c_total, nu, 3, P, P, c0, 3, 3, 1, 1, st)
            return stem_out
        sc, sh = fold[self.features.norm0]
        u8 = xu.dtype == torch.uint8
        # config 5: the stem's matrix operands in fp16 too (float or uint8 patches)
        if use_h and self.f16_stem and L.try_call(
                'gnx_conv_stem_bnrelu_maxpool_f16mul', xu.data_ptr(), 1 if u8 else 0, L.ptr(w0), rows.data_ptr(), c_total, nu, 3,
                P, P, c0, 7, 7, 2, 3, L.ptr(sc), L.ptr(sh), L.ptr(self._norm_vector(dev)) if u8 else None, st):
            return stem_out
        # conv0 -> norm0 -> relu0 -> pool0 in one kernel where the geometry allows (128- / 256-px patches): the conv0 map
        # (5.2 GB per 128-px array) then never touches HBM.  uint8 patches: ToTensor (+ Normalize) inside that kernel too.
        if u8:
            if L.try_call('gnx_conv_stem_bnrelu_maxpool_u8', xu.data_ptr(), L.ptr(w0), rows.data_ptr(), c_total, nu, 3, P, P,
                          c0, 7, 7, 2, 3, L.ptr(sc), L.ptr(sh), L.ptr(self._norm_vector(dev)), 1 if use_h else 0, st):
                return stem_out
            xu = self._unit_floats(xu)                        # other geometries: convert, then the float stems
        if use_h:
            L.call('gnx_conv_stem_bnrelu_maxpool_h16', L.ptr(xu), L.ptr(w0), L.ptr(rows, torch.float16), c_total, nu, 3, P, P,
                   c0, 7, 7, 2, 3, L.ptr(sc), L.ptr(sh), st)
        elif not L.try_call('gnx_conv_stem_bnrelu_maxpool', L.ptr(xu), L.ptr(w0), L.ptr(rows), c_total, nu, 3, P, P, c0, 7, 7,
                            2, 3, L.ptr(sc), L.ptr(sh), st):
            if stem_out is None:
                stem_out = torch.empty((chunk * hs * hs, c0), device=dev, dtype=F32)
            L.call('gnx_conv_stem', L.ptr(xu), L.ptr(w0), L.ptr(stem_out), c0, nu, 3, P, P, c0, 7, 7, 2, 3, st)
            L.call('gnx_bnrelu_maxpool', L.ptr(stem_out), c0, L.ptr(rows), c_total, nu, c0, hs, hs, L.ptr(sc), L.ptr(sh), st)
        return stem_out

    def _block_f16(self, bi, buf, nxt, xs, n, s, P, bn, dlp, st, tape=None):
        """One dense block of config 5 on its channel-blocked fp16 buffer `buf` [c_total / 32][rows][32] for `n` spots - the
        eval forward and the taped forward of densenet_train_f16 both run it: the fp16 stem of the patches `xs` (block 0;
        `xs` None: the caller ran a stem of its own), every dense layer as ONE kernel, and the transition into `nxt`.
        `bn`: callable BatchNorm -> (scale, shift, ...), asked in launch order (eval: the cached table; taped: one fold launch
        each).  `dlp`: _dense_f16_packed(), or None: built after the stem, with _trans_f16() (the taped forward's order);
        returned for the next block.  With `tape` the `_tape` entry points run - the same kernels, bit for bit - and record
        norm0's stats0, per layer (activated bottleneck [4][n s s][32], norm1 stats, norm2 stats), (stt, pooled)."""
        c_in, layers, trans, c_total = self._blocks[bi]
        H, dev, rows_total, M = torch.float16, buf.device, buf.shape[1], n * s * s
        if bi == 0 and xs is not None:
            conv0, s0, u8 = self.features.conv0, bn(self.features.norm0), xs.dtype == torch.uint8
            L.call('gnx_conv_stem_bnrelu_maxpool_f16mul_cb', xs.data_ptr(), 1 if u8 else 0, L.ptr(conv0.weight.detach().contiguous()),
                   buf.data_ptr(), rows_total, n, 3, P, P, conv0.out_channels, 7, 7, 2, 3, L.ptr(s0[0]), L.ptr(s0[1]),
                   L.ptr(self._norm_vector(dev)) if u8 else None, st)
            if tape is not None:
                tape.stats0 = s0
        if dlp is None:
            dlp = self._dense_f16_packed()
            self._trans_f16()       # (refreshed here as well, as the taped forward always has, whichever transition form runs)
        recs = []
        for li, layer in enumerate(layers):
            cin = c_in + li * self.growth_rate
            s1, s2 = bn(layer.norm1), bn(layer.norm2)
            args = (L.ptr(buf, H), rows_total, n, s, cin, L.ptr(dlp[layer][0], H), L.ptr(dlp[layer][1], H), L.ptr(s1[0]),
                    L.ptr(s1[1]), L.ptr(s2[0]), L.ptr(s2[1]))
            flops = 2 * M * (cin * 128 + 9 * 128 * 32)
            if tape is None:
                t0 = self._probe_begin()
                L.call('gnx_dense_layer_f16', *args, st)
                self._probe_mark('dense_layer', t0, flops, 2 * M * (cin + 32))
            else:
                a = torch.empty((4, M, 32), device=dev, dtype=H)
                t0 = self._probe_begin()
                L.call('gnx_dense_layer_f16_tape', *args, a.data_ptr(), M, st)
                self._probe_mark('dense_layer_tape', t0, flops, 2 * M * (cin + 32 + 128))
                recs.append((a, s1, s2))
        rec = None
        if trans is not None:
            Mo, cout, stt = n * (s // 2) ** 2, trans.conv.out_channels, bn(trans.norm)
            # (what gnx_transition_f16 and its `_tape` twin take: whole 128-row output tiles, 32-bit byte offsets in a channel block)
            fused = (self.f16_fused_transitions and s in (8, 16, 32, 64) and 64 <= c_total <= 1024 and cout % 128 == 0 and
                     cout <= 512 and Mo % 128 == 0 and rows_total * 64 < 2 ** 32 - 2 ** 25)
            pooled = torch.empty((Mo, c_total), device=dev, dtype=H) if (tape is not None or not fused) else None
            rec = (stt, pooled)
            if fused:       # one kernel: the pooled operand exists in the LDS only (bit-identical to the pooling pass's output)
                args = (L.ptr(buf, H), rows_total, n, s, c_total, cout, L.ptr(self._trans_f16_packed()[trans], H), L.ptr(stt[0]),
                        L.ptr(stt[1]), L.ptr(nxt, H), nxt.shape[1])
                if tape is None:
                    L.call('gnx_transition_f16', *args, st)
                else:
                    L.call('gnx_transition_f16_tape', *args, pooled.data_ptr(), c_total, st)
            else:
                L.call('gnx_bnrelu_avgpool2_h16_cb', L.ptr(buf, H), rows_total, L.ptr(pooled, H), c_total, n, c_total, s,
                       L.ptr(stt[0]), L.ptr(stt[1]), st)
                L.call('gnx_conv1x1_bnrelu_h16_cb', L.ptr(pooled, H), c_total, L.ptr(self._trans_f16()[trans], H), L.ptr(nxt, H),
                       nxt.shape[1], Mo, cout, c_total, None, None, None, None, st)
        if tape is not None:
            tape.layers.append(recs)
            tape.trans.append(rec)
        return dlp

    def _f16_pad(self, x):
        """Empty patches that pad a ragged batch to whole groups of 8 spots (128-row tiles on the 4 x 4 maps) under running
        statistics: spots are independent, the extra rows are dropped and get a zero output gradient.  Only for calls the
        fp16-buffer kernels can take - others would pay for nothing (maps, channels not asked: unchanged from before)."""
        ok = self.mfma == 'f16' and x.shape[0] > 0 and not self.training and not x.requires_grad and self.f16_buffers and \
            self._f16_patches_ok(x.shape[2]) and self._f16_growth_ok()
        return (-x.shape[0]) % 8 if ok else 0

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("gridnext_amd.DenseNet runs on a HIP device only (input is on %s); "
                               "there is no CPU fallback" % x.device)
        if self._input_transform_set():
            if x.dim() != 4 or x.shape[1] != 3:
                raise ValueError("expected RGB patches (N, 3, H, W), got %s" % (tuple(x.shape),))
            # the stored patches -> the patches the network sees, first; the rest is the uint8 call on the result.  Bytes where
            # a fused uint8 stem takes them (the eval forward on 128 / 256 px), else the floats `_unit_floats` would make next
            on_tape = self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))
            P = self._input_geometry(x.shape[2], x.shape[3])[4]
            x = self._transformed_input(x, on_tape or self.small_inputs or P not in (128, 256))
        return self._forward_patches(x)

    def _input_geometry(self, H0, W0):
        from .transforms import transform_geometry
        return transform_geometry(H0, W0, self.input_resize, self.input_crop)

    def _forward_patches(self, x):
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError("expected square RGB patches (N, 3, P, P), got %s" % (tuple(x.shape),))
        if x.dtype not in (torch.uint8, torch.float32):
            x = x.float()
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        pad = self._f16_pad(x)
        if pad:
            xp = torch.cat([x, x.new_zeros((pad,) + tuple(x.shape[1:]))], 0)
            return self._forward_patches(xp)[:x.shape[0]]
        if self.training or needs_grad:
            from .densenet_train import densenet_autograd       # training / gradient path
            return densenet_autograd(self, x)
        return self._forward_eval(x.detach())

    def _eval_plan(self, N, P):
        """(spots per chunk, fp16 block buffers?, fused fp16 layers?) of an eval forward over N patches of P px: host
        arithmetic on the model's settings, decided for the whole call (the buffers cannot change type half-way)."""
        if self.mfma not in ('f32', 'f16'):
            raise ValueError("DenseNet.mfma must be 'f32' or 'f16'")
        f16, mid, c0 = self.mfma == 'f16', self.bn_size * self.growth_rate, self.features.conv0.out_channels
        sizes = self._geometry(P)[1]
        # the fused dense layers need fp16 block buffers and the one stem that writes them channel-blocked (gnx_conv_stem_bnrelu_
        # maxpool_f16mul_cb: 32 | c0 <= 64, multiplies fp16 operands: f16_stem); the gradient path has an fp32 stem besides: `eligible`
        fused_ok = f16 and self.f16_buffers and self.f16_fused and self.f16_stem and self._f16_fused_shapes_ok(P) and c0 in (32, 64)
        # fp16 BLOCK BUFFERS hold twice the spots in the same bytes - a whole 256-px array, 34 GB, is then one chunk; the chunk
        # is sized for the element type that is actually taken.  (c0 % 4: the stem kernels store 4 channels at a time;
        # N % 8: whole 128-row tiles on the 4 x 4 maps - N = 0 passes: unchanged from before)
        h_shapes = f16 and self.f16_buffers and self._f16_patches_ok(P) and self._f16_growth_ok() and c0 % 4 == 0 and \
            N % 8 == 0 and self._f16_maps_ok(P)
        chunk = self._auto_chunk(P, N, 2 if h_shapes else 4)

        def whole_groups(g):
            # chunks of whole groups of g spots whose element offsets fit the 32 bits the LDS-DMA kernels index with
            lim = min((2 ** 31 - 1) // (s * s * max(mid, c_total)) for (_, _, _, c_total), s in zip(self._blocks, sizes))
            return max(g, min(chunk, lim) // g * g)
        if not f16 and self.atonce is None and 128 <= chunk < N:
            # fp32 path, a batch that goes through in chunks anyway: chunks of whole groups of 128 spots - every map then has
            # whole 128-row tiles even for 7 x 7 maps (224-px patches: the reference's own geometry).  Otherwise every launch
            # falls back to the generic kernels (conv1x1_kernel / conv3x3_pipe_kernel: 0.69 / 0.72 of the matrix peak against
            # 0.78 / 0.89).
            chunk = whole_groups(128)
        if f16 and self.atonce is None and chunk >= 8:
            # whole 128-row tiles; the fused path indexes with 64 bits, the two-kernel one (its DMA kernels) with 32
            chunk = chunk // 8 * 8 if (fused_ok and h_shapes) else whole_groups(8)
        # config 5 with fp16 BLOCK BUFFERS: the concatenated features live in HBM as fp16 (as under the reference's autocast),
        # every kernel of the chain reads / writes halves.  Taken when every launch of the call has a shape those kernels take.
        use_h = h_shapes and chunk % 8 == 0 and \
            (fused_ok or all(min(chunk, N) * s * s * max(mid, c_total) < 2 ** 31
                             for (_, _, _, c_total), s in zip(self._blocks, sizes)))
        return chunk, use_h, use_h and fused_ok

    def _skip_empty_shapes(self, x, P):
        """Whether an eval forward over the patches `x` can go through the indexed entry points: fp32 block buffers, the
        geometry and alignment the fused stem takes (gnx_conv_stem_bnrelu_maxpool_idx / _u8_idx), power-of-two maps."""
        c0 = self.features.conv0.out_channels
        hs, sizes = self._geometry(P)
        return (self.mfma == 'f32' and not self.small_inputs and P in (128, 256) and c0 <= 64 and c0 % 4 == 0 and
                self.features.conv0.kernel_size == (7, 7) and all(s in (4, 8, 16, 32, 64) for s in sizes) and
                all(c_total % 4 == 0 for _, _, _, c_total in self._blocks) and
                x.data_ptr() % (4 if x.dtype == torch.uint8 else 16) == 0)

    def _compact_empty(self, x, N, P, chunk):
        """The empty-spot lists of the patches `x` when this call evaluates them once (skip_empty; compacted_spots says
        whether and how many spots then run), else None.  Costs one scan of the batch (early exit at a spot's first non-zero
        slab) and ONE host read, of the two counts - which a stream capture cannot do: a captured call runs every spot."""
        if not self.skip_empty or N <= EMPTY_GRANULE or not self._skip_empty_shapes(x, P) or \
                torch.cuda.is_current_stream_capturing():
            return None
        lists = empty_spot_lists(x)
        if lists is None:
            return None
        fg, bg, counts = lists
        n_fg = int(counts[0].item())                            # the host waits here for the scan
        n = compacted_spots(N, n_fg, chunk)
        return None if n is None else SimpleNamespace(fg=fg, bg=bg, n_fg=n_fg, n=n)

    @torch.no_grad()
    def _forward_eval(self, x):
        # uint8 patches stay uint8 up to the stem kernel's operand load (a quarter of the bytes over PCIe and out of HBM)
        x = x.contiguous() if x.dtype == torch.uint8 else x.contiguous().float()
        N, _, P, _ = x.shape
        chunk, use_h, fused = self._eval_plan(N, P)
        empty = self._compact_empty(x, N, P, chunk)             # the empty spots' lists when the call skips them, else None
        Nc = N if empty is None else empty.n                    # spots that go through the kernels
        if empty is not None:
            chunk = self._eval_plan(Nc, P)[0]
        self._skipped_empty = 0 if empty is None else N - Nc    # introspection (tests, bench)
        self._used_f16_buffers, self._used_f16_fused = use_h, fused      # introspection (tests, bench)
        self._two_range_blocks = 0                              # ... dense blocks (per chunk) that ran as two ranges
        f32, mid = self.mfma == 'f32', self.bn_size * self.growth_rate
        w = SimpleNamespace(                                    # the derived weights this call reads, built in this order
            fold=self._folded_eval(), w2=self._repacked_conv2(),
            w2u=self._winograd_conv2() if (self.winograd and f32) else None,
            w2h=self._repacked_conv2_f16() if not f32 else None,
            w1s=self._split_conv1() if (self.split_conv1 and f32 and mid == 128) else None,
            w2s=self._split_conv2() if (self.split_conv2 and f32 and mid == 128 and self.growth_rate == 32) else None,
            w1h=self._conv1_f16() if (use_h and not fused) else None,
            dlp=self._dense_f16_packed() if fused else None)
        dev = x.device
        hs, sizes = self._geometry(P)
        if fused:
            # channel-blocked block buffers [c_total / 32][rows][32] (include/gridnext_hip.h: gnx_dense_layer_f16): the 32
            # channels a layer's K-loop stage needs of consecutive pixels are contiguous memory
            bufs = [torch.empty((c_total // 32, chunk * s * s, 32), device=dev, dtype=torch.float16)
                    for (_, _, _, c_total), s in zip(self._blocks, sizes)]
        else:
            bufs = [torch.empty((chunk * s * s, c_total), device=dev, dtype=torch.float16 if use_h else F32)
                    for (_, _, _, c_total), s in zip(self._blocks, sizes)]
        bott = torch.empty((1 if fused else chunk * sizes[0] * sizes[0], mid), device=dev, dtype=F32)
        stem_out = None                                         # conv0 map: only the unfused stem needs it
        feats = torch.empty((N, self.num_features), device=dev, dtype=F32)
        w0 = self.features.conv0.weight.detach().contiguous()
        st = L.stream()
        for s0 in range(0, Nc, chunk):
            n = min(chunk, Nc - s0)
            xs = x[s0:s0 + n] if empty is None else x           # (compacted: the stem reads the chunk's spots through the list)
            src = None if empty is None else empty.fg[s0:s0 + n]
            for bi, ((c_in, layers, trans, c_total), s) in enumerate(zip(self._blocks, sizes)):
                nxt = bufs[bi + 1] if trans is not None else None
                if fused:
                    self._block_f16(bi, bufs[bi], nxt, xs, n, s, P, w.fold.__getitem__, w.dlp, st)
                    continue
                rows = bufs[bi][:n * s * s]
                if bi == 0:
                    stem_out = self._stem_eval(xs, rows, c_total, P, hs, use_h, w.fold, w0, stem_out, chunk, st, src, n)
                if not self._block_ranges_eval(layers, rows, c_total, c_in, n, s, w, bott, st):
                    for li, layer in enumerate(layers):
                        self._layer_eval(layer, rows, c_total, c_in + li * self.growth_rate, n, s, use_h, w, bott, st)
                if trans is not None:
                    self._transition_eval(trans, rows, nxt, c_total, n, s, use_h, w.fold, st)
            if empty is None:
                self._tail_eval(bufs[-1], feats[s0:], n, sizes[-1], use_h, fused, w.fold[self.features.norm_final], st)
            elif s0 <= empty.n_fg:
                # the non-empty spots' features go back to their spots, the first empty spot's to its own: entries
                # [0, n_fg] of the list (what follows is padding: more copies of that empty spot)
                scf, shf = w.fold[self.features.norm_final]
                L.call('gnx_bnrelu_avgpool_idx', L.ptr(bufs[-1]), bufs[-1].shape[1], L.ptr(feats), self.num_features,
                       min(n, empty.n_fg + 1 - s0), self.num_features, sizes[-1] ** 2, L.ptr(scf), L.ptr(shf),
                       L.ptr(src, torch.int32), N, st)
        if empty is not None:                                   # ... and every other empty spot gets that row
            L.call('gnx_spot_broadcast_rows', L.ptr(feats), self.num_features, N, self.num_features,
                   L.ptr(empty.bg, torch.int32), N - empty.n_fg, st)
        if not self.classify:
            return feats
        return GF.linear(feats, self.classifier.weight.detach(), self.classifier.bias.detach())

    def _block_ranges_eval(self, layers, rows, c_total, c_in, n, s, w, bott, st):
        """Every layer of one dense block of the fp32 eval forward over `n` spots as two row ranges on two streams
        (gnx_dense_block_ranges), where `block_ranges` splits the block: True when the block ran this way, False: the caller runs
        it layer by layer.  The launches are the ones `dense_layer_f32_act` makes, per range.  Not under the opt-in split forms, and
        not while the stream is capturing: a captured step keeps one chain of whole-block launches."""
        if not self.two_ranges or self.mfma != 'f32' or w.w1s is not None or w.w2s is not None or \
                torch.cuda.is_current_stream_capturing():
            return False
        m0 = block_ranges(n, s, self.range_rows)
        if not m0:
            return False
        M, mid, g = n * s * s, self.bn_size * self.growth_rate, self.growth_rate
        items = (L.struct('gnx_dense_layer_item') * len(layers))()
        for li, (a, layer) in enumerate(zip(items, layers)):
            bn1, bn2 = w.fold[layer.norm1], w.fold[layer.norm2]
            a.W1, a.W2r = L.ptr(layer.conv1.weight), L.ptr(w.w2[layer])
            a.W2u = L.ptr(w.w2u[layer]) if (w.w2u is not None and s >= 8) else None      # (4 x 4 measured faster direct)
            a.scale1, a.shift1, a.scale2, a.shift2 = L.ptr(bn1[0]), L.ptr(bn1[1]), L.ptr(bn2[0]), L.ptr(bn2[1])
            a.cin, a.pad = c_in + li * g, 0
        t0 = self._probe_begin()
        L.call('gnx_dense_block_ranges', L.ptr(rows), c_total, L.ptr(bott), M, m0, s, mid, g, ctypes.addressof(items),
               len(layers), st)
        cins = sum(c_in + li * g for li in range(len(layers)))
        self._probe_mark('dense_block_ranges', t0, 2 * M * mid * (cins + 9 * g * len(layers)),
                         4 * M * (cins + len(layers) * (2 * mid + g)))
        self._two_range_blocks += 1
        return True

    def _layer_eval(self, layer, rows, c_total, cin, n, s, use_h, w, bott, st):
        """One dense layer of the unfused eval forward over `n` spots of the block buffer `rows` [n * s * s][c_total]: its
        `growth_rate` new columns start at `cin`.  `w`: the call's derived weights; `bott`: the bottleneck scratch."""
        M, mid, g = n * s * s, self.bn_size * self.growth_rate, self.growth_rate
        bn1, bn2 = w.fold[layer.norm1], w.fold[layer.norm2]
        if self.mfma == 'f32':
            dense_layer_f32_act(self, layer, rows, c_total, cin, bott, M, s, bn1, bn2, w.w2[layer], w.w1s, w.w2s, w.w2u, st)
            return
        H = torch.float16
        bott16 = bott.view(H)                                   # the same memory as [rows][2 mid] halves
        dma = use_h or self._f16_dma_ok(M, s, mid, c_total)
        eb, em = (2 if use_h else 4), (2 if dma else 4)         # bytes per block-buffer / bottleneck element
        t0 = self._probe_begin()
        if use_h:
            L.call('gnx_conv1x1_bnrelu_h16', L.ptr(rows, H), c_total, L.ptr(w.w1h[layer], H), L.ptr(bott16, H), mid, M, mid,
                   cin, L.ptr(bn1[0]), L.ptr(bn1[1]), L.ptr(bn2[0]), L.ptr(bn2[1]), st)
        elif dma:
            # fp16 bottleneck: conv1 stores it activated and rounded, conv2 streams it by DMA.  The choice depends on the map
            # size and channel counts only (128 | M holds for every whole spot)
            L.call('gnx_conv1x1_bnrelu_f16_act16', L.ptr(rows), c_total, L.ptr(layer.conv1.weight), L.ptr(bott16, H), mid, M,
                   mid, cin, L.ptr(bn1[0]), L.ptr(bn1[1]), L.ptr(bn2[0]), L.ptr(bn2[1]), st)
        else:
            L.call('gnx_conv1x1_bnrelu_f16', L.ptr(rows), c_total, L.ptr(layer.conv1.weight), L.ptr(bott), mid, M, mid, cin,
                   L.ptr(bn1[0]), L.ptr(bn1[1]), 0, 0, st)
        t1 = self._probe_mark('conv1x1', t0, 2 * M * cin * mid, M * (cin * eb + mid * em))
        if use_h:
            L.call('gnx_conv3x3_f16_dma_h', L.ptr(bott16, H), mid, L.ptr(w.w2h[layer], H), rows.data_ptr() + 2 * cin, c_total,
                   M, g, mid, s, st)
        elif dma:
            L.call('gnx_conv3x3_f16_dma', L.ptr(bott16, H), mid, L.ptr(w.w2h[layer], H), rows.data_ptr() + 4 * cin, c_total,
                   M, g, mid, s, st)
        else:
            L.call('gnx_conv3x3_bnrelu_f16', L.ptr(bott), mid, L.ptr(w.w2[layer]), rows.data_ptr() + 4 * cin, c_total, M, g,
                   mid, s, L.ptr(bn2[0]), L.ptr(bn2[1]), st)
        self._probe_mark('conv3x3', t1, 2 * M * 9 * mid * g, M * (mid * em + g * eb))

    def _transition_eval(self, trans, rows, nxt, c_total, n, s, use_h, fold, st):
        """norm -> relu -> 2x2 mean -> 1x1 conv of the block buffer `rows` into the first columns of the next one, `nxt`.
        Transitions are HBM-bound (4x the input bytes of their output): the fp32 wave-specialised kernel serves both matrix
        precisions."""
        H = torch.float16
        so = s // 2
        sct, sht = fold[trans.norm]
        cout = trans.conv.out_channels
        if use_h and c_total % 32 == 0:
            # two steps: norm -> relu -> 2x2 mean in one pass over the block buffer (16-B accesses), then the 1x1 conv on the
            # pooled rows without prologue or consumer activation
            pooled = torch.empty((n * so * so, c_total), device=rows.device, dtype=H)
            L.call('gnx_bnrelu_avgpool2_h16', L.ptr(rows, H), c_total, L.ptr(pooled, H), c_total, n, c_total, s, L.ptr(sct),
                   L.ptr(sht), st)
            L.call('gnx_conv1x1_bnrelu_h16', L.ptr(pooled, H), c_total, L.ptr(self._trans_f16()[trans], H), L.ptr(nxt, H),
                   nxt.shape[1], n * so * so, cout, c_total, None, None, None, None, st)
        elif use_h:
            L.call('gnx_conv1x1_bnrelu_f16_h', L.ptr(rows, H), c_total, L.ptr(trans.conv.weight), L.ptr(nxt, H), nxt.shape[1],
                   n * so * so, cout, c_total, L.ptr(sct), L.ptr(sht), None, None, 1, s, st)
        else:
            L.call('gnx_conv1x1_bnrelu', L.ptr(rows), c_total, L.ptr(trans.conv.weight), L.ptr(nxt), nxt.shape[1], n * so * so,
                   cout, c_total, L.ptr(sct), L.ptr(sht), 1, s, st)

    def _tail_eval(self, buf, feats, n, s, use_h, fused, sf, st):
        """norm_final (folded: `sf`) -> relu -> global average of the last block buffer's `n` spots into the rows of `feats`."""
        name = 'gnx_bnrelu_avgpool_h16_cb' if fused else ('gnx_bnrelu_avgpool_h16' if use_h else 'gnx_bnrelu_avgpool')
        c = self.num_features
        L.call(name, L.ptr(buf, torch.float16 if use_h else F32), buf.shape[1], L.ptr(feats), c, n, c, s * s, L.ptr(sf[0]),
               L.ptr(sf[1]), st)


def dense_layer_f32_act(model, layer, buf, ld, cin, bott, M, s, bn1, bn2, w2r, w1s, w2s, w2u, st):
    """One dense layer of the fp32 path whose norm2 map is known before conv1 runs (running statistics): conv1 with
    norm1 -> relu1 on its operand load stores the bottleneck `bott` ACTIVATED (norm2 -> relu2 on its store), then conv2 takes
    that operand as it lies in HBM (global -> LDS DMA, no prologue) and writes columns [cin, cin + growth) of the block
    buffer `buf` [M][ld].  bn1 / bn2: (scale, shift, ...) device vectors; w2r: the tap-major conv2 weight of `layer`;
    w1s / w2s / w2u: the model's split conv1 / split conv2 / Winograd weight tables, or None where that form is off.
    Shared by the eval forward and the taped forward of densenet_train."""
    mid, g = model.bn_size * model.growth_rate, model.growth_rate
    t0 = model._probe_begin()
    # (opt-in) the same product on split bf16 operands; shapes it declines keep the fp32 instruction
    if w1s is None or not L.try_call('gnx_conv1x1_bnrelu_act_split', L.ptr(buf), ld, w1s[layer].data_ptr(), L.ptr(bott), mid,
                                     M, cin, L.ptr(bn1[0]), L.ptr(bn1[1]), L.ptr(bn2[0]), L.ptr(bn2[1]), st):
        L.call('gnx_conv1x1_bnrelu_act', L.ptr(buf), ld, L.ptr(layer.conv1.weight), L.ptr(bott), mid, M, mid, cin,
               L.ptr(bn1[0]), L.ptr(bn1[1]), L.ptr(bn2[0]), L.ptr(bn2[1]), st)
    t1 = model._probe_mark('conv1x1', t0, 2 * M * cin * mid, 4 * M * (cin + mid))
    # conv2: (opt-in) nine shifted products of split bf16 operands, or Winograd F(2,3) along x (1.5x fewer matrix
    # operations, rounding-level differences) for maps of 8 x 8 and up (4 x 4 measured faster direct), or the direct form;
    # each declines shapes it does not take.  The choice depends on the map size only - never on how many spots a call or a
    # chunk holds - so chunked and unchunked evaluation stay bit-identical.
    out = buf.data_ptr() + 4 * cin
    if not ((w2s is not None and L.try_call('gnx_conv3x3_split', L.ptr(bott), mid, w2s[layer].data_ptr(), out, ld, M, s, st)) or
            (w2u is not None and s >= 8 and L.try_call('gnx_conv3x3_winograd', L.ptr(bott), mid, L.ptr(w2u[layer]), out, ld,
                                                       M, g, mid, s, st))):
        L.call('gnx_conv3x3_bnrelu', L.ptr(bott), mid, L.ptr(w2r), out, ld, M, g, mid, s, None, None, st)
    model._probe_mark('conv3x3', t1, 2 * M * 9 * mid * g, 4 * M * (mid + g))
