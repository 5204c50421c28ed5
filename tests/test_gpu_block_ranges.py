"""Dense blocks as two row ranges on two streams (gnx_dense_block_ranges, DenseNet.two_ranges): the driver alone on small
blocks, the splits it declines, its ordering against the caller's stream, its serial form under stream capture, and
DenseNet-121 with the switch on and off.

The kernels are the same on both paths; what can go wrong is the range arithmetic, the ordering and the scratch.  Criterion
everywhere: bit for bit (`torch.equal`) against the one-range path of the same build.  Block buffer and bottleneck start as
NaN, so a row nobody wrote, or a range that read the other's scratch, shows."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K0, GROWTH, MID, LAYERS = 64, 32, 128, 3            # K grows 64 -> 96 -> 128; conv1 N = 128, conv2 N = 32
LD = K0 + LAYERS * GROWTH


class _Block:
    """A three-layer dense block on `spots` spots of an S x S map: input columns, weights in every layout the launchers take,
    folded BN vectors, and the item table of the driver.  Winograd weights are passed for S >= 8, as the model does."""

    def __init__(self, S, spots, seed):
        from gridnext_amd import _lib as L
        self.L, self.S, self.M = L, S, spots * S * S
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.x = torch.randn((self.M, K0), device=DEV, generator=gen)
        self.buf = torch.empty((self.M, LD), device=DEV)
        self.bott = torch.empty((self.M, MID), device=DEV)
        self.keep = []
        self.items = (L.struct('gnx_dense_layer_item') * LAYERS)()
        st = L.stream()
        for li, a in enumerate(self.items):
            cin = K0 + li * GROWTH
            w1 = torch.randn((MID, cin), device=DEV, generator=gen) * (2.0 / cin) ** 0.5
            w2 = torch.randn((GROWTH, MID, 3, 3), device=DEV, generator=gen) * (2.0 / (9 * MID)) ** 0.5
            w2r = torch.empty((9, GROWTH, MID), device=DEV)
            w2u = torch.empty((12, GROWTH, MID), device=DEV)
            L.call('gnx_repack_conv3x3', L.ptr(w2), L.ptr(w2r), GROWTH, MID, st)
            L.call('gnx_winograd_conv3x3_weights', L.ptr(w2), L.ptr(w2u), GROWTH, MID, st)
            bn = [torch.rand(c, device=DEV, generator=gen) * s + o for c, s, o in
                  ((cin, 1.0, 0.5), (cin, 0.2, -0.1), (MID, 1.0, 0.5), (MID, 0.2, -0.1))]
            self.keep += [w1, w2, w2r, w2u] + bn
            a.W1, a.W2r, a.W2u = L.ptr(w1), L.ptr(w2r), (L.ptr(w2u) if S >= 8 else None)
            a.scale1, a.shift1, a.scale2, a.shift2 = (L.ptr(t) for t in bn)
            a.cin, a.pad = cin, 0
        torch.cuda.synchronize()

    def args(self, M0):
        L = self.L
        return (L.ptr(self.buf), LD, L.ptr(self.bott), self.M, M0, self.S, MID, GROWTH, ctypes.addressof(self.items), LAYERS,
                L.stream())

    def plan(self, M0):
        return self.L.query('gnx_dense_block_ranges_form', *self.args(M0))

    def fill(self):
        self.buf.fill_(float('nan'))
        self.bott.fill_(float('nan'))
        self.buf[:, :K0] = self.x

    def launch(self, M0):
        self.L.call('gnx_dense_block_ranges', *self.args(M0))

    def run(self, M0):
        """(block buffer, bottleneck) after one call on NaN-filled buffers"""
        self.fill()
        self.launch(M0)
        torch.cuda.synchronize()
        return self.buf.clone(), self.bott.clone()


def _codes():
    from gridnext_amd import _lib as L
    return L.CONSTANTS['GNX_BR_ONE'], L.CONSTANTS['GNX_BR_SERIAL'], L.CONSTANTS['GNX_BR_TWO']


def _check_equal(name, got, ref):
    for what, a, b in zip(('block buffer', 'bottleneck'), got, ref):
        print("%s, %s: NaN %d, rows differing %d" % (name, what, int(torch.isnan(a).sum()), int((a != b).any(1).sum())))
        assert not torch.isnan(b).any() and float(b.abs().sum()) > 0        # the reference wrote every element
        assert torch.equal(a, b)


@pytest.mark.parametrize("S,spots,spots0", [(8, 24, 12), (8, 40, 16), (4, 24, 8), (4, 16, 8)])
def test_driver_two_ranges_equal_one_range(S, spots, spots0):
    """S = 8: 24 spots as 768 + 768 rows, 40 spots as 1024 + 1536; S = 4: 24 spots as 128 + 256 rows, 16 spots as one tile per
    range.  The one-range call of the driver itself equals the launchers called one by one."""
    ONE, _, TWO = _codes()
    b = _Block(S, spots, seed=S * 100 + spots)
    L, M0 = b.L, spots0 * S * S
    assert b.plan(0) == ONE and b.plan(M0) == TWO
    ref = b.run(0)
    b.fill()                                                    # the same launches by hand
    for a in b.items:
        L.call('gnx_conv1x1_bnrelu_act', L.ptr(b.buf), LD, a.W1, L.ptr(b.bott), MID, b.M, MID, a.cin, a.scale1, a.shift1, a.scale2,
               a.shift2, L.stream())
        out = b.buf.data_ptr() + 4 * a.cin
        if S >= 8:
            L.call('gnx_conv3x3_winograd', L.ptr(b.bott), MID, a.W2u, out, LD, b.M, GROWTH, MID, S, L.stream())
        else:
            L.call('gnx_conv3x3_bnrelu', L.ptr(b.bott), MID, a.W2r, out, LD, b.M, GROWTH, MID, S, None, None, L.stream())
    torch.cuda.synchronize()
    _check_equal("by hand", (b.buf, b.bott), ref)
    _check_equal("two ranges %d + %d rows" % (M0, b.M - M0), b.run(M0), ref)


def test_driver_declines_illegal_splits_and_empty_ranges():
    """A split that leaves a range without whole 128-row tiles (or, with Winograd layers, range 0 without whole 256-pixel
    tiles) runs as ONE range - the header's choice, not an error; M0 = 0 and M0 = M are one range too: nothing is launched for
    the empty one.  M0 outside [0, M] is a bad argument."""
    ONE, _, TWO = _codes()
    b4, b8 = _Block(4, 24, seed=1), _Block(8, 24, seed=2)
    ref4, ref8 = b4.run(0), b8.run(0)
    for b, ref, M0s in ((b4, ref4, (64, 192, 320, b4.M)), (b8, ref8, (128, 640, 1408, b8.M))):
        for M0 in M0s:
            assert b.plan(M0) == ONE, (b.S, M0)
            _check_equal("S %d, M0 %d" % (b.S, M0), b.run(M0), ref)
        for M0 in (-128, b.M + 128):
            assert b.plan(M0) == b.L.CONSTANTS['GNX_ERR_BAD_ARG']
            with pytest.raises(RuntimeError, match='bad argument'):
                b.launch(M0)
    assert b4.plan(256) == TWO and b8.plan(512) == TWO          # (the legal neighbours of the splits above)
    odd = _Block(4, 20, seed=3)                                 # 320 rows: no split leaves both ranges in whole tiles
    assert all(odd.plan(M0) == ONE for M0 in range(0, odd.M + 1, 16))


@pytest.mark.parametrize("own_stream", [False, True])
def test_caller_stream_is_ordered_after_both_ranges(own_stream):
    """The driver, then at once a copy on the caller's stream of the last rows of range 1 - no device synchronisation in
    between -, 20 times over with the buffers refilled each time (the events are reused): the last copy equals the serial
    result.  Range 1 is 15 times range 0, so a missing join would read rows not yet written; a missing fork would start range 1
    on the NaN of the refill.  On the default stream and on a stream of the caller's own."""
    _, _, TWO = _codes()
    b = _Block(8, 128, seed=7)
    M0 = 8 * 64
    ref = b.run(0)[0]
    stream = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert b.plan(M0) == TWO
        for _ in range(20):
            b.fill()
            b.launch(M0)
            tail = b.buf[-256:].clone()
            head = b.buf[:256].clone()
    torch.cuda.synchronize()
    print("last rows differing: %d, first: %d" % (int((tail != ref[-256:]).any(1).sum()), int((head != ref[:256]).any(1).sum())))
    assert torch.equal(tail, ref[-256:]) and torch.equal(head, ref[:256])
    assert torch.equal(b.buf, ref)


def test_captured_call_runs_both_ranges_on_one_stream():
    """Under torch.cuda.graph the plan of a legal split is GNX_BR_SERIAL (both ranges on the capturing stream: the graph stays
    one chain), the capture succeeds, and a replay on refilled buffers gives the same bits; outside the capture the plan is
    GNX_BR_TWO again."""
    _, SERIAL, TWO = _codes()
    b = _Block(8, 24, seed=9)
    M0 = 768
    ref = b.run(0)
    _check_equal("eager", b.run(M0), ref)                       # (also: every kernel configured before the capture)
    graph = torch.cuda.CUDAGraph()
    b.fill()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        plan = b.plan(M0)
        b.launch(M0)
    assert plan == SERIAL and b.plan(M0) == TWO
    b.fill()
    graph.replay()
    torch.cuda.synchronize()
    _check_equal("replay", (b.buf, b.bott), ref)


def _densenet121(C=8):
    import gridnext_amd as ga
    from oracle import densenet as odn
    torch.manual_seed(0)
    f = ga.DenseNet(num_classes=C, **odn.DENSENET121).to(DEV).eval()
    f.range_rows = 128                                          # the test-only threshold: 32 spots reach the path
    return f


def _logits(f, x, two_ranges, skip_empty=True, atonce=None):
    f.two_ranges, f.skip_empty, f.atonce = two_ranges, skip_empty, atonce
    with torch.no_grad():
        out = f(x)
    blocks, skipped = f._two_range_blocks, f._skipped_empty
    f.two_ranges, f.skip_empty, f.atonce = False, True, None
    return out, blocks, skipped


def test_densenet121_with_and_without_two_ranges():
    """DenseNet-121, eval, 32 spots of 128 px: blocks 3 and 4 (8 x 8 and 4 x 4 maps) go through the driver with the switch on
    and through the per-layer launches with it off - equal logits; chunked (16 spots at a time) equals unchunked with the
    switch on; and with a zero background, skip_empty on equals off (the compacted batch splits 8 + 16 spots)."""
    f = _densenet121()
    gen = torch.Generator(device=DEV).manual_seed(31)
    x = torch.rand((32, 3, 128, 128), device=DEV, generator=gen)
    on, blocks, _ = _logits(f, x, True)
    off, blocks_off, _ = _logits(f, x, False)
    print("two_ranges on vs off: max |d| %.3e" % (on - off).abs().max().item())
    assert blocks == 2 and blocks_off == 0
    assert torch.equal(on, off)
    chunked, blocks_c, _ = _logits(f, x, True, atonce=16)
    assert blocks_c == 4 and torch.equal(chunked, on)
    x[torch.tensor([1, 2, 5, 8, 9, 13, 14, 20, 21, 22, 27, 30], device=DEV)] = 0       # 20 non-empty -> 24 compacted spots
    on_s, blocks_s, skipped = _logits(f, x, True, skip_empty=True)
    off_s, blocks_n, skipped_n = _logits(f, x, True, skip_empty=False)
    ref_s, _, _ = _logits(f, x, False, skip_empty=False)
    print("skip_empty on vs off under two_ranges: skipped %d, max |d| %.3e" % (skipped, (on_s - off_s).abs().max().item()))
    assert skipped == 8 and skipped_n == 0 and blocks_s == 2 and blocks_n == 2
    assert torch.equal(on_s, off_s) and torch.equal(on_s, ref_s)


def test_two_ranges_is_part_of_the_cache_key_and_the_fcache_token():
    from gridnext_amd import fcache
    f = _densenet121()
    w = [f.features.conv0.weight]
    assert f.two_ranges is False                                # opt-in
    k_off, t_off = f._key(w), fcache.classifier_state(f)[0]
    f.two_ranges = True
    assert f._key(w) != k_off and fcache.classifier_state(f)[0] != t_off
    f.two_ranges = False
    assert f._key(w) == k_off and fcache.classifier_state(f)[0] == t_off
