"""Empty spots of the DenseNet eval forward (DenseNet.skip_empty): the scan / compaction kernel, the indexed stem, and the
compacted forward against the uncompacted one.

Criterion for the forward: bit for bit (`torch.equal`).  A row's sums do not depend on the row's position in a launch or on
how many rows the launch has, only on which kernel the launch picks; the compacted count keeps N's remainder modulo 8
(densenet.compacted_spots), so every launch keeps its kernel.  Each comparison prints its largest difference first."""
import contextlib
import io
import warnings

import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _empty_reference(x):
    """(fg_idx, bg_idx) by torch: a spot is empty iff all its bytes are zero."""
    raw = x.reshape(x.shape[0], -1)
    raw = raw.view(torch.int32) if x.dtype == torch.float32 else raw
    empty = ~(raw != 0).any(1)
    idx = torch.arange(x.shape[0], device=x.device, dtype=torch.int32)
    return idx[~empty], idx[empty]


def _check_lists(x):
    from gridnext_amd.densenet import empty_spot_lists
    N = x.shape[0]
    runs = []
    for _ in range(2):
        fg, bg, counts = empty_spot_lists(x)
        runs.append((fg.clone(), bg[:int(counts[1])].clone(), counts.clone()))
    rf, rb = _empty_reference(x)
    fg, bg, counts = runs[0]
    n_fg, n_bg = counts.tolist()
    assert (n_fg, n_bg) == (rf.numel(), rb.numel()) and n_fg + n_bg == N
    assert torch.equal(fg[:n_fg], rf) and torch.equal(bg, rb)              # ascending spot order
    fill = int(rb[0]) if n_bg else 0
    assert torch.equal(fg[n_fg:], torch.full((N - n_fg,), fill, device=x.device, dtype=torch.int32))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                            # identical over two runs
    return n_fg, n_bg


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_scan_and_compaction_against_torch(dtype):
    """gnx_spot_compact on 128-px patches, float32 and uint8: a mixed batch whose size is not a multiple of 8 (and larger
    than the compaction's 1024-spot rounds), no empty spot, all empty, a spot whose only non-zero byte is its last one, and
    for floats -0.0 and NaN (bitwise non-zero: not empty)."""
    gen = torch.Generator(device=DEV).manual_seed(3)
    P = 128

    def batch(n):
        if dtype == torch.uint8:
            return torch.randint(1, 256, (n, 3, P, P), device=DEV, generator=gen, dtype=torch.uint8)
        return torch.rand((n, 3, P, P), device=DEV, generator=gen) + 0.5

    x = batch(1101)
    keep = torch.rand(1101, device=DEV, generator=gen) > 0.3
    keep[0], keep[1100] = False, False
    x *= keep.view(-1, 1, 1, 1).to(dtype)
    n_fg, n_bg = _check_lists(x)
    assert n_bg == int((~keep).sum()) and n_fg == int(keep.sum())
    assert _check_lists(batch(43)) == (43, 0)                               # no empty spot
    assert _check_lists(torch.zeros((43, 3, P, P), device=DEV, dtype=dtype)) == (0, 43)      # all empty
    x = torch.zeros((21, 3, P, P), device=DEV, dtype=dtype)
    x[5, 2, P - 1, P - 1] = 1                                               # the last byte(s) of the spot only
    x[9, 0, 0, 0] = 3                                                       # the first
    x[20, 1, 64, 7] = 1                                                     # somewhere inside
    expect = {5, 9, 20}
    if dtype == torch.float32:
        x[2, 1, 77, 3] = -0.0
        x[13, 2, 100, 100] = float('nan')
        expect |= {2, 13}
        raw = torch.zeros(3 * P * P, dtype=torch.int32)
        raw[-1] = 1 << 24                                                   # the very last BYTE of the spot (a denormal float)
        x[17] = raw.view(torch.float32).reshape(3, P, P).to(DEV)
        expect.add(17)
    assert _check_lists(x) == (len(expect), 21 - len(expect))
    from gridnext_amd.densenet import empty_spot_lists
    fg, _, counts = empty_spot_lists(x)
    assert set(fg[:int(counts[0])].tolist()) == expect


@pytest.mark.parametrize("u8,norm", [(False, False), (True, False), (True, True)])
def test_indexed_stem_equals_the_plain_stem_on_a_gathered_copy(u8, norm):
    """gnx_conv_stem_bnrelu_maxpool_idx / _u8_idx on 128-px patches through a list (unordered, with repeats) == the plain
    entry point on the gathered patches, bit for bit; float, uint8, uint8 with Normalize."""
    from gridnext_amd import _lib as L
    gen = torch.Generator(device=DEV).manual_seed(11)
    P, O, ld, n_src = 128, 64, 96, 37
    if u8:
        x = torch.randint(0, 256, (n_src, 3, P, P), device=DEV, generator=gen, dtype=torch.uint8)
    else:
        x = torch.randn((n_src, 3, P, P), device=DEV, generator=gen)
    x[4] = 0
    w = torch.randn((O, 3, 7, 7), device=DEV, generator=gen) * 0.1
    sc = torch.rand(O, device=DEV, generator=gen) + 0.5
    sh = torch.randn(O, device=DEV, generator=gen) * 0.1
    nrm = torch.tensor([0.485, 0.456, 0.406, 0.229, 0.224, 0.225, 1 / 0.229, 1 / 0.224, 1 / 0.225], device=DEV) if norm else None
    src = torch.tensor([36, 4, 4, 0, 17, 3, 36, 22, 9, 4, 30, 1, 2, 8, 35, 34, 4, 19, 20, 21, 5], device=DEV, dtype=torch.int32)
    n = src.numel()
    rows = n * (P // 4) ** 2
    out_idx = torch.full((rows, ld), -7.0, device=DEV)
    out_ref = torch.full((rows, ld), -7.0, device=DEV)
    xg = x[src.long()].contiguous()
    st = L.stream()
    tail = (L.ptr(sc), L.ptr(sh))
    if u8:
        L.call('gnx_conv_stem_bnrelu_maxpool_u8', xg.data_ptr(), L.ptr(w), out_ref.data_ptr(), ld, n, 3, P, P, O, 7, 7, 2, 3, *tail,
               L.ptr(nrm), 0, st)
        L.call('gnx_conv_stem_bnrelu_maxpool_u8_idx', x.data_ptr(), L.ptr(w), L.ptr(out_idx), ld, n, 3, P, P, O, 7, 7, 2, 3, *tail,
               L.ptr(nrm), L.ptr(src, torch.int32), n_src, st)
    else:
        L.call('gnx_conv_stem_bnrelu_maxpool', L.ptr(xg), L.ptr(w), L.ptr(out_ref), ld, n, 3, P, P, O, 7, 7, 2, 3, *tail, st)
        L.call('gnx_conv_stem_bnrelu_maxpool_idx', L.ptr(x), L.ptr(w), L.ptr(out_idx), ld, n, 3, P, P, O, 7, 7, 2, 3, *tail,
               L.ptr(src, torch.int32), n_src, st)
    assert float(out_ref[:, :O].abs().sum()) > 0 and bool((out_ref[:, O:] == -7.0).all())
    assert torch.equal(out_idx, out_ref)


def _densenet121(C=8):
    import gridnext_amd as ga
    from oracle import densenet as odn
    torch.manual_seed(0)
    return ga.DenseNet(num_classes=C, **odn.DENSENET121).to(DEV).eval()


def _both(f, x, atonce=None):
    """(rows with skip_empty, rows without, spots the compacted call skipped)"""
    with torch.no_grad():
        f.skip_empty, f.atonce = True, atonce
        on = f(x)
        skipped = f._skipped_empty
        f.skip_empty, f.atonce = False, None
        off = f(x)
        assert f._skipped_empty == 0
    f.skip_empty = True
    print("skip_empty on vs off: %d spots, %d skipped, max |d| %.3e" % (x.shape[0], skipped, (on - off).abs().max().item()))
    return on, off, skipped


def _zero_rows(f, P, dtype):
    """What a batch of 8 all-zero patches gives when run on its own, every spot through every kernel."""
    with torch.no_grad():
        f.skip_empty = False
        z = f(torch.zeros((8, 3, P, P), device=DEV, dtype=dtype))
        f.skip_empty = True
    assert torch.equal(z, z[:1].expand_as(z))
    return z[0]


def _patches(n, empty_share, gen, u8=False, P=128):
    if u8:
        x = torch.randint(0, 256, (n, 3, P, P), device=DEV, generator=gen, dtype=torch.uint8)
    else:
        x = torch.rand((n, 3, P, P), device=DEV, generator=gen)
    empty = torch.rand(n, device=DEV, generator=gen) < empty_share
    x *= (~empty).view(-1, 1, 1, 1).to(x.dtype)
    return x, empty


def test_densenet121_compacted_forward_equals_the_uncompacted_one():
    """DenseNet-121, eval, 128-px float patches with zero background: (a) a few hundred spots (8 | N, and N = 301), (c)
    `atonce` chunks, (d) all empty, (e) no empty spot, (f) so few empty spots that the padding eats the saving (path not
    taken).  Bit for bit, and every background row == the row of all-zero patches run on their own with the switch off."""
    f = _densenet121()
    gen = torch.Generator(device=DEV).manual_seed(21)
    zrow = _zero_rows(f, 128, torch.float32)
    for n in (304, 301):                                       # (a)
        x, empty = _patches(n, 0.2, gen)
        on, off, skipped = _both(f, x)
        assert skipped >= 8 and (n - skipped) % 8 == n % 8
        assert torch.equal(on, off)
        assert torch.equal(on[empty], zrow.expand(int(empty.sum()), -1))
    x, empty = _patches(304, 0.3, gen)                         # (c): chunks of 64 compacted spots, the last one shorter
    on, off, skipped = _both(f, x, atonce=64)
    assert skipped >= 8 and torch.equal(on, off)
    assert torch.equal(on[empty], zrow.expand(int(empty.sum()), -1))
    f.classify = False                                        # the scattered features themselves
    on_f, off_f, _ = _both(f, x)
    f.classify = True
    assert on_f.shape == (304, f.num_features) and torch.equal(on_f, off_f)
    x = torch.zeros((304, 3, 128, 128), device=DEV)            # (d)
    on, off, skipped = _both(f, x)
    assert skipped == 296 and torch.equal(on, off) and torch.equal(on, zrow.expand(304, -1))
    x, _ = _patches(304, 0.0, gen)                             # (e)
    x += 0.01
    on, off, skipped = _both(f, x)
    assert skipped == 0 and torch.equal(on, off)
    x[[7, 100, 303]] = 0                                       # (f): 301 non-empty + 1 -> 304 after padding
    on, off, skipped = _both(f, x)
    assert skipped == 0 and torch.equal(on, off)
    assert torch.equal(on[[7, 100, 303]], zrow.expand(3, -1))


def test_densenet121_uint8_normalize_compacted_forward():
    """(g) uint8 patches with a fused Normalize: the empty spots' zero bytes become -mean / std inside the stem - equal
    bytes in, equal row out."""
    f = _densenet121()
    f.input_norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    gen = torch.Generator(device=DEV).manual_seed(22)
    x, empty = _patches(304, 0.25, gen, u8=True)
    on, off, skipped = _both(f, x)
    assert skipped >= 8 and torch.equal(on, off)
    zrow = _zero_rows(f, 128, torch.uint8)
    assert torch.equal(on[empty], zrow.expand(int(empty.sum()), -1))
    f.input_norm = None                                        # ToTensor only
    on, off, skipped = _both(f, x)
    assert skipped >= 8 and torch.equal(on, off)


def test_densenet121_whole_array_compacted():
    """(b) one whole 78 x 64 array (4 992 spots, the benchmark's synthetic array with its zero background), in one pass and
    (c) in `atonce` chunks of 1000."""
    from gridnext_amd.synthetic import visium_array
    f = _densenet121()
    x_img, _, y = visium_array(0, 2000, 8, 128, image=True, counts=False, device=DEV)
    spots = x_img.reshape(-1, 3, 128, 128)
    bg = (y.reshape(-1) == 0)
    on, off, skipped = _both(f, spots)
    assert int(bg.sum()) == 563 and skipped == 4992 - 4432
    assert torch.equal(on, off)
    assert torch.equal(on[bg], _zero_rows(f, 128, torch.float32).expand(563, -1))
    on_c, _, skipped_c = _both(f, spots, atonce=1000)
    assert skipped_c == skipped and torch.equal(on_c, off)


def _small_mm(C=5, G=24, H=12, W=10, P=128):
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    torch.manual_seed(5)
    f = ga.DenseNet(num_classes=C, growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16, bn_size=2, small_inputs=False)
    m = ga.GridNetHexMM(f, count_mlp(G, C), (3, P, P), (G,), (H, W), C)
    for p in m.patch_classifier.parameters():
        p.requires_grad = False
    return m, f


def _small_arrays(n, C=5, G=24, H=12, W=10, P=128):
    gen = torch.Generator().manual_seed(17)
    y = torch.randint(1, C + 1, (n, H, W), generator=gen) * (torch.rand((n, H, W), generator=gen) > 0.4)
    xi = torch.rand((n, H, W, 3, P, P), generator=gen) * (y > 0).view(n, H, W, 1, 1, 1)
    xc = torch.randint(0, 10, (n, G, H, W), generator=gen).float() * (y > 0).view(n, 1, H, W)
    return xi, xc, y


def test_gridnet_forward_nhwc_with_and_without_the_switch():
    """GridNetHexMM.forward_nhwc on a 12 x 10 grid (frozen DenseNet f in eval mode, g in train mode: its BatchNorm sees the
    background rows): the logits with and without skip_empty, bit for bit."""
    m, f = _small_mm()
    m.to(DEV).train()
    m.patch_classifier.eval()
    xi, xc, y = _small_arrays(1)
    inputs = [xi.to(DEV), xc.to(DEV)]
    outs = []
    for flag in (True, False):
        f.skip_empty = flag
        with torch.no_grad():
            outs.append(m.forward_nhwc(inputs).clone())
        assert (f._skipped_empty > 0) == flag
    print("forward_nhwc on vs off: max |d| %.3e" % (outs[0] - outs[1]).abs().max().item())
    assert torch.equal(outs[0], outs[1])


def test_capture_falls_back_and_still_replays(monkeypatch):
    """GNX_GRAPH=1 with a frozen DenseNet: the step is captured into a hipGraph.  The empty-spot scan needs a host read,
    which a capture cannot hold: while capturing, the forward must run uncompacted (no failed capture), the graph must
    replay, and the loop's histories and weights equal the eager (compacted) loop's bit for bit."""
    import gridnext_amd as ga
    from gridnext_amd import graphs
    from gridnext_amd.densenet import DenseNet
    xi, xc, y = _small_arrays(6)
    data = [((xi[i].to(DEV), xc[i].to(DEV)), y[i].to(DEV)) for i in range(6)]
    replays, during_capture = [0], []
    real_replay, real_compact = graphs.GridStepGraph.replay, DenseNet._compact_empty

    def counting_replay(self, inputs, labels):
        replays[0] += 1
        return real_replay(self, inputs, labels)

    def watching_compact(self, x, N, P, chunk):
        out = real_compact(self, x, N, P, chunk)
        if torch.cuda.is_current_stream_capturing():
            during_capture.append(out)
        return out
    monkeypatch.setattr(graphs.GridStepGraph, 'replay', counting_replay)
    monkeypatch.setattr(DenseNet, '_compact_empty', watching_compact)
    results = []
    for flag in ('0', '1'):
        monkeypatch.setenv('GNX_GRAPH', flag)
        m, f = _small_mm()
        f.eval()                                               # (graphs.wanted looks at the model as the loop is entered)
        assert graphs.wanted(m.to(DEV), True, DEV) == (flag == '1')
        dl = {'train': DataLoader(data[:5], batch_size=1), 'val': DataLoader(data[5:], batch_size=1)}
        opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
        before = replays[0]
        with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter('always')
            m, vh, th = ga.train_gridwise(m, dl, nn.CrossEntropyLoss(), opt, num_epochs=2)
        assert not [str(w.message) for w in caught if 'capture failed' in str(w.message)]
        results.append((th, vh, {k: v.clone() for k, v in m.state_dict().items()}, replays[0] - before))
    (th0, vh0, sd0, r0), (th1, vh1, sd1, r1) = results
    assert r0 == 0 and r1 == 2 * 5 - graphs.WARMUP, (r0, r1)
    assert during_capture and all(c is None for c in during_capture)
    assert th0 == th1 and vh0 == vh1
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
