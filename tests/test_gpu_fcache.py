"""The frozen-classifier row cache on the device (gridnext_amd/fcache.py, GridNet.enable_f_cache) and its key, the content
fingerprint kernel (csrc/fingerprint.hip):

 1. the kernel equals tests/fingerprint_ref.py - the header's definition in numpy - BIT FOR BIT: every head / tail shape,
    every byte alignment, batches, both forms of the launch on either side of their switch, one segment past 16 MiB;
 2. a hit skips f: same logits as without the cache, the DenseNet's forward not called;
 3. what must not be served is not: other bytes, an edited / reloaded classifier, train mode, a parameter on the tape, a
    stream capture;
 4. batches with hits and misses mixed, a budget that does not hold everything, callers writing into what they were given;
 5. `train_gridwise` for 3 epochs with the cache off and on: histories and weights equal, 3 misses and 6 hits.
Every comparison is exact (torch.equal / ==): the cache returns copies of rows f itself wrote.
"""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

import fingerprint_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

BIG = 16 * 1024 * 1024 + 5          # the one large segment
_POOL = {}


def _pool():
    """BIG + 16 random bytes, on the host (numpy) and on the device, made once."""
    if not _POOL:
        host = np.random.default_rng(11).integers(0, 256, BIG + 16, dtype=np.uint8)
        host[1000:1200] = 0                                     # a run of zero words, as a background spot has
        _POOL['host'] = host
        _POOL['dev'] = torch.from_numpy(host).to(DEV)
        assert _POOL['dev'].data_ptr() % 16 == 0
    return _POOL['host'], _POOL['dev']


def _device(offset, seg_bytes, n_seg=1):
    """The kernel's fingerprints of n_seg segments of seg_bytes bytes starting `offset` bytes into the pool."""
    from gridnext_amd.fcache import device_fingerprint
    _, dev = _pool()
    return device_fingerprint(dev[offset:offset + seg_bytes * n_seg], n_seg)


def _direct(offset, seg_bytes, n_seg):
    """The same through the C ABI by hand (seg_bytes = 0 included, which a tensor view cannot express per segment)."""
    from gridnext_amd import _lib as L
    _, dev = _pool()
    out = torch.zeros((max(n_seg, 1), 2), device=DEV, dtype=torch.int64)
    ws_bytes = L.query('gnx_fingerprint128_batch_workspace', seg_bytes, n_seg)
    ws = torch.empty(max(ws_bytes // 8, 1), device=DEV, dtype=torch.int64)
    L.call('gnx_fingerprint128_batch', dev.data_ptr() + offset, seg_bytes, n_seg, out.data_ptr(), ws.data_ptr(), L.stream())
    return [(a & (2 ** 64 - 1), b & (2 ** 64 - 1)) for a, b in out.tolist()][:n_seg]


def _host(offset, seg_bytes, n_seg=1):
    host, _ = _pool()
    return [R.fingerprint128(host[offset + s * seg_bytes:offset + (s + 1) * seg_bytes].tobytes()) for s in range(n_seg)]


# ------------------------------------------------------------------------------------------------ 1. the kernel
def test_kernel_equals_the_restatement_at_every_length_and_alignment():
    """Lengths 0, 1, 7, 8, 9, 63, 64, 65, 4 095, 4 096, 4 097 at byte offsets 0 .. 7 from a 16-byte aligned base (and 8 .. 15:
    the kernel's loads are 16 bytes wide), single segments and batches of 3 whose later segments start wherever the length
    puts them."""
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097):
        for off in range(16):
            assert _direct(off, n, 1) == _host(off, n), (n, off)
            assert _direct(off, n, 3) == _host(off, n, 3), (n, off, 'batch of 3')
            if n:
                assert _device(off, n) == _host(off, n), (n, off)
    assert _direct(0, 0, 1) == [R.fingerprint128(b'')]
    assert _direct(0, 4096, 0) == []


def test_batch_of_37_segments_equals_the_37_single_calls():
    n, k = 12288, 37
    for off in (0, 5):
        batch = _device(off, n, k)
        singles = [_device(off + s * n, n)[0] for s in range(k)]
        assert batch == singles
        assert batch == _host(off, n, k)
        assert len(set(batch)) == k


def test_both_forms_on_either_side_of_the_switch():
    """Segments of up to gnx_fingerprint128_split_bytes() bytes take one workgroup and no workspace; one byte more and the
    segment is cut into parts that a second launch sums.  More than 1 024 segments always take the one-launch form."""
    from gridnext_amd import _lib as L
    split = L.query('gnx_fingerprint128_split_bytes')
    assert split == 32768
    for n, two_launches in ((split - 1, False), (split, False), (split + 1, True), (2 * split, True), (2 * split + 3, True),
                            (5 * split + 17, True)):
        assert (L.query('gnx_fingerprint128_batch_workspace', n, 1) > 0) == two_launches, n
        for off in (0, 3, 8, 13):
            assert _device(off, n) == _host(off, n), (n, off)
    # batches: 3 long segments (cut into parts), and 1 100 segments longer than the switch that still go one workgroup each
    assert L.query('gnx_fingerprint128_batch_workspace', split + 9, 3) == 3 * 2 * 16
    assert _device(1, split + 9, 3) == _host(1, split + 9, 3)
    assert L.query('gnx_fingerprint128_batch_workspace', 4097, 1100) == 0
    assert _device(2, 4097, 1100) == _host(2, 4097, 1100)
    assert L.query('gnx_fingerprint128_batch_workspace', 40000, 1024) == 1024 * 2 * 16
    assert L.query('gnx_fingerprint128_batch_workspace', 40000, 1025) == 0


def test_one_segment_of_16_mib_and_5_bytes():
    """2 048 workgroups, ~8 KiB each; the tail word holds 5 bytes."""
    assert _device(0, BIG) == _host(0, BIG)
    assert _device(7, BIG) == _host(7, BIG)


# ------------------------------------------------------------------------------------------------ the model
C, G, H, W, P, N_ARR = 5, 24, 6, 4, 64, 3


def _model(seed=5):
    import gridnext_amd as ga
    from gridnext_amd.synthetic import count_mlp
    torch.manual_seed(seed)
    f = ga.DenseNet(num_classes=C, growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16, bn_size=2, small_inputs=False)
    m = ga.GridNetHexMM(f, count_mlp(G, C), (3, P, P), (G,), (H, W), C)
    for p in m.image_classifier.parameters():
        p.requires_grad = False
    for p in m.count_classifier.parameters():
        p.requires_grad = False
    return m, f


def _arrays(n=N_ARR, u8=False):
    gen = torch.Generator().manual_seed(17)
    y = torch.randint(1, C + 1, (n, H, W), generator=gen) * (torch.rand((n, H, W), generator=gen) > 0.4)
    fg = (y > 0).view(n, H, W, 1, 1, 1)
    if u8:
        xi = torch.randint(0, 256, (n, H, W, 3, P, P), generator=gen, dtype=torch.uint8) * fg.to(torch.uint8)
    else:
        xi = torch.rand((n, H, W, 3, P, P), generator=gen) * fg
    xc = torch.randint(0, 10, (n, G, H, W), generator=gen).float() * (y > 0).view(n, 1, H, W)
    return xi, xc, y


def _ready(m):
    """The grid loop's train phase: g trains, the image f is in eval mode, the count f is left in train mode."""
    m.to(DEV).train()
    m.patch_classifier.eval()
    return m


def _count_calls(f):
    calls = [0]
    real = f.forward

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    f.forward = counting
    return calls


def _inputs(xi, xc, idx):
    return [xi[idx].to(DEV).contiguous(), xc[idx].to(DEV).contiguous()]


def test_hit_skips_f():
    """forward_nhwc, cache off, then on: first pass all misses, second pass all hits, each torch.equal to the uncached
    logits; on the hit pass the DenseNet's forward is not called.  (The count classifier is in train mode, as in the train
    phase of the loop: its calls are bypassed.)"""
    m, f = _model()
    _ready(m)
    xi, xc, _ = _arrays()
    batches = [_inputs(xi, xc, slice(i, i + 1)) for i in range(N_ARR)]
    assert m.f_cache is None
    off = [m.forward_nhwc(b).detach().clone() for b in batches]
    calls = _count_calls(f)
    m.enable_f_cache()
    img, cnt = m.image_f_cache, m.count_f_cache
    first = [m.forward_nhwc(b).detach().clone() for b in batches]
    assert calls[0] == N_ARR and (img.hits, img.misses, img.bypassed) == (0, N_ARR, 0)
    second = [m.forward_nhwc(b).detach().clone() for b in batches]
    assert calls[0] == N_ARR, "the hit pass called f"
    assert (img.hits, img.misses, img.bypassed) == (N_ARR, N_ARR, 0) and len(img) == N_ARR
    assert (cnt.hits, cnt.misses, cnt.bypassed) == (0, 0, 2 * N_ARR)
    for a, b, c in zip(off, first, second):
        assert torch.equal(a, b) and torch.equal(a, c)
    m.disable_f_cache()
    assert m.f_cache is None and m.image_f_cache is None
    again = m.forward_nhwc(batches[0]).detach()
    assert calls[0] == N_ARR + 1 and torch.equal(again, off[0])


def _pp(m, batch):
    with torch.no_grad():
        return m.patch_predictions(batch).clone()


def test_invalidation():
    """Other bytes are another entry; an in-place parameter edit, a running-statistic edit and load_state_dict each force
    misses, and the rows are those of the changed network."""
    m, f = _model()
    m.to(DEV).eval()
    xi, xc, _ = _arrays(1)
    a = _inputs(xi, xc, slice(0, 1))
    b = [a[0].clone(), a[1]]
    raw = b[0].view(torch.uint8).reshape(-1)
    raw[raw.numel() // 2 + 1] ^= 1                              # one bit of one byte of the image array
    m.enable_f_cache()
    img, cnt = m.image_f_cache, m.count_f_cache
    _pp(m, a), _pp(m, b)
    assert (img.hits, img.misses, len(img)) == (0, 2, 2)
    assert (cnt.hits, cnt.misses, len(cnt)) == (1, 1, 1)        # the count grids are the same bytes
    _pp(m, a), _pp(m, b)
    assert (img.hits, img.misses) == (2, 2)

    def changed_network_check(edit):
        misses = img.misses
        edit()
        got = _pp(m, a)
        assert img.misses == misses + 1 and len(img) == 1, "the cache survived the edit"
        caches = (m.image_f_cache, m.count_f_cache)
        m.disable_f_cache()
        want = _pp(m, a)
        m.image_f_cache, m.count_f_cache = caches
        m.f_cache = caches[0]
        assert torch.equal(got, want)
        assert torch.equal(_pp(m, a), want) and img.misses == misses + 1
        return want

    base = _pp(m, a)

    def edit_parameter():
        with torch.no_grad():
            f.features.conv0.weight.mul_(1.25)
    r1 = changed_network_check(edit_parameter)
    assert not torch.equal(r1, base)
    r2 = changed_network_check(lambda: f.features.norm0.running_mean.add_(0.05))
    assert not torch.equal(r2, r1)

    def reload():
        sd = {k: v.clone() for k, v in f.state_dict().items()}
        sd['classifier.weight'] *= 0.5
        f.load_state_dict(sd)
    r3 = changed_network_check(reload)
    assert not torch.equal(r3, r2)


def test_train_mode_and_requires_grad_bypass():
    """f.train(): the call is bypassed and f's running statistics move exactly as without the cache.  A parameter that
    requires grad: bypassed."""
    m, f = _model()
    m.to(DEV).eval()
    xi, xc, _ = _arrays(1)
    a = _inputs(xi, xc, slice(0, 1))
    start = {k: v.clone() for k, v in f.state_dict().items()}
    f.train()
    want = _pp(m, a)
    moved = {k: v.clone() for k, v in f.state_dict().items()}
    assert not torch.equal(moved['features.norm0.running_mean'], start['features.norm0.running_mean'])
    f.load_state_dict(start)
    f.train()
    m.enable_f_cache()
    img = m.image_f_cache
    got = _pp(m, a)
    assert (img.hits, img.misses, img.bypassed, len(img)) == (0, 0, 1, 0)
    assert torch.equal(got, want)
    for k, v in f.state_dict().items():
        assert torch.equal(v, moved[k]), k
    # one submodule in train mode is enough
    f.eval()
    f.features.norm_final.train()
    _pp(m, a)
    assert (img.misses, img.bypassed) == (0, 2)
    f.eval()
    f.classifier.bias.requires_grad = True
    m.disable_f_cache()
    want = m.patch_predictions(a).detach().clone()
    m.enable_f_cache()
    img = m.image_f_cache
    got = m.patch_predictions(a).detach().clone()
    assert (img.hits, img.misses, img.bypassed) == (0, 0, 1) and torch.equal(got, want)
    f.classifier.bias.requires_grad = False
    _pp(m, a)
    assert (img.misses, img.bypassed) == (1, 1)


def test_stream_capture_bypasses():
    """The lookup reads back to the host, which a capture cannot hold: while capturing, f is computed as ever (even for an
    array the cache holds), the capture succeeds and replays to the uncached result."""
    m, f = _model()
    m.to(DEV).eval()
    xi, xc, _ = _arrays(1)
    a = _inputs(xi, xc, slice(0, 1))
    want = _pp(m, a)                                            # (also sizes f's derived tensors outside the capture)
    m.enable_f_cache()
    img, cnt = m.image_f_cache, m.count_f_cache
    _pp(m, a)
    assert (img.misses, cnt.misses) == (1, 1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        with torch.no_grad():
            out = m.patch_predictions(a)
    assert (img.hits, img.misses, img.bypassed) == (0, 1, 1) and (cnt.hits, cnt.misses, cnt.bypassed) == (0, 1, 1)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(_pp(m, a), want) and img.hits == 1      # and eager calls are served again


def test_batch_budget_and_copies():
    m, f = _model()
    _ready(m)
    m.count_classifier.eval()                                   # both modalities cached (the 4-D count grid per array)
    xi, xc, _ = _arrays()
    both = _inputs(xi, xc, slice(0, 2))
    with torch.no_grad():
        want_both = m.forward_nhwc(both).clone()
        want_each = [m.forward_nhwc(_inputs(xi, xc, slice(i, i + 1))).clone() for i in range(N_ARR)]
        want_pp = m.patch_predictions(_inputs(xi, xc, slice(0, 1))).clone()
    # a batch of 2 with one hit and one miss
    m.enable_f_cache()
    img, cnt = m.image_f_cache, m.count_f_cache
    calls = _count_calls(f)
    with torch.no_grad():
        assert torch.equal(m.forward_nhwc(_inputs(xi, xc, slice(0, 1))), want_each[0])
        got = m.forward_nhwc(both)
    assert (img.hits, img.misses) == (1, 2) and (cnt.hits, cnt.misses) == (1, 2) and calls[0] == 2
    assert torch.equal(got, want_both)
    with torch.no_grad():
        assert torch.equal(m.forward_nhwc(both), want_both)     # two hits
    assert (img.hits, img.misses) == (3, 2) and calls[0] == 2
    # a budget smaller than two arrays' rows: the first array is kept, the others are evaluated every time
    row_bytes = H * W * C * 4
    m.enable_f_cache(max_bytes=2 * row_bytes - 1)
    img = m.image_f_cache
    for _ in range(2):
        for i in range(N_ARR):
            with torch.no_grad():
                assert torch.equal(m.forward_nhwc(_inputs(xi, xc, slice(i, i + 1))), want_each[i])
    assert len(img) == 1 and img.bytes == row_bytes and (img.hits, img.misses) == (1, 5)
    # writing into what patch_predictions returned does not reach the cache
    m.enable_f_cache()
    one = _inputs(xi, xc, slice(0, 1))
    p0 = _pp(m, one)
    with torch.no_grad():
        p1 = m.patch_predictions(one)                           # a hit, not cloned by the caller
        assert torch.equal(p1, want_pp) and torch.equal(p0, want_pp)
        p1.zero_()
        p2 = m.patch_predictions(one)
        assert torch.equal(p2, want_pp)
        p2.fill_(3.0)
        assert torch.equal(m.patch_predictions(one), want_pp)
    assert m.image_f_cache.hits == 3 and m.image_f_cache.misses == 1


# ------------------------------------------------------------------------------------------------ 5. the loop
def _loop(cached, u8):
    import gridnext_amd as ga
    from gridnext_amd.utils import all_fgd_predictions
    xi, xc, y = _arrays(u8=u8)
    if u8:          # uint8 patches in host memory: they reach the device through the loop's prefetcher
        data = [((xi[i], xc[i]), y[i]) for i in range(N_ARR)]
    else:           # float patches resident on the device
        data = [((xi[i].to(DEV), xc[i].to(DEV)), y[i].to(DEV)) for i in range(N_ARR)]
    m, f = _model()
    if cached:
        m.enable_f_cache()
    dl = {'train': DataLoader(data[:2], batch_size=1, shuffle=True, generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(data[2:], batch_size=1)}
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        m, vh, th = ga.train_gridwise(m, dl, nn.CrossEntropyLoss(), opt, num_epochs=3)
    counts = None
    if cached:
        img = m.image_f_cache
        counts = (img.hits, img.misses, img.bypassed)
    # (every array twice in ONE call: all_fgd_predictions begins with model.to(device), and a DenseNet drops everything
    # derived from its tensors on any _apply - the row cache's token with it - so hits are hits within a call)
    preds = all_fgd_predictions(DataLoader(data + data, batch_size=1), m)
    after = (m.image_f_cache.hits, m.image_f_cache.misses) if cached else None
    return th, vh, {k: v.clone() for k, v in m.state_dict().items()}, counts, preds, after


@pytest.mark.parametrize('u8', [False, True], ids=['float_resident', 'uint8_prefetched'])
def test_train_gridwise_three_epochs_cache_off_vs_on(u8):
    """2 train arrays (shuffled, seeded) + 1 val array, 3 epochs: the image modality sees each array once (3 misses) and
    finds it six times; histories and final weights are those of the uncached loop.  The loop ends by restoring the best
    weights with load_state_dict, which - rightly - empties the cache: all_fgd_predictions afterwards, over every array
    twice, misses each array once and then hits it, with the uncached predictions."""
    th0, vh0, sd0, _, preds0, _ = _loop(False, u8)
    th1, vh1, sd1, counts, preds1, after = _loop(True, u8)
    print("train history", th0, th1, "val history", vh0, vh1, "image cache (hits, misses, bypassed)", counts, "after", after)
    assert len(th0) == 3 and len(vh0) == 3
    assert th0 == th1 and vh0 == vh1
    assert list(sd0) == list(sd1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    assert counts == (6, 3, 0)
    assert after == (6 + N_ARR, 3 + N_ARR)
    for a, b in zip(preds0, preds1):
        assert np.array_equal(a, b)
    half = len(preds1[2]) // 2
    assert np.array_equal(preds1[2][:half], preds1[2][half:])       # the hit pass gives the miss pass's probabilities
