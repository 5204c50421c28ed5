"""gridnext_amd/fcache.py: FrozenRowCache's bookkeeping on CPU tensors with an injected fingerprint (the device kernel is
held to its definition in test_gpu_fcache.py).  No GPU."""
import torch

import fingerprint_ref as R
from gridnext_amd.fcache import FrozenRowCache, state_token

S, F = 6, 3          # spots per array, feature columns


def host_fingerprint(src, n_seg):
    data = src.contiguous().numpy().tobytes()
    n = len(data) // max(n_seg, 1)
    return [R.fingerprint128(data[i * n:(i + 1) * n]) for i in range(n_seg)]


def f_rows(arrays):
    """A stand-in classifier: rows that depend on the array and on the spot."""
    a = arrays.reshape(arrays.shape[0], S, -1).float()
    return torch.stack([a.sum(2) * (c + 1) for c in range(F)], 2).reshape(-1, F)


class Calls:
    """compute(idx) as the model passes it, recording what it was asked for."""

    def __init__(self, arrays):
        self.arrays, self.asked = arrays, []

    def __call__(self, idx):
        self.asked.append(idx)
        return f_rows(self.arrays if idx is None else self.arrays[idx])


def arrays(n, seed=0):
    return torch.randint(0, 255, (n, S, 4), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_miss_then_hit_then_partial_hit_in_batch_order():
    cache = FrozenRowCache(fingerprint=host_fingerprint)
    x = arrays(4)
    want = f_rows(x)
    c = Calls(x[:2])
    assert torch.equal(cache.fetch('t', x[:2], 2, c), want[:2 * S]) and c.asked == [None]
    assert (cache.hits, cache.misses, len(cache)) == (0, 2, 2)
    c = Calls(x[:2])
    assert torch.equal(cache.fetch('t', x[:2], 2, c), want[:2 * S]) and c.asked == []            # all hits: f not called
    assert (cache.hits, cache.misses) == (2, 2)
    # arrays 3, 0, 2, 1: 0 and 1 are held, 3 and 2 are evaluated together, in batch order (positions 0 and 2)
    mixed = x[[3, 0, 2, 1]].contiguous()
    c = Calls(mixed)
    got = cache.fetch('t', mixed, 4, c)
    assert c.asked == [[0, 2]]
    assert torch.equal(got, f_rows(mixed))
    assert (cache.hits, cache.misses, len(cache)) == (4, 4, 4)
    # one array alone, held
    c = Calls(x[3:4])
    assert torch.equal(cache.fetch('t', x[3:4], 1, c), want[3 * S:]) and c.asked == []
    assert cache.bypassed == 0
    cache.bypass()
    assert cache.bypassed == 1


def test_key_holds_dtype_shape_and_length():
    """The same bytes as another dtype or another per-array shape are another entry."""
    cache = FrozenRowCache(fingerprint=host_fingerprint)
    x = arrays(1)
    cache.fetch('t', x, 1, Calls(x))
    as_i8 = x.view(torch.int8)
    c = Calls(as_i8)
    cache.fetch('t', as_i8, 1, c)
    assert c.asked == [None]
    reshaped = x.reshape(1, S * 2, 2)
    c = Calls(reshaped)
    cache.fetch('t', reshaped, 1, c)
    assert c.asked == [None] and len(cache) == 3


def test_budget_exhaustion_inserts_nothing_more_and_evicts_nothing():
    row_bytes = S * F * 4
    cache = FrozenRowCache(max_bytes=2 * row_bytes + 5, fingerprint=host_fingerprint)
    x = arrays(4)
    want = f_rows(x)
    assert torch.equal(cache.fetch('t', x, 4, Calls(x)), want)
    assert len(cache) == 2 and cache.bytes == 2 * row_bytes                 # arrays 0 and 1 fit, 2 and 3 do not
    c = Calls(x)
    assert torch.equal(cache.fetch('t', x, 4, c), want)                     # still right, 2 and 3 evaluated again
    assert c.asked == [[2, 3]] and len(cache) == 2
    assert (cache.hits, cache.misses) == (2, 6)
    zero = FrozenRowCache(max_bytes=0, fingerprint=host_fingerprint)
    assert torch.equal(zero.fetch('t', x, 4, Calls(x)), want) and len(zero) == 0
    cache.clear()
    assert len(cache) == 0 and cache.bytes == 0 and cache.misses == 6       # clear() drops entries, not the counters


def test_state_token_change_clears():
    cache = FrozenRowCache(fingerprint=host_fingerprint)
    x = arrays(2)
    cache.fetch('a', x, 2, Calls(x))
    c = Calls(x)
    cache.fetch('b', x, 2, c)
    assert c.asked == [None] and len(cache) == 2 and cache.misses == 4
    c = Calls(x)
    cache.fetch('b', x, 2, c)
    assert c.asked == []


def test_state_token_follows_the_classifier():
    """state_token: in-place parameter edits, buffer edits and load_state_dict change it; reading does not; a DenseNet's
    arithmetic switches and its cache epoch are part of it."""
    import torch.nn as nn
    from gridnext_amd.densenet import DenseNet
    seq = nn.Sequential(nn.Linear(4, 3), nn.BatchNorm1d(3))
    t0 = state_token(seq)
    seq.eval()(torch.rand(5, 4))
    assert state_token(seq) == t0
    with torch.no_grad():
        seq[0].weight.mul_(2.0)
    t1 = state_token(seq)
    assert t1 != t0
    seq[1].running_mean.add_(1.0)
    t2 = state_token(seq)
    assert t2 != t1
    seq.load_state_dict({k: v.clone() for k, v in seq.state_dict().items()})
    assert state_token(seq) != t2
    assert state_token(nn.Sequential(nn.Linear(4, 3), nn.BatchNorm1d(3))) != state_token(seq)
    f = DenseNet(growth_rate=4, block_config=(2,), num_init_features=8, bn_size=2, num_classes=3, small_inputs=True)
    d0 = state_token(f)
    assert state_token(f) == d0
    for name, value in (('mfma', 'f16'), ('split_conv1', True), ('split_conv2', True), ('winograd', False),
                        ('skip_empty', False), ('f16_buffers', False), ('f16_stem', False), ('f16_fused', False),
                        ('input_norm', ((0.5,) * 3, (0.2,) * 3))):
        keep = getattr(f, name)
        setattr(f, name, value)
        assert state_token(f) != d0, name
        setattr(f, name, keep)
        assert state_token(f) == d0, name
    f.invalidate_cache()
    assert state_token(f) != d0


def test_rows_handed_out_are_copies():
    cache = FrozenRowCache(fingerprint=host_fingerprint)
    x = arrays(2)
    want = f_rows(x)
    first = cache.fetch('t', x, 2, Calls(x))            # the miss pass returns the computed rows ...
    first.fill_(-1.0)                                   # ... which are not the cache's storage
    second = cache.fetch('t', x, 2, Calls(x))
    assert torch.equal(second, want)
    second.zero_()
    one = cache.fetch('t', x[:1], 1, Calls(x[:1]))
    assert torch.equal(one, want[:S])
    one.zero_()
    y = torch.cat([x[1:], arrays(1, seed=9)], 0)
    part = cache.fetch('t', y, 2, Calls(y))             # a partial hit
    assert torch.equal(part, f_rows(y))
    part.zero_()
    assert torch.equal(cache.fetch('t', x, 2, Calls(x)), want)
