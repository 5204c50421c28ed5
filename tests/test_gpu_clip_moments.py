"""gnx_sparse_line_clip_moments_f64 (csrc/sparse_counts.hip) through the C ABI: the moments of a line's entries cut at the ROW's
bound, against math.fsum within n 2^-53 sum |term| (tests/sparse_counts_ref.py), exact on integers, equal bits with
gnx_sparse_line_moments_f64 under a bound of +inf, its refusals and determinism."""
import math

import numpy as np
import pytest
import torch

import sparse_counts_ref as CR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [0, 1, 63, 64, 65, 257, 0, 300]
NAN, INF = float('nan'), float('inf')


def _L():
    from gridnext_amd import _lib
    return _lib


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offset(array, dtype):
    """The array on the device, one element into its storage."""
    t = torch.empty(len(array) + 1, dtype=dtype, device=DEV)
    t[1:] = torch.from_numpy(np.ascontiguousarray(array)).to(DEV)
    return t[1:]


def _run(name, ptr, idx, val, lines, n, mask, clip=None):
    """(n, 2) float64 CPU tensor; the output sits one element into its storage, pre-filled with NaN, and its surroundings stay."""
    lib = _L()
    out = torch.full((2 * n + 2,), NAN, dtype=torch.float64, device=DEV)
    args = (_dev(ptr), _offset(idx, torch.int32), _offset(val, torch.float32), _dev(lines), _dev(mask))
    head = (lib.ptr(args[0], torch.int64), lib.ptr(args[1], torch.int32), lib.ptr(args[2]), lib.ptr(args[3], torch.int32), n,
            lib.ptr(args[4], torch.uint8))
    bound = None if clip is None else _offset(clip, torch.float64)
    extra = () if clip is None else (lib.ptr(bound, torch.float64),)
    lib.call(name, *head, *extra, out[1:].data_ptr(), lib.stream())
    host = out.cpu()
    assert torch.isnan(host[0]) and torch.isnan(host[-1])                            # nothing around the 2 n results
    return host[1:-1].view(n, 2)


def _clip(*a):
    return _run('gnx_sparse_line_clip_moments_f64', *a)


def _want(ptr, idx, val, lines, n, mask, clip):
    """Per row (fsum t, fsum t^2, terms), t = min(v, clip[row]) in double; a negative line is empty."""
    rows = []
    for i in range(n):
        line = i if lines is None else int(lines[i])
        v = CR.line_entries(ptr, idx, val, line, mask).astype(np.float64) if line >= 0 else np.zeros(0)
        t = np.minimum(v, clip[i])
        rows.append((math.fsum(t), math.fsum(t * t), len(t)))
    return rows


CASES = [(None, len(LENGTHS), False), (None, len(LENGTHS), True), (np.array([7, 5, -1, 5, 0, 2, 1, 3, 4, 6], dtype=np.int32), 10, True),
         (np.array([7, 5, -1, 5, 0, 2, 1, 3, 4, 6], dtype=np.int32), 10, False), (None, 3, False)]


def test_integer_values_with_integer_bounds_are_exact():
    rng = np.random.default_rng(6)
    ptr, idx, val = CR.random_lines(rng, LENGTHS, 400, integer=True)
    mask = (rng.random(400) < 0.5).astype(np.uint8)
    clipped = 0
    for lines, n, masked in CASES:
        clip = rng.integers(1, 150, size=n).astype(np.float64)
        m = mask if masked else None
        got = _clip(ptr, idx, val, lines, n, m, clip).numpy()
        want = _want(ptr, idx, val, lines, n, m, clip)
        assert np.array_equal(got, np.array([(a, b) for a, b, _ in want]).reshape(n, 2)), (n, masked)
        plain = _want(ptr, idx, val, lines, n, m, np.full(n, INF))
        clipped += sum(a < b for (a, _, _), (b, _, _) in zip(want, plain))
    assert clipped >= 10                                                             # the bounds did cut


def test_fractional_bounds_within_the_summation_bound():
    rng = np.random.default_rng(7)
    worst = 0.0
    for integer in (True, False):
        ptr, idx, val = CR.random_lines(rng, LENGTHS, 400, integer=integer)
        mask = (rng.random(400) < 0.5).astype(np.uint8)
        for lines, n, masked in CASES:
            clip = rng.random(n) * (120.0 if integer else 6.0) + 0.37
            m = mask if masked else None
            got = _clip(ptr, idx, val, lines, n, m, clip).numpy()
            for i, (s1, s2, terms) in enumerate(_want(ptr, idx, val, lines, n, m, clip)):
                # t >= 0: sum |term| is the sum itself; the square adds one rounding per term, inside the fma: n + 1
                b1, b2 = CR.moments_bound(terms, s1), CR.moments_bound(terms + 1, s2)
                assert abs(got[i, 0] - s1) <= b1 and abs(got[i, 1] - s2) <= b2, (integer, n, masked, i)
                worst = max(worst, abs(got[i, 0] - s1) / b1 if b1 else 0.0, abs(got[i, 1] - s2) / b2 if b2 else 0.0)
    print("clipped moments against fsum: largest |err| / (n 2^-53 sum |term|) = %.3f" % worst)


def test_unbounded_equals_the_plain_moments_and_zero_gives_zero():
    rng = np.random.default_rng(8)
    for integer in (True, False):
        ptr, idx, val = CR.random_lines(rng, LENGTHS, 400, integer=integer)
        mask = (rng.random(400) < 0.5).astype(np.uint8)
        for lines, n, masked in CASES:
            m = mask if masked else None
            plain = _run('gnx_sparse_line_moments_f64', ptr, idx, val, lines, n, m)
            got = _clip(ptr, idx, val, lines, n, m, np.full(n, INF))
            assert torch.equal(got.view(torch.int64), plain.view(torch.int64)) and float(got.sum()) > 0
            assert torch.equal(_clip(ptr, idx, val, lines, n, m, np.zeros(n)), torch.zeros(n, 2, dtype=torch.float64))
            some = rng.random(n) * 50
            first, again = _clip(ptr, idx, val, lines, n, m, some), _clip(ptr, idx, val, lines, n, m, some)
            assert torch.equal(first.view(torch.int64), again.view(torch.int64))     # equal bits on a second call


def test_refusals_leave_the_output_untouched():
    lib = _L()
    ptr, idx, val = CR.random_lines(np.random.default_rng(5), [3, 4], 10)
    p, i, v, c = _dev(ptr), _dev(idx), _dev(val), _dev(np.array([2.5, 100.0]))
    out = torch.full((6,), NAN, dtype=torch.float64, device=DEV)
    P, I, V, C, O, S = p.data_ptr(), i.data_ptr(), v.data_ptr(), c.data_ptr(), out.data_ptr(), lib.stream()
    bad, q, name = lib.CONSTANTS['GNX_ERR_BAD_ARG'], lib.query, 'gnx_sparse_line_clip_moments_f64'
    assert q(name, None, I, V, None, 2, None, C, O, S) == bad
    assert q(name, P, None, V, None, 2, None, C, O, S) == bad
    assert q(name, P, I, None, None, 2, None, C, O, S) == bad
    assert q(name, P, I, V, None, 2, None, None, O, S) == bad                        # a NULL clip
    assert q(name, P, I, V, None, 2, None, C, None, S) == bad
    assert q(name, P, I, V, None, -1, None, C, O, S) == bad
    assert q(name, P, I, V, None, 0, None, None, O, S) == bad                        # bad arguments come before n == 0
    assert q(name, P, I, V, None, 2 ** 31, None, C, O, S) == lib.ERR_UNSUPPORTED
    assert q(name, P, I, V, None, 0, None, C, O, S) == 0
    assert q(name, P, None, None, None, 0, None, C, O, S) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                    # nothing was launched
    assert q(name, P, I, V, None, 2, None, C, O, S) == 0
    torch.cuda.synchronize()
    want = _want(ptr, idx, val, None, 2, None, np.array([2.5, 100.0]))
    assert out[:4].cpu().tolist() == [want[0][0], want[0][1], want[1][0], want[1][1]] and torch.isnan(out[4:]).all()
