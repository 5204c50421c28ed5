"""gnx_loess_fit_f64 (csrc/loess.hip) through the C ABI against the per-point lstsq restatement (tests/hvg_ref.py).  Bar per point,
derived and not tuned: 8 cond(M) (cnt + 16) 2^-53 max |y in window|, M the point's weighted moment matrix - normal equations
lose cond(M), any order of cnt additions loses cnt 2^-53.  Windows of 1, 2, 3, 64, 65 and n points on n in {1, 2, 3, 4, 63, 64, 65,
129, 700}, every degree on every window that can carry it, inv_h = 0, buffers one element into their storage, the refusals and
determinism.

Measured on an MI355X (printed by the test): see the README's highly-variable-genes section."""
import numpy as np
import pytest
import torch

import hvg_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
SIZES = [1, 2, 3, 4, 63, 64, 65, 129, 700]
WINDOWS = [1, 2, 3, 64, 65, None]                                                    # None: all n points


def _L():
    from gridnext_amd import _lib
    return _lib


def _offset(array, dtype):
    """The array on the device, one element into its storage."""
    t = torch.empty(len(array) + 1, dtype=dtype, device=DEV)
    t[1:] = torch.from_numpy(np.ascontiguousarray(array)).to(DEV)
    return t[1:]


def _fit(xs, ys, lo, cnt, inv_h, degree, n_eval=None):
    lib = _L()
    n = len(xs)
    n_eval = n if n_eval is None else n_eval
    out = torch.full((n + 2,), NAN, dtype=torch.float64, device=DEV)
    a = (_offset(xs, torch.float64), _offset(ys, torch.float64), _offset(lo, torch.int32), _offset(cnt, torch.int32),
         _offset(inv_h, torch.float64), _offset(degree, torch.int32))
    lib.call('gnx_loess_fit_f64', lib.ptr(a[0], torch.float64), lib.ptr(a[1], torch.float64), n, lib.ptr(a[2], torch.int32),
             lib.ptr(a[3], torch.int32), lib.ptr(a[4], torch.float64), lib.ptr(a[5], torch.int32), out[1:].data_ptr(), n_eval,
             lib.stream())
    host = out.cpu()
    assert torch.isnan(host[0]) and torch.isnan(host[n_eval + 1:]).all()              # nothing around the n_eval results
    return host[1:n_eval + 1]


def _data(n):
    rng = np.random.default_rng(100 + n)
    xs = rng.random(n) * 5 - 1
    if n > 60:
        xs = rng.choice(xs[:(2 * n) // 3], size=n)                                    # ties at the larger sizes: h == 0 occurs
    return np.sort(xs), rng.standard_normal(n) * 2


_made = {}


def _cases():
    """[(n, q, forced degree or None, xs, ys, windows, fit, bar)], the restatement computed once."""
    if 'c' not in _made:
        out = []
        for n in SIZES:
            xs, ys = _data(n)
            for q in sorted({n if w is None else w for w in WINDOWS if w is None or w <= n}):
                span = 1.0 if q == n else (q + 0.5) / n
                assert R.q_of(n, span) == q
                fit, bar, wins = R.loess(xs, ys, span)
                out.append((n, q, None, xs, ys, wins, fit, bar))
                lo, cnt, inv_h, degree = wins
                for d in (0, 1):                                                      # a lower degree on the same windows
                    forced = np.minimum(degree, d).astype(np.int32)
                    if (forced != degree).any():
                        pts = [R.point(xs, ys, int(lo[i]), int(cnt[i]), float(inv_h[i]), int(forced[i]), xs[i]) for i in range(n)]
                        f = np.array([p[0] for p in pts])
                        b = np.array([8 * p[1] * (cnt[i] + 16) * R.U * p[2] for i, p in enumerate(pts)])
                        out.append((n, q, d, xs, ys, (lo, cnt, inv_h, forced), f, b))
        _made['c'] = out
    return _made['c']


def test_fit_against_lstsq_under_the_bar():
    worst, seen_deg, seen_tie, seen_cnt = 0.0, set(), 0, set()
    for n, q, d, xs, ys, (lo, cnt, inv_h, degree), fit, bar in _cases():
        got = _fit(xs, ys, lo, cnt, inv_h, degree).numpy()
        err = np.abs(got - fit)
        assert np.isfinite(got).all() and (err <= bar).all(), (n, q, d, float((err / bar).max()))
        assert bar.max() < 1e-6                                                      # no bar of this fixture is vacuous
        worst = max(worst, float((err / bar).max()))
        seen_deg |= set(degree.tolist())
        seen_tie += int((inv_h == 0).sum())
        seen_cnt |= set(cnt.tolist())
    print("loess against lstsq over %d launches: largest |err| / (8 cond(M) (cnt + 16) 2^-53 max |y|) = %.4f" % (len(_cases()), worst))
    assert seen_deg == {0, 1, 2} and seen_tie > 50 and {1, 2, 3, 64, 65, 129, 700} <= seen_cnt


def test_a_second_call_gives_equal_bits_and_a_prefix_of_the_points():
    for n, q, d, xs, ys, (lo, cnt, inv_h, degree), fit, bar in _cases():
        if n == 700 and d is None:
            first, again = _fit(xs, ys, lo, cnt, inv_h, degree), _fit(xs, ys, lo, cnt, inv_h, degree)
            assert torch.equal(first.view(torch.int64), again.view(torch.int64)), q
            part = _fit(xs, ys, lo, cnt, inv_h, degree, n_eval=130)                   # n_eval < n: the first points alone
            assert torch.equal(part.view(torch.int64), first[:130].view(torch.int64))


def test_windows_are_cut_to_the_points_and_a_wild_degree_is_nan():
    """A window that reaches outside [0, n) reads nothing outside: the result is the fit over its part inside.  A degree outside
    0 .. 2 cannot be refused by a launcher that never reads device memory: that point alone is NaN (gridnext_amd/hvg.py refuses
    it on the host, tests/test_hvg_host.py)."""
    xs, ys = _data(65)
    fit, bar, (lo, cnt, inv_h, degree) = R.loess(xs, ys, 1.0)
    wide_lo, wide_cnt = (lo - 7).astype(np.int32), (cnt + 1000).astype(np.int32)
    got = _fit(xs, ys, wide_lo, wide_cnt, inv_h, degree).numpy()
    assert (np.abs(got - fit) <= bar).all()
    wild = degree.copy()
    wild[[3, 40]] = [3, -1]
    got = _fit(xs, ys, lo, cnt, inv_h, wild).numpy()
    keep = np.ones(65, dtype=bool)
    keep[[3, 40]] = False
    assert np.isnan(got[~keep]).all() and (np.abs(got[keep] - fit[keep]) <= bar[keep]).all()


def test_refusals_leave_the_output_untouched():
    lib = _L()
    xs, ys = _data(4)
    fit, bar, (lo, cnt, inv_h, degree) = R.loess(xs, ys, 1.0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (xs, ys, lo, cnt, inv_h, degree)]
    out = torch.full((6,), NAN, dtype=torch.float64, device=DEV)
    X, Y, LO, CN, IH, DG = (a.data_ptr() for a in t)
    O, S = out.data_ptr(), lib.stream()
    bad, q, name = lib.CONSTANTS['GNX_ERR_BAD_ARG'], lib.query, 'gnx_loess_fit_f64'
    for k in range(7):                                                                # every pointer in turn
        args = [X, Y, 4, LO, CN, IH, DG, O, 4, S]
        args[[0, 1, 3, 4, 5, 6, 7][k]] = None
        assert q(name, *args) == bad, k
    assert q(name, X, Y, -1, LO, CN, IH, DG, O, 0, S) == bad
    assert q(name, X, Y, 4, LO, CN, IH, DG, O, -1, S) == bad
    assert q(name, X, Y, 4, LO, CN, IH, DG, O, 5, S) == bad                           # more evaluation points than points
    assert q(name, X + 4, Y, 4, LO, CN, IH, DG, O, 4, S) == bad                       # doubles that are not 8-byte aligned
    assert q(name, X, Y, 4, LO, CN, IH, DG, O + 4, 4, S) == bad
    assert q(name, X, Y, 2 ** 31, LO, CN, IH, DG, O, 4, S) == lib.ERR_UNSUPPORTED
    assert q(name, X, Y, 4, LO, CN, IH, DG, O, 0, S) == 0                             # n_eval == 0: OK, nothing launched
    assert q(name, None, None, 0, None, None, None, None, None, 0, S) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert q(name, X, Y, 4, LO, CN, IH, DG, O, 4, S) == 0
    torch.cuda.synchronize()
    assert (np.abs(out[:4].cpu().numpy() - fit) <= bar).all() and torch.isnan(out[4:]).all()


def test_package_device_loess_equals_its_host_loess_under_the_bar():
    from gridnext_amd import hvg
    xs, ys = _data(700)
    fit, bar, _ = R.loess(xs, ys, 0.3)
    dev, host = hvg.loess_fit(xs, ys, 0.3, DEV), hvg.loess_fit(xs, ys, 0.3)
    assert (np.abs(dev - fit) <= bar).all() and (np.abs(host - fit) <= bar).all()
    with pytest.raises(ValueError, match="degree must be 0, 1 or 2"):
        hvg.fit_windows(xs, ys, *hvg.loess_windows(xs, 0.3)[:3], np.full(700, 5, dtype=np.int32), DEV)
