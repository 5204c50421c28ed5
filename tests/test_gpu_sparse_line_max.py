"""gnx_sparse_line_max_f32 (csrc/sparse_counts.hip) through the C ABI against the numpy restatement (tests/sparse_mse_ref.py) -
a maximum has no order, so the comparison is bit for bit - its refusals, and `SpotCounts.gene_max` / `SparseMSELoss.unit_scale`
on resident counts against the host path."""
import numpy as np
import pytest
import torch

import sparse_counts_ref as CR
import sparse_mse_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [0, 1, 63, 64, 65, 257, 0, 300]
NAN = float('nan')


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


def _line_max(ptr, idx, val, lines, n, mask):
    lib = _L()
    out = torch.full((n + 2,), NAN, dtype=torch.float32, device=DEV)
    args = (_dev(ptr), _offset(idx, torch.int32), _offset(val, torch.float32), _dev(lines), _dev(mask))
    lib.call('gnx_sparse_line_max_f32', lib.ptr(args[0], torch.int64), lib.ptr(args[1], torch.int32), lib.ptr(args[2]),
             lib.ptr(args[3], torch.int32), n, lib.ptr(args[4], torch.uint8), out[1:].data_ptr(), lib.stream())
    host = out.cpu()
    assert torch.isnan(host[0]) and torch.isnan(host[-1])                            # nothing around the n results
    return host[1:-1]


@pytest.mark.parametrize("integer", [True, False])
def test_line_max_equals_numpy(integer):
    """Lines of 0, 1, 63, 64, 65, 257 and 300 entries (under, at and over a wavefront, several strides), all lines, a prefix of
    them, a list with repeats, with and without a mask, a mask that keeps nothing."""
    rng = np.random.default_rng(6)
    ptr, idx, val = CR.random_lines(rng, LENGTHS, 400, integer=integer)
    n = len(LENGTHS)
    mask = (rng.random(400) < 0.5).astype(np.uint8)
    lines = np.array([7, 5, 5, 0, 2, 1, 3, 4, 6], dtype=np.int32)
    for ls, k, m in ((None, n, None), (None, n, mask), (lines, len(lines), mask), (lines, len(lines), None), (None, 3, None)):
        want = R.line_max(ptr, idx, val, ls, k, m)
        assert torch.equal(_line_max(ptr, idx, val, ls, k, m), torch.from_numpy(want)), (k, m is None)
    assert want[0] == 0 and want[2] > 0
    assert torch.equal(_line_max(ptr, idx, val, None, n, np.zeros(400, np.uint8)), torch.zeros(n))


def test_refusals_leave_the_output_untouched():
    lib = _L()
    ptr, idx, val = CR.random_lines(np.random.default_rng(5), [3, 4], 10)
    p, i, v = _dev(ptr), _dev(idx), _dev(val)
    out = torch.full((4,), NAN, device=DEV)
    P, I, V, O, S = p.data_ptr(), i.data_ptr(), v.data_ptr(), out.data_ptr(), lib.stream()
    bad, q = lib.CONSTANTS['GNX_ERR_BAD_ARG'], lib.query
    assert q('gnx_sparse_line_max_f32', None, I, V, None, 2, None, O, S) == bad
    assert q('gnx_sparse_line_max_f32', P, None, V, None, 2, None, O, S) == bad
    assert q('gnx_sparse_line_max_f32', P, I, None, None, 2, None, O, S) == bad
    assert q('gnx_sparse_line_max_f32', P, I, V, None, 2, None, None, S) == bad
    assert q('gnx_sparse_line_max_f32', P, I, V, None, -1, None, O, S) == bad
    assert q('gnx_sparse_line_max_f32', P, I, V, None, 2 ** 31, None, O, S) == lib.ERR_UNSUPPORTED
    assert q('gnx_sparse_line_max_f32', P, I, V, None, 0, None, O, S) == 0
    assert q('gnx_sparse_line_max_f32', P, None, None, None, 0, None, O, S) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                    # nothing was launched
    assert q('gnx_sparse_line_max_f32', P, I, V, None, 2, None, O, S) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:2].cpu(), torch.from_numpy(R.line_max(ptr, idx, val, None, 2))) and torch.isnan(out[2:]).all()


def test_gene_max_on_resident_counts_equals_the_host_path(monkeypatch):
    import gridnext_amd as ga
    X, obs, genes = CR.synthetic_arrays(seed=6, n_arrays=2)
    host = ga.SpotCounts(X, obs, genes)
    host.normalize_total(1e4).log1p()
    dev = host.to(DEV)
    picked = [genes[g] for g in np.random.default_rng(6).permutation(300)[:64]]
    from gridnext_amd import _lib
    seen, real = [], _lib.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    for h, d in ((host, dev), (host.subset_genes(picked), dev.subset_genes(picked)),
                 (host.subset_genes(picked).subset_arrays(['arr1']), dev.subset_genes(picked).subset_arrays(['arr1']))):
        del seen[:]
        got = d.gene_max()
        assert seen == ['gnx_sparse_line_max_f32'] * len(d.arrays)                   # one launch per array of the view
        assert got.dtype == torch.float32 and not got.is_cuda and torch.equal(got, h.gene_max()) and float(got.max()) > 0
        assert torch.equal(d.gene_max(arrays=['arr0']), h.gene_max(arrays=['arr0']))
        assert torch.equal(ga.SparseMSELoss.unit_scale(d), ga.SparseMSELoss.unit_scale(h))
    with pytest.raises(RuntimeError, match="the counts are on cuda:0; the criterion has no device form"):
        ga.SparseMSELoss(dev)
