"""A negative entry of a line list is an empty line in every sparse kernel (csrc/sparse_lines.h): `gnx_sparse_expand_f32`,
`gnx_sparse_line_moments_f64` and `gnx_sparse_line_max_f32` write exact zeros for it - into outputs pre-filled with NaN, so an
unwritten element shows - and the rows around it carry the bits of a call without it.  Matrix: 5 lines x 70 positions, line 2
with 70 entries (more than one lane stride), line 1 empty, line 0 NOT empty: a kernel that only clamped the -1 to line 0 would
write line 0's values into its row.  lines = [2, -1, 0, 1]."""
import numpy as np
import pytest
import torch

import sparse_counts_ref as CR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS, L_POS = [9, 0, 70, 5, 33], 70
NAN = float('nan')


def _run(lines):
    """(expand (n, 70), moments (n, 2), max (n,)) on the host for the line list `lines`."""
    from gridnext_amd import _lib as lib
    ptr, idx, val = CR.random_lines(np.random.default_rng(12), LENGTHS, L_POS, integer=False)
    ptr, idx, val = (torch.from_numpy(a).to(DEV) for a in (ptr, idx, val))
    ls, n = torch.tensor(lines, dtype=torch.int32, device=DEV), len(lines)
    dense = torch.full((n, L_POS), NAN, dtype=torch.float32, device=DEV)
    mom = torch.full((n, 2), NAN, dtype=torch.float64, device=DEV)
    top = torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    head = (lib.ptr(ptr, torch.int64), lib.ptr(idx, torch.int32), lib.ptr(val), lib.ptr(ls, torch.int32), n)
    lib.call('gnx_sparse_expand_f32', *head, None, lib.ptr(dense), L_POS, L_POS, lib.stream())
    lib.call('gnx_sparse_line_moments_f64', *head, None, lib.ptr(mom, torch.float64), lib.stream())
    lib.call('gnx_sparse_line_max_f32', *head, None, lib.ptr(top), lib.stream())
    return dense.cpu(), mom.cpu(), top.cpu()


def test_a_negative_line_is_an_empty_line():
    with_hole, without = _run([2, -1, 0, 1]), _run([2, 0, 1])
    for got, want in zip(with_hole, without):
        assert not torch.isnan(got).any() and not torch.isnan(want).any()        # every element was written
        assert torch.equal(got[1], torch.zeros_like(got[1]))                     # exact zeros for the -1
        assert torch.equal(got[[0, 2, 3]], want)                                 # the others: the bits of a call without it
    dense, mom, top = with_hole
    assert int((dense[0] != 0).sum()) == 70 and float(mom[0, 1]) > 0 and float(top[0]) > 0     # the long line was walked
    assert int((dense[2] != 0).sum()) == 9 and float(mom[2, 0]) > 0 and float(top[2]) > 0      # line 0 holds values
    assert not dense[3].any() and not mom[3].any() and float(top[3]) == 0                      # the empty line
