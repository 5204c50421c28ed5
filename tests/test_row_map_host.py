"""`visium_datasets.RowMap`, the one storage-row -> batch-position map of SparseCountLinear, ExpressionMetrics and SparseMSELoss,
without a GPU: `ok` and the filled positions against a plain numpy restatement, the two users' own refusal messages on the bad
batches, and the state_dict keys the map must not add to.  Storage: 3 arrays of 4, 3 and 5 rows, arrays 0 and 2 bound."""
import numpy as np
import pandas as pd
import pytest
import torch

SIZES, G, F = (4, 3, 5), 6, 3
N = sum(SIZES)
# name -> (rows, lies in the view, distinct)
CASES = {
    'inside': ([0, 3, 7, 11, 9], True, True),
    'storage size': ([0, N], False, True),
    'minus one': ([1, -1], False, True),
    'array 1': ([2, 5], False, True),
    'repeated': ([3, 8, 3], True, False),
    'empty': ([], True, True),
}
_made = {}


def _view():
    if 'v' not in _made:
        import gridnext_amd as ga
        rng = np.random.default_rng(0)
        X = rng.integers(0, 5, size=(N, G))
        obs = pd.DataFrame({'x': np.arange(N), 'y': np.zeros(N, dtype=int),
                            'array': np.repeat(['a0', 'a1', 'a2'], SIZES)}, index=['s%d' % k for k in range(N)])
        _made['v'] = ga.SpotCounts(X, obs, ['g%d' % g for g in range(G)]).subset_arrays(['a0', 'a2'])
    return _made['v']


def _restated(rows):
    """(in the view, distinct, positions of the rows clamped into the storage) in plain numpy."""
    bound = np.zeros(N, dtype=bool)
    bound[0:4] = bound[7:12] = True
    r = np.asarray(rows, dtype=np.int64)
    safe = np.clip(r, 0, N - 1)
    pos = np.full(N, -1, dtype=np.int32)
    for b, row in enumerate(safe):
        pos[row] = b
    return bool(np.all((r >= 0) & (r < N)) and np.all(bound[safe])), len(set(r.tolist())) == len(r), safe, pos


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("case", list(CASES))
def test_map_equals_the_numpy_restatement(case, dtype):
    from gridnext_amd.visium_datasets import RowMap
    rows, in_view, distinct = CASES[case]
    m = RowMap(_view())
    assert m.bound.dtype == torch.bool and m.pos.dtype == torch.int32 and m.pos.numel() == N and bool((m.pos == -1).all())
    want_in, want_distinct, want_safe, want_pos = _restated(rows)
    assert (want_in, want_distinct) == (in_view, distinct)
    t = torch.tensor(rows, dtype=dtype)
    ok, safe = m.in_view(t)
    assert ok.dim() == 0 and ok.dtype == torch.bool and bool(ok) == in_view
    assert safe.dtype == torch.int64 and np.array_equal(safe.numpy(), want_safe)
    pos = m.fill(safe)
    assert pos is m.pos and bool(m.distinct(safe, pos)) == distinct
    if distinct:                                                                 # a repeat leaves the repeated row's position open
        assert np.array_equal(pos.numpy(), want_pos)
        assert np.array_equal(pos[7:].numpy(), want_pos[7:])                     # array 2's slice of the map
    m.fill(torch.tensor([5], dtype=dtype))                                       # a second batch clears the first
    assert pos.tolist() == [-1] * 5 + [0] + [-1] * 6


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("case", list(CASES))
def test_both_users_raise_their_own_messages(case, dtype):
    import gridnext_amd as ga
    rows, in_view, distinct = CASES[case]
    v = _view()
    t = torch.tensor(rows, dtype=dtype)
    torch.manual_seed(0)
    layer, metrics = ga.SparseCountLinear(v, F), ga.ExpressionMetrics(v, activation=None)
    z = torch.zeros((len(rows), G))
    if in_view and distinct:
        out = layer(t)
        assert out.shape == (len(rows), F) and out.requires_grad
        assert metrics.update(z, t).n == len(rows)
        return
    with pytest.raises(ValueError, match=r"SparseCountLinear: a batch that takes gradients must hold distinct storage rows of the "
                                         r"bound arrays \['a0', 'a2'\] \(rows 0 \.\. 11 of the storage\): a repeated row, a row "
                                         r"outside the storage or a row of an unbound array would lose its contribution"):
        layer(t)
    with torch.no_grad():
        if in_view:
            layer(t)                                                             # forwards under no_grad are never checked
    why = ("a repeated row would lose its sparse terms while its prediction is counted twice" if in_view else
           "a row outside the storage or of another array has no target here")
    with pytest.raises(ValueError, match=r"ExpressionMetrics: a batch must hold distinct storage rows of the bound arrays "
                                         r"\['a0', 'a2'\] \(rows 0 \.\. 11 of the storage\): " + why):
        metrics.update(z, t)
    assert metrics.n == 0 and not metrics.table.any()


def test_the_map_adds_no_state_dict_key():
    import gridnext_amd as ga
    v = _view()
    assert list(ga.SparseCountLinear(v, F).state_dict()) == ['weight', 'bias']
    assert list(ga.SparseCountLinear(v, F, bias=False).state_dict()) == ['weight']
    assert list(ga.SparseMSELoss(v).state_dict()) == []
    assert list(ga.SparseMSELoss(v, gene_scale=torch.ones(G)).state_dict()) == []
    mse = ga.SparseMSELoss(v)
    with pytest.raises(ValueError, match=r"SparseMSELoss: the rows must be storage rows of the bound arrays \['a0', 'a2'\] "
                                         r"\(rows 0 \.\. 11 of the storage"):
        mse(torch.zeros((2, G)), torch.tensor([2, 5]))
    assert mse(torch.zeros((3, G)), torch.tensor([3, 8, 3])).dim() == 0          # repeats are fine for the criterion
