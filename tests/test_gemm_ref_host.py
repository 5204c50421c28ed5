"""tests/gemm_ref.py proved before test_gpu_gemm_forms.py uses it: `product` against a float64 torch.matmul, the input recipe,
detectability of every shape of GRID, and - through `form`, the Python restatement of gemm_f32_impl's dispatch - that GRID reaches
every kernel body, every instantiation and both sides of every edge between two forms.  Runs on the CPU."""
import pytest
import torch

import gemm_ref as R


def test_product_equals_float64_matmul():
    r = R.recipe(37, 21, 130, seed=3)
    ref, T = R.product(r.A, r.B)
    assert torch.equal(ref, torch.matmul(r.A, r.B.t())) and ref.dtype == torch.float64
    assert torch.equal(T, torch.matmul(r.A.abs(), r.B.abs().t()))
    ref2, T2 = R.product(r.A, r.B, r.bias, r.C0)
    want = torch.matmul(r.A, r.B.t()) + r.bias[None, :] + r.C0
    assert (ref2 - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert torch.equal(T2, T + r.bias.abs()[None, :] + r.C0.abs())
    assert (T2 >= ref2.abs() - 1e-9).all()
    ref3, T3 = R.product(None, None, r.bias, r.C0, parts=(ref, T))           # the cached matmuls give the same
    assert torch.equal(ref3, ref2) and torch.equal(T3, T2)
    # float32 operands are taken up to float64 first
    ref4, _ = R.product(r.A.float(), r.B.float())
    assert torch.equal(ref4, ref)


@pytest.mark.parametrize("M,N,K", [(5, 3, 8192), (64, 64, 2048), (1, 1, 1)])
def test_recipe_keeps_every_term_at_a_quarter_or_more(M, N, K):
    r = R.recipe(M, N, K, seed=1)
    for t in (r.A, r.B, r.bias, r.C0):
        assert t.dtype == torch.float64 and torch.equal(t, t.float().double())           # float32 values
        assert t.abs().min().item() >= 0.5 and t.abs().max().item() <= 1.5
    terms = (r.A[:, None, :] * r.B[None, :, :]).abs()
    assert terms.min().item() >= R.MIN_TERM
    if K >= 64:
        assert (r.A < 0).any() and (r.A > 0).any() and (r.B < 0).any() and (r.B > 0).any()
    _, T = R.product(r.A, r.B, r.bias, r.C0)
    assert T.max().item() <= R.t_bound(K)
    r2 = R.recipe(M, N, K, seed=1)
    assert torch.equal(r.A, r2.A) and torch.equal(r.C0, r2.C0)                            # reproducible


@pytest.mark.parametrize("M,N,K", R.SHAPES)
def test_grid_shapes_are_detectable(M, N, K):
    """With T <= 2.25 K + 3 for the recipe, a bound of the largest tolerance of the shape; the GPU test asserts the same
    on the T it computes."""
    assert R.detectable(R.tol(torch.tensor(R.t_bound(K))))


def test_G_is_what_the_measured_ratios_make_it():
    assert R.G == max(8.0, 4 * R.TORCH_FP32_RATIO, 4 * R.CHAIN_FP32_RATIO)
    # detectability holds up to K of about 40 000 for G near 24: the largest K of GRID is far below
    assert max(K for _, _, K in R.SHAPES) == 2048
    assert R.detectable(R.tol(torch.tensor(R.t_bound(2048)), g=24.0))


@pytest.mark.parametrize("M,N,K", R.SHAPES)
def test_sequential_fp32_chain_stays_within_the_ratio_G_was_set_from(M, N, K, capsys):
    """One of the two figures behind gemm_ref.G, kept runnable: a sequential fp32 multiply-add chain on the CPU against the
    float64 product, |err| / (2^-24 T), on up to 64 x 64 evenly spread elements of every shape of GRID."""
    r = R.recipe_of((M, N, K))
    rows, cols = R.sample(M, 64), R.sample(N, 64)
    A, B = r.A[rows].double(), r.B[cols].double()
    ref, T = R.product(A, B)
    ratio = ((R.chain_fp32(A, B).double() - ref).abs() / (R.U * T)).max().item()
    with capsys.disabled():
        print(' fp32 chain ratio at %d x %d x %d: %.4f' % (M, N, K, ratio))
    assert ratio <= R.CHAIN_FP32_RATIO, ratio


# ------------------------------------------------------------------------------------------------- the dispatch, restated
def test_split_counts_are_those_of_the_source():
    assert R.wide_splits(2048, 256, 512) == 4 and R.wide_splits(2048, 256, 2048) == 16 and R.wide_splits(2048, 256, 2016) == 15
    assert R.wide_splits(*R.EMPTY_SPLIT) == 10 and R.wide_split_tiles(R.EMPTY_SPLIT[2], 10) == [5] * 8 + [1, 0]
    assert 0 not in R.wide_split_tiles(1280, R.wide_splits(2048, 512, 1280))
    assert R.wide_splits(*R.WORKLOAD) == 6
    assert R.wide_splits(2047, 256, 512) == R.wide_splits(2048, 255, 512) == R.wide_splits(2048, 256, 511) == 0
    assert [R.tall_splits(130, 128, K) for K in (1020, 1024, 1472, 1473, 2000)] == [1, 2, 2, 3, 3]
    assert R.tall_splits(130, 129, 1024) == 1
    assert R.tall_splits(*R.CAP_BELOW) == 3 and R.tall_splits(*R.CAP_ABOVE) == 1
    assert 3 * R.CAP_BELOW[0] * 128 <= 1 << 26 < 3 * R.CAP_ABOVE[0] * 128
    assert R.workspace_floats(*R.WIDE) == 4 * 2048 * 256 and R.workspace_floats(*R.TALL) == 2 * 130 * 128
    assert R.workspace_floats(*R.BIG) == 0 and R.workspace_floats(*R.CAP_ABOVE) == 0
    # a wide shape never asks for the tall form's slabs and the other way round
    for M, N, K in R.SHAPES:
        assert not (R.wide_splits(M, N, K) >= 1 and R.tall_splits(M, N, K) > 1)


def test_grid_reaches_every_body_and_instantiation():
    forms = {}
    for c in R.GRID:
        body, S, av, bv = R.form_of(c)
        forms.setdefault((body, c.ak, c.bk, av, bv), []).append((c, S))
    for ak, bk in R.PAIRS:
        assert ('wide', ak, bk, True, True) in forms and ('big', ak, bk, True, True) in forms
        for body in ('tall', 'plain'):
            for av in (False, True):
                for bv in (False, True):
                    got = forms.get((body, ak, bk, av, bv), [])
                    assert got, (body, ak, bk, av, bv)
                    if not av:           # a scalar side comes about both by the pointer and by the leading dimension
                        assert {c.alay for c, _ in got} >= {'shifted', 'oddld'}, (body, ak, bk, av, bv)
                    if not bv:
                        assert {c.blay for c, _ in got} >= {'shifted', 'oddld'}, (body, ak, bk, av, bv)
        # per body and layout pair: bias NULL and present, accumulate 0 and 1
        for body in ('wide', 'big', 'tall', 'plain'):
            cs = [c for key, v in forms.items() if key[:3] == (body, ak, bk) for c, _ in v]
            assert {(c.bias, c.acc) for c in cs} == set(R.FLAGS), (body, ak, bk)
        # the wide body without a split (no workspace), with accumulate and bias in the kernel itself
        s1 = [c for c, S in forms[('wide', ak, bk, True, True)] if S == 1]
        assert {(c.bias, c.acc) for c in s1} == set(R.FLAGS) and all(not c.ws for c in s1)
    wide = [(c, S) for key, v in forms.items() if key[0] == 'wide' for c, S in v]
    assert {S for _, S in wide} >= {1, 4, 6, 10, 15, 16}
    assert any(0 in R.wide_split_tiles(c.K, S) for c, S in wide)                          # a split without a K tile
    assert any(R.wide_units(c.M, S) % 8 for c, S in wide) and any(R.wide_units(c.M, S) % 8 == 0 for c, S in wide)
    assert any(c.acc for c, S in wide if S > 1) and any(c.bias for c, S in wide if S > 1)
    big = [c for key, v in forms.items() if key[0] == 'big' for c, _ in v]
    assert {c.K for c in big} >= {4, 36, 508} and {c.M for c in big} >= {2048, 2049} and {c.N for c in big} >= {256, 257}
    tall = [(c, S) for key, v in forms.items() if key[0] == 'tall' for c, S in v]
    assert {S for _, S in tall} == {2, 3}
    # a wide and a big shape that one misaligned operand sends to the 64 x 64 body
    for shape in (R.WIDE, R.BIG):
        off = [c for c in R.GRID if (c.M, c.N, c.K) == shape and (c.alay, c.blay) != ('aligned', 'aligned')]
        assert off and all(R.form_of(c)[0] == 'plain' for c in off)
        assert {c.alay for c in off} >= set(R.LAYS) and {c.blay for c in off} >= set(R.LAYS)
    # plain: every ragged extent in every dimension, K off 4 included
    plain = [c for key, v in forms.items() if key[0] == 'plain' for c, _ in v]
    for dim, want in (('M', R.RAGGED_MN), ('N', R.RAGGED_MN), ('K', R.RAGGED_K)):
        assert {getattr(c, dim) for c in plain} >= set(want)
    assert (4992, 500, 2000) in R.SHAPES


@pytest.mark.parametrize("edge", range(len(R.EDGES)))
def test_every_edge_has_a_case_on_each_side(edge):
    lo, hi, want_lo, want_hi = R.EDGES[edge]
    for shape, want in ((lo, want_lo), (hi, want_hi)):
        cs = [c for c in R.GRID if (c.M, c.N, c.K) == shape and (c.ak, c.bk, c.alay, c.blay, c.ws) == (0, 0, 'aligned', 'aligned', 1)]
        assert cs, shape
        assert all(R.form_of(c)[:2] == want for c in cs), (shape, [R.form_of(c) for c in cs], want)


def test_threshold_neighbours_of_the_issue_are_in_the_grid():
    shapes = set(R.SHAPES)
    for M in (2044, 2047, 2048, 2052):
        assert (M, 256, 512) in shapes
    for N in (252, 255, 256, 260):
        assert (2048, N, 512) in shapes
    for K in (508, 512, 516):
        assert (2048, 256, K) in shapes
    for K in (4, 36, 508):
        for M in (2048, 2049):
            for N in (256, 257):
                assert (M, N, K) in shapes
    for N in (128, 129, 132):
        for K in (1020, 1024):
            assert (130, N, K) in shapes
    assert {(130, 128, 1472), (130, 128, 1473)} <= shapes
    # the reduce kernel's grid covers 2048 * 256 elements in one round: exactly that and past it, on both routes
    assert R.WIDE[0] * R.WIDE[1] == R.TALL_ROUND[0] * R.TALL_ROUND[1] == 2048 * 256
    assert {R.WIDE, R.WIDE_PAST, R.TALL_ROUND, R.TALL_ROUND_PAST} <= shapes
    # K-major A only where 4 | M goes through 16-B loads; the rest is counted among the scalar forms
    assert R.form_of(R.Case(2047, 256, 512, 1, 0, 'aligned', 'aligned', 0, 0, 1))[2] is False
