"""CPU proofs of tests/conv0_dgrad_ref.py, the float64 reference test_gpu_conv0_dgrad.py holds gnx_conv0_dgrad to: that it is
the gradient autograd derives from F.conv2d, that all-ones operands give the window count, that the fp32 ratios G was set from
are still what the grid gives, and that it is the adjoint of the forward convolution."""
import pytest
import torch
import torch.nn.functional as F

import conv0_dgrad_ref as R

# one case per distinct reference (ldd and the alignment do not reach it)
DISTINCT = list({(c.geo, c.imgs, c.H, c.W, c.O): c for c in R.GRID}.values())
SEEN = {}


def note(kind, ratio, c):
    if ratio > SEEN.get(kind, (0.0, None))[0]:
        SEEN[kind] = (ratio, c)


def test_grid_holds_what_the_kernel_tests_need():
    for geo, shapes in R.SHAPES.items():
        for H, W in shapes:
            for imgs in (1, 3):
                for O, ldd in R.LAYOUTS:
                    assert R.Case(geo, imgs, H, W, O, ldd, 0) in R.GRID
    assert any(c.imgs == 130 and (c.H, c.W) == (16, 16) for c in R.GRID)
    assert any(c.shift for c in R.GRID)
    assert any(c.ldd % 4 for c in R.GRID) and any(c.ldd > c.O and c.ldd % 4 == 0 for c in R.GRID)
    assert {R.out_size(c) for c in R.GRID if c.geo == 7} >= {(8, 8), (9, 9), (11, 11), (8, 12), (64, 64), (112, 112)}
    assert R.G >= R.G_FLOOR and R.G == max(R.G_FLOOR, 4 * max(R.TORCH_FP32_RATIO, R.CHAIN_FP32_RATIO))


@pytest.mark.parametrize('c', DISTINCT, ids=R.ids)
def test_reference_is_autograd_of_conv2d(c):
    """float64 on both sides: the two differ by the order of a few thousand float64 additions at most."""
    r, ref = R.recipe(c), R.reference(c)
    got = R.dgrad_autograd(r.dS.double(), r.w.double(), c)
    assert got.shape == ref.ref.shape == (c.imgs, 3, c.H, c.W)
    assert bool(((got - ref.ref).abs() <= 2.0 ** -40 * ref.T).all())
    assert bool((ref.T > 0).all())                       # in these geometries every pixel is under at least one window
    assert R.detectable(ref.term, R.tol(ref.T))


@pytest.mark.parametrize('c', DISTINCT, ids=R.ids)
def test_all_ones_give_the_window_count(c):
    """dS = w = 1: every term is 1, dX = O x the number of windows that cover the pixel - exactly, in fp32 too."""
    ho, wo = R.out_size(c)
    ones = torch.ones(c.imgs * ho * wo, c.O)
    w = torch.ones(c.O, 3, c.geo, c.geo)
    want = (c.O * R.cover_counts(c)).expand(c.imgs, 3, c.H, c.W)
    assert torch.equal(R.dgrad(ones.double(), w.double(), c), want.double())
    assert torch.equal(R.chain_fp32(ones, w, c), want.float())
    cnt = R.cover_counts(c)
    assert int(cnt.max()) == (16 if c.geo == 7 else 9) and int(cnt.min()) == 4      # interior, corners


@pytest.mark.parametrize('c', DISTINCT, ids=R.ids)
def test_fp32_ratios_stay_within_what_G_was_set_from(c, capsys):
    r, ref = R.recipe(c), R.reference(c)
    rt = R.ratio(R.dgrad(r.dS, r.w, c), ref.ref, ref.T)
    rc = R.ratio(R.chain_fp32(r.dS, r.w, c), ref.ref, ref.T)
    note('torch', rt, c)
    note('chain', rc, c)
    with capsys.disabled():
        print(' fp32 ratios at %s: torch %.4f, chain %.4f' % (R.ids(c), rt, rc))
    assert rt <= R.G / 4 and rc <= R.G / 4, (rt, rc)


def test_recorded_ratios_are_what_the_grid_gives(capsys):
    """After the cases above (run alone: measures them itself).  The chain is elementwise IEEE arithmetic: its largest ratio is
    the recorded one to the printed digits.  torch's CPU convolution blocks its sums by the thread count, so its ratio is held to
    the recorded one only where that is the larger of the two - G must not rest on a figure the grid no longer gives."""
    if len(SEEN) < 2 or any(SEEN[k][1] is None for k in SEEN):
        for c in DISTINCT:
            r, ref = R.recipe(c), R.reference(c)
            note('torch', R.ratio(R.dgrad(r.dS, r.w, c), ref.ref, ref.T), c)
            note('chain', R.ratio(R.chain_fp32(r.dS, r.w, c), ref.ref, ref.T), c)
    with capsys.disabled():
        print('\n G = %.3f' % R.G)
        for kind, (ratio, c) in sorted(SEEN.items()):
            print(' largest fp32 %-5s ratio %.4f at %s' % (kind, ratio, R.ids(c)))
    assert abs(SEEN['chain'][0] - R.CHAIN_FP32_RATIO) <= 5e-4, SEEN['chain']
    assert SEEN['chain'][1][:5] == (3, 130, 16, 16, 64)
    assert SEEN['torch'][0] <= max(R.TORCH_FP32_RATIO, R.CHAIN_FP32_RATIO) + 5e-4, SEEN['torch']
    assert R.G == pytest.approx(4 * R.CHAIN_FP32_RATIO)


@pytest.mark.parametrize('c', [c for c in DISTINCT if c.imgs == 3 and c.O in (10, 64)], ids=R.ids)
def test_adjoint_identity(c):
    """<conv2d(x, w), dS> == <x, dgrad(dS)> in float64, x random: the reference is the adjoint of the forward convolution."""
    ks, s, p = R.GEOMETRY[c.geo]
    r, ref = R.recipe(c), R.reference(c)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(c.imgs, 3, c.H, c.W, generator=g, dtype=torch.float64) - 0.5
    fwd = F.conv2d(x, r.w.double(), stride=s, padding=p)
    lhs = (R.as_rows(fwd) * r.dS.double()).sum().item()
    rhs = (x * ref.ref).sum().item()
    scale = (x.abs() * ref.T).sum().item()
    assert abs(lhs - rhs) <= 2.0 ** -40 * scale, (lhs, rhs)
