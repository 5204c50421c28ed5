"""gnx_conv0_dgrad (csrc/conv0_dgrad.hip), the gradient of the stem convolution with respect to the patches, through the C ABI
against the float64 reference of tests/conv0_dgrad_ref.py, over conv0_dgrad_ref.GRID: the smallest shapes at which each index rule
can go wrong (odd conv map, odd patch, H != W, one and several tiles, more tiles than workgroups, both dS read paths, a window of
a wider buffer, dS off a 16-B boundary) and the two geometries that ship.

dS is a window of a NaN-filled [rows][ldd] buffer (4 columns in where ldd leaves room), dX sits between two NaN frames and is
NaN-filled itself: a column read past O, an element not written or a write outside dX shows as a NaN or a changed frame.

Per case: (1) within G 2^-24 T of float64 on the same fp32 operands (G, T: conv0_dgrad_ref; G came from plain fp32 evaluations of
the reference operation, not from the kernel), every element finite; (2) all-ones operands give O x the window count exactly;
(3) a second launch gives the same bits, and each image of a batch the bits of that image launched alone.  Per geometry: the
adjoint identity against the project's own forward, gnx_conv_stem; the refusals."""
import pytest
import torch

import conv0_dgrad_ref as R
from gridnext_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FRAME = 64
NAN = float('nan')
BAD_ARG, UNSUPPORTED = -1, -3


def bits(t):
    return t.view(torch.int32)


class Rows:
    """dS [M][O] as the window [:, col0 : col0 + O] of a NaN-filled [M][ldd] buffer that starts 4 + shift floats into its
    storage."""

    def __init__(self, dS, c):
        M = dS.shape[0]
        self.col0 = min(4, c.ldd - c.O)
        self.store = torch.full((M * c.ldd + 8,), NAN, device=DEV)
        self.buf = self.store[4 + c.shift:4 + c.shift + M * c.ldd].view(M, c.ldd)
        self.buf[:, self.col0:self.col0 + c.O] = dS.to(DEV)
        self.before = self.store.clone()
        self.ldd = c.ldd
        assert self.store.data_ptr() % 16 == 0

    def ptr(self, row=0):
        return self.buf.data_ptr() + 4 * (row * self.ldd + self.col0)

    def unchanged(self):
        return torch.equal(bits(self.store), bits(self.before))


class Out:
    """dX [imgs][3][H][W], NaN-filled, between two NaN frames."""

    def __init__(self, imgs, H, W):
        self.n, self.shape = imgs * 3 * H * W, (imgs, 3, H, W)
        self.store = torch.full((self.n + 2 * FRAME,), NAN, device=DEV)
        self.frame = bits(self.store[:FRAME]).clone()

    @property
    def ptr(self):
        return self.store.data_ptr() + 4 * FRAME

    def get(self):
        return self.store[FRAME:FRAME + self.n].view(self.shape)

    def frames_unchanged(self):
        return torch.equal(bits(self.store[:FRAME]), self.frame) and torch.equal(bits(self.store[FRAME + self.n:]), self.frame)

    def untouched(self):
        return self.frames_unchanged() and bool(torch.isnan(self.get()).all())


def launch(rows, w, out, c, imgs=None, row=0):
    ks, s, p = R.GEOMETRY[c.geo]
    L.call('gnx_conv0_dgrad', rows.ptr(row), rows.ldd, L.ptr(w), out.ptr, c.imgs if imgs is None else imgs, c.H, c.W, c.O, ks, ks,
           s, p, L.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize('c', R.GRID, ids=R.ids)
def test_conv0_dgrad_against_float64(c, capsys):
    r, ref = R.recipe(c), R.reference(c)
    rows, w, out = Rows(r.dS, c), r.w.to(DEV), Out(c.imgs, c.H, c.W)
    launch(rows, w, out, c)
    got = out.get().cpu()
    assert bool(torch.isfinite(got).all()), 'an element of dX was not written, or a column past O was read'
    assert out.frames_unchanged() and rows.unchanged() and torch.equal(w.cpu(), r.w)
    t = R.tol(ref.T)
    assert R.detectable(ref.term, t)
    with capsys.disabled():
        print(' %s: |err| / (u T) = %.4f (G = %.3f)' % (R.ids(c), R.ratio(got, ref.ref, ref.T), R.G))
    assert not R.flagged(got, ref.ref, t), R.ratio(got, ref.ref, ref.T)
    # a second launch: the same bits; each image alone: the bits it has in the batch
    again = Out(c.imgs, c.H, c.W)
    launch(rows, w, again, c)
    assert torch.equal(again.get().cpu(), got)
    if c.imgs == 3:
        ho, wo = R.out_size(c)
        for i in range(3):
            one = Out(1, c.H, c.W)
            launch(rows, w, one, c, imgs=1, row=i * ho * wo)
            assert one.frames_unchanged()
            assert torch.equal(one.get().cpu()[0], got[i]), 'image %d alone differs from image %d of the batch' % (i, i)
    # all ones: O x the number of windows over the pixel, an integer
    ones = Rows(torch.ones_like(r.dS), c)
    w1, o1 = torch.ones_like(w), Out(c.imgs, c.H, c.W)
    launch(ones, w1, o1, c)
    want = (c.O * R.cover_counts(c)).float().expand(c.imgs, 3, c.H, c.W)
    assert torch.equal(o1.get().cpu(), want)


ADJOINT = [c for c in R.GRID if c.imgs == 3 and (c.O, c.ldd) in ((10, 22), (64, 64)) and not c.shift]


@pytest.mark.parametrize('c', ADJOINT, ids=R.ids)
def test_adjoint_of_the_forward_stem_kernel(c):
    """sum(gnx_conv_stem(x) * dS) == sum(x * gnx_conv0_dgrad(dS)), both sums in float64 on the host; tolerance: the two sides'
    G u T bounds, sum |dS| G u conv(|x|, |w|) + sum |x| G u T.  Ties the gradient to the forward KERNEL's geometry."""
    ks, s, p = R.GEOMETRY[c.geo]
    r, ref = R.recipe(c), R.reference(c)
    ho, wo = R.out_size(c)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(c.imgs, 3, c.H, c.W, generator=g) + 0.5) * (torch.randint(0, 2, (c.imgs, 3, c.H, c.W), generator=g) * 2 - 1)
    xd, w = x.to(DEV), r.w.to(DEV)
    fwd = torch.full((c.imgs * ho * wo, c.O), NAN, device=DEV)
    L.call('gnx_conv_stem', L.ptr(xd), L.ptr(w), L.ptr(fwd), c.O, c.imgs, 3, c.H, c.W, c.O, ks, ks, s, p, L.stream())
    rows, out = Rows(r.dS, c), Out(c.imgs, c.H, c.W)
    launch(rows, w, out, c)
    lhs = (fwd.cpu().double() * r.dS.double()).sum().item()
    rhs = (x.double() * out.get().cpu().double()).sum().item()
    T_fwd = torch.nn.functional.conv2d(x.double().abs(), r.w.double().abs(), stride=s, padding=p)
    bound = R.G * R.U * ((R.as_rows(T_fwd) * r.dS.double().abs()).sum().item() + (x.double().abs() * ref.T).sum().item())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def test_refusals_leave_the_output_alone():
    c = R.Case(7, 1, 16, 16, 64, 65, 0)
    dS = torch.ones(64 * 65, device=DEV)                      # 8 x 8 positions, up to 65 channels
    w = torch.ones(65 * 3 * 7 * 7, device=DEV)
    out = Out(1, 16, 16)
    st = L.stream()

    def rc(dS_ptr, w_ptr, out_ptr, imgs=1, H=16, W=16, O=64, KH=7, KW=7, stride=2, pad=3, ldd=65):
        code = L.query('gnx_conv0_dgrad', dS_ptr, ldd, w_ptr, out_ptr, imgs, H, W, O, KH, KW, stride, pad, st)
        torch.cuda.synchronize()
        assert out.untouched()
        return code

    a = (L.ptr(dS), L.ptr(w), out.ptr)
    assert rc(*a, O=65) == UNSUPPORTED
    assert rc(*a, KH=5, KW=5, pad=2) == UNSUPPORTED
    assert rc(*a, stride=3) == UNSUPPORTED
    assert rc(*a, pad=1) == UNSUPPORTED and rc(*a, KH=3, KW=3, stride=1, pad=3) == UNSUPPORTED
    assert rc(None, a[1], a[2]) == BAD_ARG and rc(a[0], None, a[2]) == BAD_ARG and rc(a[0], a[1], None) == BAD_ARG
    assert rc(*a, imgs=-1) == BAD_ARG and rc(*a, H=-16) == BAD_ARG and rc(*a, O=-1) == BAD_ARG and rc(*a, ldd=63) == BAD_ARG
    L.call('gnx_conv0_dgrad', a[0], 65, a[1], a[2], 1, 16, 16, 64, 7, 7, 2, 3, st)        # ... and the accepted call does write
    torch.cuda.synchronize()
    assert torch.equal(out.get().cpu(), (64 * R.cover_counts(c)).float().expand(1, 3, 16, 16)) and out.frames_unchanged()
