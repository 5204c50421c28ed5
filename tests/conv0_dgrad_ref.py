"""Float64 reference of gnx_conv0_dgrad (csrc/conv0_dgrad.hip), the gradient of the stem convolution with respect to the
patches, and the grid of shapes the kernel tests run (test_conv0_dgrad_ref_host.py proves it on the CPU, test_gpu_conv0_dgrad.py
uses it).  Not imported by the package.

  dX[i][c][y][x] = sum_(o, ky, kx) dS[(i Ho + yo) Wo + xo][o] w[o][c][ky][kx],   yo stride = y + pad - ky, xo stride = x + pad - kx,
  integer yo in [0, Ho), xo in [0, Wo):  F.conv_transpose2d of the conv0 map's gradient with conv0's own weight, in float64.

Tolerance, per element (u = 2^-24):  |err| <= G u T,  T = conv_transpose(|dS|, |w|), the sum of the magnitudes of every term.
G = max(8, 4 x the largest ratio |err| / (u T) of two plain fp32 evaluations of the same operation against float64 over every
case of GRID); the kernel's own error has no part in it:
  torch's fp32 F.conv_transpose2d on the CPU                           TORCH_FP32_RATIO
  a sequential fp32 multiply-add chain over (ky, kx, o) on the CPU      CHAIN_FP32_RATIO
  measured (rounded up): 3.1910 (torch) and 5.1572 (chain): G = 20.629
(where each occurred: the constants below; measured by test_conv0_dgrad_ref_host.py, which prints its figures).

Detectability.  dS and w: magnitude in [0.5, 1.5], random sign - every term is at least 0.25 in magnitude, and T <= 64 x 16 x
2.25 = 2304, so the largest tolerance is at most G u 2304 = 2.9e-3: one dropped, doubled or misplaced tap, position or channel
fails (`detectable`).  The all-ones case is exact: dX = O x the number of windows that cover the pixel, an integer below 2^24.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

U = 2.0 ** -24
G_FLOOR = 8.0
MIN_TERM = 0.25
# largest |err| / (u T) over GRID and the case it came from
# (the torch figure is INFORMATIONAL: its blocking follows the thread count, so the host test holds what it measures to G / 4 and
# below the chain's figure, not to this constant; G rests on the chain's ratio, which is pinned)
TORCH_FP32_RATIO = 3.1910        # torch's fp32 F.conv_transpose2d on the CPU, 8 threads
TORCH_FP32_AT = '3x3, 3 images of 32 x 32, O 64 (2.94 at 7x7, 3 images of 16 x 16, O 64; 2.88 at 7x7, 3 images of 128 x 128, O 8)'
CHAIN_FP32_RATIO = 5.1572        # sequential fp32 multiply-add chain on the CPU
CHAIN_FP32_AT = '3x3, 130 images of 16 x 16, O 64 (3.89 at 7x7, 3 images of 224 x 224, O 64; 3.84 at 7x7, one image of 128 x 128, O 64)'
G = max(G_FLOOR, 4 * max(TORCH_FP32_RATIO, CHAIN_FP32_RATIO))

GEOMETRY = {7: (7, 2, 3), 3: (3, 1, 1)}          # window -> (KS, stride, pad)

# geo: 7 | 3 (the window);  imgs images of H x W;  O channels of dS, leading dimension ldd;  shift: dS starts `shift` floats off
# a 16-B boundary
Case = namedtuple('Case', 'geo imgs H W O ldd shift')


def ids(c):
    return '-'.join(str(v) for v in c)


def out_size(c):
    ks, s, p = GEOMETRY[c.geo]
    return (c.H + 2 * p - ks) // s + 1, (c.W + 2 * p - ks) // s + 1


SHAPES = {7: ((16, 16), (18, 18), (21, 21), (16, 24), (128, 128), (224, 224)),         # baseline, odd conv map, odd patch (the last
          3: ((5, 5), (16, 16), (32, 32))}                                             # row and column: the other parity), H != W,
LAYOUTS = ((8, 8), (10, 22), (10, 24), (64, 64), (64, 256))                                      # the shipping and the reference's geometry
# (O, ldd): O = 10, ldd = 22: the small_inputs tiny net's block buffer - not a multiple of 4, the scalar path; O = 10, ldd = 24: the
# 16-B path with a partial last group of 4 channels (read by single floats inside it); ldd = 256: a window of a block buffer


def _grid():
    g = [Case(geo, imgs, H, W, O, ldd, 0) for geo in (7, 3) for H, W in SHAPES[geo] for imgs in (1, 3) for O, ldd in LAYOUTS]
    g += [Case(geo, 130, 16, 16, 64, 64, 0) for geo in (7, 3)]              # more images than any cap on a launch's tiles
    g += [Case(7, 3, 21, 21, 64, 64, 1), Case(3, 3, 5, 5, 8, 8, 1)]         # dS one float off a 16-B boundary (4 | ldd: scalar path)
    return g


GRID = _grid()


# ------------------------------------------------------------------------------------------------------------ inputs
def _signed(g, lo, hi, *shape):
    """float32 values with a magnitude in [lo, hi] and a random sign."""
    u = torch.rand(*shape, generator=g, dtype=torch.float32)
    s = torch.randint(0, 2, shape, generator=g, dtype=torch.int8)
    return u.mul_(hi - lo).add_(lo).clamp_(lo, hi).mul_(s.float().mul_(2).sub_(1))


@functools.lru_cache(maxsize=4)
def _recipe(geo, imgs, H, W, O):
    c = Case(geo, imgs, H, W, O, O, 0)
    ho, wo = out_size(c)
    g = torch.Generator().manual_seed(7919 * imgs + 131 * H + 17 * W + 1000003 * O + geo)
    return NS(dS=_signed(g, 0.5, 1.5, imgs * ho * wo, O), w=_signed(g, 0.5, 1.5, O, 3, geo, geo))


def recipe(c):
    """The operands of a case as float32 tensors (layout-independent; shared: do not write to them): dS [imgs Ho Wo][O], the
    gradient of the conv0 map, rows in (image, y, x) order, and w [O][3][KS][KS], conv0's weight in torch's layout."""
    return _recipe(c.geo, c.imgs, c.H, c.W, c.O)


def as_map(dS, c):
    """dS [imgs Ho Wo][O] -> NCHW [imgs][O][Ho][Wo]."""
    ho, wo = out_size(c)
    return dS.view(c.imgs, ho, wo, -1).permute(0, 3, 1, 2)


def as_rows(m):
    """NCHW [imgs][O][Ho][Wo] -> rows [imgs Ho Wo][O]."""
    return m.permute(0, 2, 3, 1).reshape(-1, m.shape[1])


# ------------------------------------------------------------------------------------------------------------ references
def dgrad(dS, w, c):
    """conv0's adjoint in its input: F.conv_transpose2d in the operands' dtype; dS [imgs Ho Wo][O] -> [imgs][3][H][W]."""
    ks, s, p = GEOMETRY[c.geo]
    ho, wo = out_size(c)
    opad = (c.H - ((ho - 1) * s - 2 * p + ks), c.W - ((wo - 1) * s - 2 * p + ks))
    return F.conv_transpose2d(as_map(dS, c), w, stride=s, padding=p, output_padding=opad)


def dgrad_autograd(dS, w, c):
    """The same as autograd derives it from F.conv2d (what the model's backward must equal)."""
    ks, s, p = GEOMETRY[c.geo]
    x = torch.zeros(c.imgs, 3, c.H, c.W, dtype=dS.dtype, requires_grad=True)
    F.conv2d(x, w, stride=s, padding=p).backward(as_map(dS, c))
    return x.grad


def _stuffed(dS, c):
    """dS on the patch's own lattice: [imgs][O][H + KS - 1][W + KS - 1], position (yo, xo) at (KS - 1 - pad + yo stride, ...),
    zeros elsewhere - tap (ky, kx) of pixel (y, x) is element (y + KS - 1 - ky, x + KS - 1 - kx)."""
    ks, s, p = GEOMETRY[c.geo]
    ho, wo = out_size(c)
    up = torch.zeros(c.imgs, dS.shape[1], c.H + ks - 1, c.W + ks - 1, dtype=dS.dtype)
    off = ks - 1 - p
    up[:, :, off:off + (ho - 1) * s + 1:s, off:off + (wo - 1) * s + 1:s] = as_map(dS, c)
    return up


def chain_fp32(dS, w, c):
    """The sum as a sequential fp32 multiply-add chain over (ky, kx, o) on the CPU (one rounding for the product, one for the
    sum), written from the definition: independent of torch's convolutions."""
    ks = c.geo
    up, w = _stuffed(dS.float(), c), w.float()
    acc = torch.zeros(c.imgs, 3, c.H, c.W, dtype=torch.float32)
    for ky in range(ks):
        for kx in range(ks):
            win = up[:, :, ks - 1 - ky:ks - 1 - ky + c.H, ks - 1 - kx:ks - 1 - kx + c.W]
            for o in range(c.O):
                acc = acc + win[:, o, None] * w[o, :, ky, kx].view(1, 3, 1, 1)
    return acc


def cover_counts(c):
    """[H][W] int64: how many windows of the convolution cover each pixel, counted tap by tap from the definition."""
    ks, s, p = GEOMETRY[c.geo]
    ho, wo = out_size(c)

    def along(n, no):
        return torch.tensor([sum(1 for k in range(ks) if (v + p - k) % s == 0 and 0 <= (v + p - k) // s < no) for v in range(n)])
    return along(c.H, ho)[:, None] * along(c.W, wo)[None, :]


@functools.lru_cache(maxsize=4)
def _reference(geo, imgs, H, W, O):
    c = Case(geo, imgs, H, W, O, O, 0)
    r = recipe(c)
    return NS(ref=dgrad(r.dS.double(), r.w.double(), c), T=dgrad(r.dS.double().abs(), r.w.double().abs(), c), term=MIN_TERM)


def reference(c):
    """NS(ref, T, term) of a case, float64 [imgs][3][H][W]; term: the smallest non-zero term.  Shared: do not write to it."""
    return _reference(c.geo, c.imgs, c.H, c.W, c.O)


def tol(T, g=None):
    return (G if g is None else g) * U * T


def detectable(term, t):
    """The smallest non-zero term of the case is at least four times its largest tolerance."""
    return term >= 4 * float(t.max())


def ratio(got, ref, T):
    """The largest |err| / (u T); an element without a term must be exactly 0."""
    err = (got.double() - ref).abs()
    r = torch.where(T > 0, err / (U * T.clamp_min(1e-300)), torch.where(err == 0, 0.0, float('inf')).double())
    return torch.nan_to_num(r, nan=float('inf')).max().item()


def flagged(got, ref, t):
    """The comparator of the kernel tests: any element off by more than its tolerance, or not finite."""
    return bool((~((got.double() - ref).abs() <= t)).any())
