"""Float64 references of the fp32 weight-gradient entry points of csrc/densenet_bwd.hip (gnx_wgrad_bnrelu, gnx_wgrad_bnrelu_batch,
gnx_conv0_wgrad), their dispatch restated in Python, and the grid of shapes the kernel tests run (test_wgrad_ref_host.py proves
it on the CPU, test_gpu_wgrad_forms.py uses it).  Not imported by the package.

  taps = 1          dW[n][k]         = sum_m dY[m][n] a[m][k]
  taps = 1, pool    the same with a = the 2x2 floor mean of the activated S x S map; m runs over the (S // 2)^2 pooled positions
  taps = 9          dW[n][k][ky][kx] = sum_(img, y, x) dY[(img, y, x)][n] a[(img, y + ky - 1, x + kx - 1)][k]   (zero outside the map)
  stem              dW[o][c][ky][kx] = sum_(img, oy, ox) dS[(img, oy, ox)][o] x[img][c][oy st + ky - pad][ox st + kx - pad]
  a = relu(scale x + shift), evaluated in float64 from the float32 inputs and rounded to float32 (the kernels make that operand
  with one fmaf); a = x without scale / shift.

Tolerance, per element (u = 2^-24):  |err| <= G u T,  T = the sum of the magnitudes of every term of the element's chain (|dW0|
included under `accumulate`).  G = max(8, 4 x the largest ratio |err| / (u T) of two plain fp32 evaluations of the same
contractions - fp32 matmuls on the device, a sequential multiply-add chain on the CPU - over every case of GRID and STEM_GRID):
measured on references only (TORCH_FP32_RATIO: test_gpu_wgrad_forms.py, CHAIN_FP32_RATIO: test_wgrad_ref_host.py).

Detectability.  x, dY, dS: magnitude in [0.5, 1.5], random sign; scale: [0.75, 1.25], random sign per channel; shift: [0.125,
0.25], random sign.  |scale x| >= 0.375 > |shift|, so an activated value is exactly 0 or at least 0.125, and a term is exactly 0
(ReLU, zero padding) or bounded away from 0; another channel's scale or shift flips masks.  `detectable` asks the smallest
non-zero term of a case (a quarter of one activated value times dY under `pool`) to be at least 4 x the case's largest tolerance.
The two stem cases with more tiles than workgroups cannot be shorter than 513 x 128 positions: they draw |x|, |dS| from [0.5,
0.625] (`stem_recipe`), which keeps the smallest term at 0.25 and brings T, and with it the tolerance, down to a third.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from gridnext_amd._lib import CONSTANTS

U = 2.0 ** -24
G_FLOOR = 8.0
# largest |err| / (u T) over GRID and STEM_GRID, and the case it came from
TORCH_FP32_RATIO = 4.3391        # fp32 torch.matmul on the device (test_gpu_wgrad_forms.py)
TORCH_FP32_AT = 'taps 1, M 130, N 260, K 132 (4.17 at taps 9, one 64 x 64 map, N 32, K 128; 3.94 at 256 x 256 x 132; 3.87 at 1000 x 512 x 1028)'
CHAIN_FP32_RATIO = 2.9688        # sequential fp32 multiply-add chain on the CPU (test_wgrad_ref_host.py)
CHAIN_FP32_AT = 'taps 9, 6 maps of 4 x 4, N 32, K 256 (2.77 at 2 maps of 8 x 8, K 256; 2.48 at taps 1, 225 x 128 x 132; stem 1.12 at 513 x 16 x 32)'
G = max(G_FLOOR, 4 * max(TORCH_FP32_RATIO, CHAIN_FP32_RATIO))

WG_BM, WG_KR, LDX = 64, 128, 132             # csrc/densenet_bwd.hip: positions per tile, k range per workgroup, LDS row stride
W_TILE = 32                                  # W1_TILE, W9_TILE
WG_BATCH = 24
LDS_LIMIT = 160 * 1024
BODIES = ('t1', 't9', 'pf', 'plain1', 'pool', 'plain9')
STEM_BODIES = ('fast', 'plain7', 'plain3')
# what gnx_wgrad_bnrelu_form / gnx_conv0_wgrad_form answer
CODES = dict({b: CONSTANTS['GNX_WG_' + b.upper()] for b in BODIES}, **{b: CONSTANTS['GNX_WG_STEM_' + b.upper()] for b in STEM_BODIES})
ERR_BAD_ARG, ERR_UNSUPPORTED = CONSTANTS['GNX_ERR_BAD_ARG'], CONSTANTS['GNX_ERR_UNSUPPORTED']


# ------------------------------------------------------------------------------------------------------------ inputs
def _signed(g, lo, hi, *shape):
    """float32 values with a magnitude in [lo, hi] and a random sign."""
    mag = torch.rand(*shape, generator=g, dtype=torch.float32) * (hi - lo) + lo
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return (mag.clamp_(lo, hi) * sign).double()


def x_rows(c):
    """Rows of X: the unpooled S x S maps under `pool`, else M."""
    return c.imgs * c.S * c.S if c.pool else c.M


@functools.lru_cache(maxsize=4)
def recipe(c):
    """The operands of one case: X [rows][K], dY [M][N], scale / shift [K], dW0 [N][K][taps]; float32 values held in float64.
    Shared between tests: do not write to them."""
    g = torch.Generator().manual_seed(7919 * c.M + 131 * c.N + c.K + 1000003 * (c.taps + 2 * c.pool) + 31 * c.S)
    return NS(X=_signed(g, 0.5, 1.5, x_rows(c), c.K), dY=_signed(g, 0.5, 1.5, c.M, c.N), scale=_signed(g, 0.75, 1.25, c.K),
              shift=_signed(g, 0.125, 0.25, c.K), dW0=_signed(g, 0.5, 1.5, c.N, c.K, c.taps))


NARROW_ABOVE = 32768         # output positions of a stem case from which on the magnitudes are drawn from [0.5, 0.625]


@functools.lru_cache(maxsize=2)
def stem_recipe(s):
    """x [imgs][3][H][W], dS [imgs Ho Wo][O], dW0 [O][3][KH][KH].  Above NARROW_ABOVE positions (the two cases with more tiles
    than workgroups: at least 513 x 128 positions) x and dS keep their smallest magnitude 0.5 and their random signs but stay
    below 0.625: T, and with it the tolerance, is then a third of the full range's while the smallest term is 0.25 as
    everywhere, so that one term stays above four tolerances at that length as well."""
    g = torch.Generator().manual_seed(7919 * s.imgs + 131 * s.H + s.W + 1000003 * s.KH + 31 * s.O + s.pad)
    Ho, Wo = stem_out(s)
    hi = 0.625 if s.imgs * Ho * Wo > NARROW_ABOVE else 1.5
    return NS(x=_signed(g, 0.5, hi, s.imgs, 3, s.H, s.W), dS=_signed(g, 0.5, hi, s.imgs * Ho * Wo, s.O),
              dW0=_signed(g, 0.5, 1.5, s.O, 3, s.KH, s.KH))


# ------------------------------------------------------------------------------------------------------------ references
def activate(X, scale=None, shift=None):
    """a = relu(scale x + shift) in float64, rounded to float32 (held in float64); X itself without scale / shift."""
    if scale is None:
        return X.double()
    return torch.relu(X.double() * scale.double() + shift.double()).float().double()


def pool2(a, imgs, S):
    """2x2 floor mean of [imgs * S * S][K] maps: [imgs * (S // 2)^2][K]; the last row and column of an odd S take no part."""
    So = S // 2
    m = a.view(imgs, S, S, -1)[:, :2 * So, :2 * So]
    m = m.reshape(imgs, So, 2, So, 2, -1)
    return (0.25 * (m[:, :, 0, :, 0] + m[:, :, 0, :, 1] + m[:, :, 1, :, 0] + m[:, :, 1, :, 1])).reshape(imgs * So * So, -1)


def shifted(a, imgs, S, ky, kx):
    """b[(img, y, x)] = a[(img, y + ky - 1, x + kx - 1)], zero outside the map; a [imgs * S * S][K]."""
    m = F.pad(a.view(imgs, S, S, -1), (0, 0, 1, 1, 1, 1))
    return m[:, ky:ky + S, kx:kx + S].reshape(imgs * S * S, -1)


def wgrad1(dY, a):
    """(dW [N][K], T): dW[n][k] = sum_m dY[m][n] a[m][k]."""
    dY, a = dY.double(), a.double()
    return dY.t() @ a, dY.abs().t() @ a.abs()


def wgrad9(dY, a, imgs, S):
    """(dW [N][K][3][3], T): the weight gradient of a pad-1 cross-correlation."""
    dY, a = dY.double(), a.double()
    ref = torch.empty(dY.shape[1], a.shape[1], 3, 3, dtype=torch.float64)
    T = torch.empty_like(ref)
    for ky in range(3):
        for kx in range(3):
            b = shifted(a, imgs, S, ky, kx)
            ref[:, :, ky, kx], T[:, :, ky, kx] = dY.t() @ b, dY.abs().t() @ b.abs()
    return ref, T


def stem_out(s):
    return (s.H + 2 * s.pad - s.KH) // s.stride + 1, (s.W + 2 * s.pad - s.KH) // s.stride + 1


def stem_wgrad(x, dS, KH, stride, pad):
    """(dW [O][3][KH][KH], T) from NCHW patches x [imgs][3][H][W] and dS [(img, oy, ox)][O]."""
    x, dS = x.double(), dS.double()
    imgs, O = x.shape[0], dS.shape[1]
    ref, T = torch.zeros(O, 3 * KH * KH, dtype=torch.float64), torch.zeros(O, 3 * KH * KH, dtype=torch.float64)
    for i0 in range(0, imgs, 64):
        cols = F.unfold(x[i0:i0 + 64], (KH, KH), padding=pad, stride=stride)           # [imgs][3 KH KH][Ho Wo]
        d = dS.view(imgs, -1, O)[i0:i0 + 64]
        ref += torch.einsum('ipl,ilo->op', cols, d)
        T += torch.einsum('ipl,ilo->op', cols.abs(), d.abs())
    return ref.view(O, 3, KH, KH), T.view(O, 3, KH, KH)


@functools.lru_cache(maxsize=4)
def _product(c, act):
    """(ref, T, smallest non-zero |a|) of a case without `accumulate`; ref and T in dW's layout [N][K][taps]."""
    r = recipe(c)
    a = activate(r.X, r.scale, r.shift) if act else activate(r.X)
    a_min = a.abs()[a != 0].min().item()
    if c.pool:
        ref, _ = wgrad1(r.dY, pool2(a, c.imgs, c.S))
        _, T = wgrad1(r.dY, pool2(a.abs(), c.imgs, c.S))
    elif c.taps == 9:
        ref, T = wgrad9(r.dY, a, c.imgs, c.S)
    else:
        ref, T = wgrad1(r.dY, a)
    return ref.reshape(c.N, c.K, c.taps), T.reshape(c.N, c.K, c.taps), a_min


def reference(c, act, acc):
    """(ref, T, smallest non-zero term) of one run of a case, float64, in dW's layout [N][K][taps]."""
    ref, T, a_min = _product(c, act)
    term = a_min * recipe(c).dY.abs().min().item() * (0.25 if c.pool else 1.0)
    if acc:
        d = recipe(c).dW0
        ref, T, term = ref + d, T + d.abs(), min(term, d.abs().min().item())
    return ref, T, term


@functools.lru_cache(maxsize=2)
def _stem_product(s):
    r = stem_recipe(s)
    return stem_wgrad(r.x, r.dS, s.KH, s.stride, s.pad)


def stem_reference(s):
    ref, T = _stem_product(s)
    r = stem_recipe(s)
    term = r.x.abs().min().item() * r.dS.abs().min().item()
    if s.acc:
        ref, T, term = ref + r.dW0, T + r.dW0.abs(), min(term, r.dW0.abs().min().item())
    return ref, T, term


def tol(T, g=None):
    return (G if g is None else g) * U * T


def detectable(term, t):
    """The smallest non-zero term of the case is at least four times its largest tolerance."""
    return term >= 4 * float(t.max())


def ratio(got, ref, T):
    """The largest |err| / (u T); an element without a term (T == 0: every tap but the centre on 1 x 1 maps) must be exactly 0."""
    err = (got.double() - ref).abs()
    r = torch.where(T > 0, err / (U * T.clamp_min(1e-300)), torch.where(err == 0, 0.0, float('inf')).double())
    return torch.nan_to_num(r, nan=float('inf')).max().item()


def sample(n, most):
    """At most `most` indices of range(n), evenly spread, both ends included."""
    if n <= most:
        return torch.arange(n)
    return torch.unique(torch.linspace(0, n - 1, most).round().long())


def chain_fp32(dY, B):
    """dY^T B as a sequential fp32 multiply-add chain over the rows (one rounding for the product, one for the sum)."""
    dY, B = dY.float(), B.float()
    acc = torch.zeros(dY.shape[1], B.shape[1], dtype=torch.float32)
    for m in range(dY.shape[0]):
        acc = acc + dY[m, :, None] * B[m, None, :]
    return acc


def activate_fp32(X, scale=None, shift=None):
    """The activation as an fp32 evaluation would make it (X, scale, shift: float32 tensors on any device)."""
    return X if scale is None else torch.relu(torch.addcmul(shift, X, scale))


# ------------------------------------------------------------------------------------------------------------ dispatch
def _cdiv(a, b):
    return -(-a // b)


def wgrad_splits(M, N, K):
    """wgrad_splits: the position splits of every body but t1 (tiles of 64 positions)."""
    per = _cdiv(N, 128) * _cdiv(K, WG_KR)
    return max(1, min(1024 // per, _cdiv(M, WG_BM), 512))


def wgrad1_t_splits(M, N, K):
    """wgrad1_t_splits: 0 = not a shape of the 128 x 256 transposed-image body."""
    if K % 4 != 0 or K <= 128 or N % 128 != 0:
        return 0
    return min(512 // (_cdiv(K, 256) * (N // 128)), _cdiv(M, W_TILE)) & ~7


def workspace_floats(M, N, K, taps):
    """gnx_wgrad_workspace."""
    s = wgrad_splits(M, N, K)
    if taps == 1:
        s = max(s, wgrad1_t_splits(M, N, K))
    return s * taps * N * K


def lds_bytes(taps, S):
    """Dynamic LDS of the generic bodies (pf, plain1, pool, plain9)."""
    halo, nt = (S + 1, 1) if taps == 9 else (0, 4)
    return (WG_BM * 32 * nt + (WG_BM + 2 * halo) * LDX + WG_BM) * 4


MAX_S_PLAIN9 = max(S for S in range(1, 400) if lds_bytes(9, S) <= LDS_LIMIT)


def form(taps, pool, M, N, K, S, ldx, lddy, x_misaligned=False, dy_misaligned=False, ss_misaligned=False):
    """What one call of gnx_wgrad_bnrelu runs: body (None: GNX_ERR_UNSUPPORTED), the split count actually written, the tile
    size in positions, tiles, tiles per split, the number of splits that own no tile, the dynamic LDS bytes, the workgroups of
    the first launch, whether X (with scale / shift) and dY go through 16-B loads.  ss_misaligned:
    scale / shift are passed and are not 16-B aligned.  The 32-bit offset limit of the t1 body (64 max(ldx, lddy) < 2^28) is
    far above every shape here and is asserted, not modelled."""
    assert 64 * max(ldx, lddy) < (1 << 28)
    x_vec = (not x_misaligned) and ldx % 4 == 0 and not ss_misaligned
    y_vec = (not dy_misaligned) and lddy % 4 == 0
    ns, tile, lds = wgrad_splits(M, N, K), WG_BM, 0
    ns1 = wgrad1_t_splits(M, N, K) if taps == 1 else 0
    if x_vec and y_vec and not pool and ns1 > 0:
        body, ns, tile = 't1', ns1, W_TILE
        wgs = ns1 * _cdiv(K, 256) * (N // 128)
    elif x_vec and y_vec and not pool and taps == 9 and N == 32 and K % 128 == 0 and S in (4, 8, 16, 32) and M % W_TILE == 0:
        body, tile = 't9', W_TILE
        wgs = ns * (K // 128)
    else:
        lds = lds_bytes(taps, S)
        wgs = ns * _cdiv(N, 32 if taps == 9 else 128) * _cdiv(K, WG_KR)
        if lds > LDS_LIMIT:
            body = None
        elif taps == 9:
            body = 'plain9'
        elif pool:
            body = 'pool'
        else:
            body = 'pf' if x_vec and y_vec and K % 4 == 0 and N % 128 == 0 else 'plain1'
    tiles = _cdiv(M, tile)
    tps = _cdiv(tiles, ns)
    empty = sum(1 for s in range(ns) if s * tps >= tiles)
    return NS(body=body, splits=ns, tile=tile, tiles=tiles, tps=tps, empty=empty, lds=lds, workgroups=wgs, x_vec=int(x_vec),
              y_vec=int(y_vec))


def answer(f):
    """(code, workgroups, splits, vec_x, vec_dy) as gnx_wgrad_bnrelu_form gives them for a call of form `f`."""
    if f.body is None:
        return ERR_UNSUPPORTED, 0, 0, 0, 0
    return CODES[f.body], f.workgroups, f.splits, f.x_vec, f.y_vec


def batch_takes(taps, items):
    """gnx_wgrad_bnrelu_batch runs these items (each a `form` of an aligned item plus .S): all t1, or all t9 of one S."""
    want = 't1' if taps == 1 else 't9'
    return all(f.body == want for f in items) and (taps == 1 or len({f.S for f in items}) == 1)


def stem_form(imgs, H, W, O, KH, stride, pad, ldd, x_misaligned=False, ds_misaligned=False):
    """(body, blocks, slabs, workspace floats) of one call of gnx_conv0_wgrad / gnx_conv0_wgrad_workspace."""
    assert (stride, KH) in ((2, 7), (1, 3))
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KH) // stride + 1
    tiles = imgs * _cdiv(Wo, 16) * _cdiv(Ho, 8)
    blocks = min(tiles, 512)
    fast = (stride == 2 and pad == 3 and W % 4 == 0 and O == 64 and Ho % 8 == 0 and Wo % 16 == 0 and ldd % 4 == 0
            and not x_misaligned and not ds_misaligned)
    body = 'fast' if fast else ('plain7' if stride == 2 else 'plain3')
    return NS(body=body, tiles=tiles, blocks=blocks, slabs=4 * blocks, floats=4 * blocks * O * 3 * KH * KH)


# ------------------------------------------------------------------------------------------------------------ layouts
LAYS = ('aligned', 'shifted', 'oddld')


def lay(name, cols):
    """(ld, off, shift) of an operand whose rows hold `cols` floats, as a window [0:rows, off:off+cols] of a [rows + 3][ld]
    tensor that starts `shift` floats into 16-B aligned storage.  aligned: pointer and rows 16-B aligned; shifted: the same
    rows one float further (pointer misaligned, 4 | ld); oddld: pointer aligned, ld = 1 mod 4.  ld > cols, off > 0 everywhere."""
    ld = (cols + 3) // 4 * 4 + 8
    return {'aligned': (ld, 4, 0), 'shifted': (ld, 4, 1), 'oddld': (ld + 1, 4, 0)}[name]


# ------------------------------------------------------------------------------------------------------------ the grid
# ss: scale / shift one float off 16 B (matters only with the activation)
Case = namedtuple('Case', 'taps pool imgs S M N K xlay ylay ss')
FLAGS = ((0, 0), (1, 0), (0, 1), (1, 1))                  # (activation, accumulate): every case runs all four


def one(M, N, K, xlay='aligned', ylay='aligned', ss=0):
    return Case(1, 0, 1, 1, M, N, K, xlay, ylay, ss)


def pooled(imgs, S, N, K, xlay='aligned', ylay='aligned'):
    return Case(1, 1, imgs, S, imgs * (S // 2) ** 2, N, K, xlay, ylay, 0)


def nine(imgs, S, N, K, xlay='aligned', ylay='aligned', ss=0):
    return Case(9, 0, imgs, S, imgs * S * S, N, K, xlay, ylay, ss)


def form_of(c, act=1):
    return form(c.taps, c.pool, c.M, c.N, c.K, c.S, lay(c.xlay, c.K)[0], lay(c.ylay, c.N)[0], c.xlay == 'shifted',
                c.ylay == 'shifted', bool(c.ss and act))


T1, PF = (256, 128, 132), (256, 128, 128)                  # the smallest t1 shape with eight whole tiles; K one block less: pf
T1_EMPTY = ((513, 128, 132), (544, 128, 132))              # 17 tiles over 16 splits of two: splits 9..15 own none
T1_CAP = (1000, 512, 1028)                                 # 512 / (5 * 4) = 25 -> 24 splits, 32 tiles: 16 splits of two, 8 empty
PF_EMPTY = (8200, 1024, 8)                                 # 129 tiles over 128 splits of two: 63 empty
T9_EMPTY = (9, 32, 32, 1024)                               # 288 tiles over 128 splits of three: the last 32 empty
MISLAYS = (('shifted', 'aligned'), ('aligned', 'shifted'), ('oddld', 'aligned'), ('aligned', 'oddld'))
PLAIN1_N, PLAIN1_K = (1, 12, 127, 129, 130), (5, 127, 129)
POOL_S = (2, 3, 6, 7)
T9_S = ((6, 4), (2, 8), (2, 16), (2, 32))                  # (images, S): at least three 32-position tiles, two images


def _grid():
    g = []
    # t1 against pf: K, k blocks, N, tiles; empty splits; the split cap
    g += [one(*PF), one(*T1), one(256, 128, 256), one(256, 128, 260), one(256, 256, 132), one(256, 256, 128)]
    g += [one(224, 128, 132), one(225, 128, 132)]
    g += [one(*s) for s in T1_EMPTY] + [one(512, 128, 132), one(*T1_CAP)]
    # pf: ragged M, one quad of K and a whole k block, two k blocks, empty splits
    g += [one(M, 128, K) for M in (1, 63, 64, 65) for K in (4, 128)]
    g += [one(64, 128, 132), one(*PF_EMPTY)]
    # plain1: ragged N and K; a whole column tile with K off 4 and the other way round
    g += [one(70, N, K) for N in PLAIN1_N for K in PLAIN1_K]
    g += [one(70, 128, K) for K in PLAIN1_K] + [one(70, 129, 128), one(70, 130, 132), one(130, 260, 132)]
    # ... and each way an operand can be off 16 B, on an otherwise-t1 and an otherwise-pf shape
    for shape in (T1, PF):
        g += [one(*shape, xlay=xl, ylay=yl) for xl, yl in MISLAYS] + [one(*shape, ss=1)]
    # pool
    g += [pooled(imgs, S, N, K) for S in POOL_S for imgs in (1, 3) for N, K in ((5, 6), (128, 130))]
    g += [pooled(3, 6, 5, 130), pooled(3, 7, 128, 6), pooled(3, 6, 128, 128, ylay='shifted'), pooled(2, 6, 128, 128, xlay='shifted'),
          pooled(20, 6, 130, 132)]
    # t9
    g += [nine(n, S, 32, K) for n, S in T9_S for K in (128, 256)]
    g += [nine(8, 4, 32, 128), nine(3, 8, 32, 128), nine(*T9_EMPTY)]
    # plain9: maps the t9 body does not take, ragged N and K, an operand off 16 B on a t9 shape, the LDS limit
    g += [nine(1, 64, 32, 128), nine(3, 1, 8, 12), nine(3, 2, 33, 130), nine(2, 3, 8, 130), nine(2, 5, 33, 12), nine(7, 4, 32, 128),
          nine(2, 8, 33, 128), nine(2, 8, 32, 132), nine(2, 8, 8, 128)]
    g += [nine(2, 8, 32, 128, xlay=xl, ylay=yl) for xl, yl in MISLAYS] + [nine(2, 8, 32, 128, ss=1)]
    g += [nine(1, MAX_S_PLAIN9, 8, 8)]
    return list(dict.fromkeys(g))


GRID = _grid()

# (case below, case above, (body, splits) below, (body, splits) above): aligned operands, with the activation
EDGES = [
    (one(*PF), one(*T1), ('pf', 4), ('t1', 8)),
    (one(256, 128, 256), one(256, 128, 260), ('t1', 8), ('t1', 8)),
    (one(*T1), one(256, 256, 132), ('t1', 8), ('t1', 8)),
    (one(224, 128, 132), one(225, 128, 132), ('pf', 4), ('t1', 8)),
    (one(512, 128, 132), one(513, 128, 132), ('t1', 16), ('t1', 16)),
    (one(70, 128, 127), one(64, 128, 128), ('plain1', 2), ('pf', 1)),
    (one(64, 128, 128), one(70, 129, 128), ('pf', 1), ('plain1', 2)),
    (one(*T1), one(70, 130, 132), ('t1', 8), ('plain1', 2)),
    (nine(2, 32, 32, 128), nine(1, 64, 32, 128), ('t9', 32), ('plain9', 64)),
    (nine(2, 8, 32, 128), nine(2, 8, 33, 128), ('t9', 2), ('plain9', 2)),
    (nine(2, 8, 32, 128), nine(2, 8, 32, 132), ('t9', 2), ('plain9', 2)),
    (nine(8, 4, 32, 128), nine(7, 4, 32, 128), ('t9', 2), ('plain9', 2)),
]

# the stem: (imgs, H, W, O, KH, stride, pad, ldd, x one float off 16 B, accumulate)
Stem = namedtuple('Stem', 'imgs H W O KH stride pad ldd xmis acc')


def stem7(imgs, H, W, O=64, pad=3, ldd=None, xmis=0, acc=0):
    return Stem(imgs, H, W, O, 7, 2, pad, O + 8 if ldd is None else ldd, xmis, acc)


def stem3(imgs, H, W, O, pad, acc=0):
    return Stem(imgs, H, W, O, 3, 1, pad, O + 8, 0, acc)


STEM_FAST_MANY, STEM_PLAIN_MANY = stem7(513, 16, 32), stem7(257, 30, 30)       # more tiles than the 512 blocks
STEM_GRID = [
    # fast: one tile per image, two across, two down, a wide dS, accumulate, the prefetch across the grid stride
    stem7(2, 16, 32), stem7(2, 16, 64), stem7(2, 32, 32), stem7(2, 16, 32, ldd=96), stem7(3, 16, 32, acc=1), STEM_FAST_MANY,
    # plain 7x7: each condition of the fast form broken alone, ragged tiles both ways, many tiles
    stem7(2, 16, 32, O=10), stem7(2, 16, 32, O=33), stem7(2, 16, 32, ldd=65), stem7(2, 16, 30), stem7(2, 20, 32),
    stem7(2, 20, 30, O=33, acc=1), stem7(2, 16, 32, pad=0), stem7(2, 16, 32, pad=2), stem7(2, 16, 32, xmis=1), STEM_PLAIN_MANY,
    # 3x3 stride 1
    stem3(2, 9, 9, 10, 0), stem3(2, 9, 9, 64, 1), stem3(2, 16, 16, 64, 1), stem3(2, 16, 16, 10, 0), stem3(2, 17, 17, 64, 1),
    stem3(2, 17, 17, 10, 0, acc=1), stem3(3, 8, 33, 64, 1), stem3(3, 8, 33, 10, 0),
]


def stem_form_of(s):
    return stem_form(s.imgs, s.H, s.W, s.O, s.KH, s.stride, s.pad, s.ldd, bool(s.xmis))
