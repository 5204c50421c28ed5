"""Float64 references of the 3x3-convolution entry points of csrc/conv3x3.hip (gnx_conv3x3_bnrelu, gnx_conv3x3_winograd,
gnx_conv3x3_dgrad_bnrelu_bwd, gnx_conv3x3_f16_dma / _h and the weight re-layouts), their dispatch restated in Python, and the grid
of shapes the kernel tests run (test_conv3_ref_host.py proves it on the CPU, test_gpu_conv3_forms.py uses it).  Not imported by
the package.

  conv    out[(img, y, x)][n] = sum_(ky, kx, k) a[(img, y + ky - 1, x + kx - 1)][k] W[n][k][ky][kx]      (zero outside the map)
          a = relu(scale x + shift) with the prologue (evaluated in float64, not rounded: its fp32 rounding is the kernel's own
          error and T below pays for it), a = x without
  wino    the same sum, a = x; only T differs (below)
  adj     g = conv(dY, Wb) with K = 32 channels in, N = 128 out;  d = g [a > 0];  dX = scale d;
          dbeta[c] (+)= sum_m d[m][c];  dgamma[c] (+)= sum_m d[m][c] xhat[m][c],  xhat = ((a - shift) / scale - mean) invstd
  h32/h16 conv of the fp16-rounded operands (both forms accumulate in fp32); h16 stores the result rounded to fp16

Tolerance, per element (u = 2^-24):  |err| <= G u T.  T is the sum of the magnitudes of every term of the element's chain:
  conv    sum |a| |W|, with the prologue (|x| |scale| + |shift|) in place of |a| (ReLU-zeroed values included: the bound of the
          activation's own rounding does not know the sign)
  wino    the terms as Winograd forms them.  Along a row, per output pair p and kernel row: V0 = d0 - d2, V1 = d1 + d2,
          V2 = d2 - d1, V3 = d1 - d3 (d = the four inputs 2p - 1 .. 2p + 2, zero outside the row), U0 = g0, U1 = (g0 + g1 + g2)
          / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2;  Tm_xi = sum_(rows, k) |V_xi| |U_xi|;  T(2p) = Tm0 + Tm1 + Tm2, T(2p + 1) = Tm1 +
          Tm2 + Tm3 (the output transform with absolute values)
  adj     T_g = sum |dY| |Wb|;  dX: |scale| T_g [a > 0];  dbeta: sum_m T_g [a > 0] (+ |dbeta0|);  dgamma: sum_m T_g [a > 0]
          (|a| / |scale| + |shift| / |scale| + |mean|) |invstd| (+ |dgamma0|): every term of the expanded expression
  h16     G u T + half an fp16 ulp of the result (taken at |ref| + G u T)

G = max(8, 4 x the largest ratio |err| / (u T) of plain fp32 evaluations of the *reference operation* against float64 over every
case of GRID), separately for the direct forms, Winograd and the adjoint sums; the kernels' own error has no part in it:
                                                          direct            Winograd          adjoint sums
  fp32 F.conv2d on the device (test_gpu_conv3_forms.py)   TORCH_FP32_RATIO  -                 TORCH_FP32_SUM_RATIO
  sequential fp32 multiply-add chain on the CPU           CHAIN_FP32_RATIO  -                 CHAIN_FP32_SUM_RATIO
  CPU fp32 emulation of the F(2,3)-along-x algebra        -                 WINO_FP32_RATIO   -
  measured:  direct 4.1767 (device) and 4.5568 (chain): G = 18.227;  Winograd 2.3925: G_WINO = 9.570;  sums 0.1024 and 0.2069:
  G_SUMS = 8 (the floor)
(where each occurred: the constants below).  The CPU measurements run in test_conv3_ref_host.py, the device one in
test_gpu_conv3_forms.py; each prints its figures and holds them to G / 4.  The device measurement covers the direct cases (conv,
adj, fp16 operands); the Winograd cases are measured through the emulation of their own algebra.

Detectability.  Activations, gradients and weights: magnitude in [0.5, 1.5], random sign - every product term is at least 0.25.
Prologue: |scale| in [1.5, 2], |shift| in [0.125, 0.25], random signs: |scale x| >= 0.75, so a pre-activation is at least 0.5
from zero (fp32 rounding cannot flip the ReLU) and an activated value is exactly 0 or at least 0.5.  The adjoint's stored
activation a is 0 or in [0.5, 1.5]; |scale|, invstd in [0.875, 1.125], |shift|, |mean| in [1/32, 1/16], so |xhat| >= (0.4375 /
1.125 - 0.0625) 0.875 = 0.28 wherever a > 0.
`detectable` asks the smallest non-zero term of a case to be at least 4 x its largest tolerance: one dropped, doubled or
misplaced tap fails.  It holds for every output map of every case; for dbeta / dgamma it is asserted up to ADJ_SUMS_DETECT_ROWS
rows (a sum over more rows cannot see one term in fp32: T grows with the rows, 288 a row and column.  There the sums detect the
loss of one wave's share of one tile - 32 rows of |g| around 18 - and each term is seen through dX).  h16: the half-ulp term
alone reaches 0.0625 at results above 128, so the fp16 output is also held bit-equal to the fp32-output form's result rounded
once (the same kernel body), and `detectable` is asserted on the fp32 part.

The 8-wave forms need 262144 rows (64 MB of activations): their references are computed on whole sampled images (`sampled_images`:
the first and last two tiles, the tiles on both sides of every round boundary, 8 random others).
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from gridnext_amd._lib import CONSTANTS

U = 2.0 ** -24
G_FLOOR = 8.0
MIN_TERM = 0.25
# largest |err| / (u T) over GRID and the case it came from
TORCH_FP32_RATIO = 4.1767        # fp32 F.conv2d on the device (test_gpu_conv3_forms.py)
TORCH_FP32_AT = '64 maps of 64 x 64, K 64, N 32 (3.84 at one map of 48 x 48, K 8; 3.50 at 79 x 79; 2.81 at the adjoint, one map of 64 x 64)'
CHAIN_FP32_RATIO = 4.5568         # sequential fp32 multiply-add chain on the CPU (test_conv3_ref_host.py)
CHAIN_FP32_AT = 'adjoint, 9 maps of 64 x 64 (4.545 at fp16 operands, 2048 maps of 4 x 4, K 128; 4.530 at 256 maps of 32 x 32, K 32, N 64)'
WINO_FP32_RATIO = 2.3925         # CPU fp32 emulation of the F(2,3)-along-x algebra (test_conv3_ref_host.py)
WINO_FP32_AT = '4112 maps of 4 x 4, K 32 (2.31 at 4096 maps; 2.00 at 2 maps of 64 x 64, K 64)'
TORCH_FP32_SUM_RATIO = 0.1024    # dbeta / dgamma from the device's fp32 conv2d and fp32 column sums
TORCH_FP32_SUM_AT = '8 maps of 4 x 4 (0.088 at 2 maps of 8 x 8; 0.033 at 64 maps of 4 x 4)'
CHAIN_FP32_SUM_RATIO = 0.2069     # ... from the CPU chain and a sequential fp32 sum over the rows
CHAIN_FP32_SUM_AT = '2 maps of 8 x 8 (0.155 at 8 maps of 4 x 4; 0.12 at 33 maps of 32 x 32)'
G = max(G_FLOOR, 4 * max(TORCH_FP32_RATIO, CHAIN_FP32_RATIO))
G_WINO = max(G_FLOOR, 4 * WINO_FP32_RATIO)
G_SUMS = max(G_FLOOR, 4 * max(TORCH_FP32_SUM_RATIO, CHAIN_FP32_SUM_RATIO))

C3_BM, C3_BN, LDK = 128, 32, 36                    # csrc/conv3x3.hip, csrc/fwd_common.h
LDS_LIMIT = 160 * 1024
MAX_WGS = 256                                      # persistent forms: one workgroup per CU
DMA_S = (4, 7, 8, 14, 16, 28, 32, 56, 64)          # map sizes conv3x3_dma_kernel is instantiated for (fp32)
POW2_S = (4, 8, 16, 32, 64)                        # Winograd, the fused adjoint, fp16
WIDE_ROWS = 1024 * 256                             # from here on (and 256 | M, S <= 32): 8 waves, 256-row tiles
# include/gridnext_hip.h: GNX_C3_* (generic ... dmag8, wino, wino8)
CODES = {k[len('GNX_C3_'):].lower(): v for k, v in CONSTANTS.items() if k.startswith('GNX_C3_')}
BODIES = ('generic', 'pipe5', 'pipe6', 'pipe7', 'pipe9', 'dma4', 'dma8', 'dmag4', 'dmag8')
ADJ_SUMS_DETECT_ROWS = 128


# ------------------------------------------------------------------------------------------------------------ the cases
# op: conv | wino | adj | h32 | h16;  n images of S x S;  act: BN+ReLU prologue (conv only)
# lay: al = every operand 16-B aligned; ash = A (dY) one float off; aodd = lda % 4 == 1; ssh = scale and shift one float off;
#      wsh = the weights one float off.  big: the leading dimensions are 1024 (+ 1 for the output) instead of a small excess
Case = namedtuple('Case', 'op n S K N act lay big')


def rows(c):
    return c.n * c.S * c.S


def conv(n, S, K, N, act=0, lay='al', big=0):
    return Case('conv', n, S, K, N, act, lay, big)


def wino(n, S, K, big=0):
    return Case('wino', n, S, K, 32, 0, 'al', big)


def adj(n, S, big=0):
    return Case('adj', n, S, 32, 128, 0, 'al', big)


def f16(n, S, K, out16=0, big=0):
    return Case('h16' if out16 else 'h32', n, S, K, 32, 0, 'al', big)


def layout(c):
    """How a case lies in memory.  A (dY) is the window [pad : pad + M, 4 : 4 + K] of a [pad + M + pad][lda] sentinel-filled
    tensor that starts `a_shift` floats into 16-B aligned storage, pad = S + 17 rows (more than the S + 1 halo rows and the 16-row
    DMA group the kernels may touch beyond either end); `out` (dX) the window [pad : pad + M, c_off : c_off + N] of a [..][ldc]
    tensor, c_off 1 or 3 floats, ldc odd; the adjoint's stored activation a third window with an lda of its own.  fp16
    operands count in halves: lda16 a multiple of 8, column offset 8."""
    half = c.op in ('h32', 'h16')
    unit = 8 if half else 4
    lda = 1024 if c.big else (c.K + unit - 1) // unit * unit + 2 * unit
    if c.lay == 'aodd':
        lda += 1
    ldc = 1025 if c.big else (c.N + 4) | 1
    return NS(pad=c.S + 17, lda=lda, a_off=unit, a_shift=1 if c.lay == 'ash' else 0, ldc=ldc, c_off=1 if c.N % 3 else 3,
              ss_shift=1 if c.lay == 'ssh' else 0, w_shift=1 if c.lay == 'wsh' else 0,
              ld_act=1024 + 4 if c.big else c.N + 12, act_off=4)


# ------------------------------------------------------------------------------------------------------------ inputs
def _signed(g, lo, hi, *shape):
    """float32 values with a magnitude in [lo, hi] and a random sign."""
    u = torch.rand(*shape, generator=g, dtype=torch.float32)
    s = torch.randint(0, 2, shape, generator=g, dtype=torch.int8)
    return u.mul_(hi - lo).add_(lo).clamp_(lo, hi).mul_(s.float().mul_(2).sub_(1))


def _seed(c):
    return 7919 * c.n + 131 * c.S + 1000003 * c.K + 31 * c.N + {'conv': 1, 'wino': 2, 'adj': 3, 'h32': 4, 'h16': 4}[c.op]


@functools.lru_cache(maxsize=3)
def _recipe(op, n, S, K, N):
    c = Case(op, n, S, K, N, 0, 'al', 0)
    g = torch.Generator().manual_seed(_seed(c))
    M = rows(c)
    r = NS(X=_signed(g, 0.5, 1.5, M, K), W=_signed(g, 0.5, 1.5, N, K, 3, 3))
    if op == 'conv':
        r.scale, r.shift = _signed(g, 1.5, 2.0, K), _signed(g, 0.125, 0.25, K)
    elif op in ('h32', 'h16'):
        r.X, r.W = r.X.half().float(), r.W.half().float()
    elif op == 'adj':
        # X = dY [M][32]; W = conv2's weight [32][128][3][3] (its data gradient has 128 channels out); act = the stored
        # activation: 0 or in [0.5, 1.5]
        r.W = _signed(g, 0.5, 1.5, K, N, 3, 3)
        r.act = _signed(g, 0.5, 1.5, M, N).clamp_min_(0)
        r.scale, r.shift = _signed(g, 0.875, 1.125, N), _signed(g, 0.03125, 0.0625, N)
        r.mean, r.invstd = _signed(g, 0.03125, 0.0625, N), _signed(g, 0.875, 1.125, N).abs_()
        r.dbeta0, r.dgamma0 = _signed(g, 0.5, 1.5, N), _signed(g, 0.5, 1.5, N)
    return r


def recipe(c):
    """The operands of a case as float32 tensors (layout-independent; shared between tests: do not write to them).
    conv / wino / h32 / h16: X [M][K], W [N][K][3][3] (torch's layout), scale / shift [K] (conv).  adj: X = dY [M][32],
    W = conv2's weight [32][128][3][3], act [M][128], scale / shift / mean / invstd [128], dbeta0 / dgamma0 [128]."""
    return _recipe(c.op, c.n, c.S, c.K, c.N)


def dgrad_weight(W):
    """conv2's weight [O][I][3][3] as the weight of its data gradient, a pad-1 cross-correlation with I channels out:
    Wd[i][o][ky][kx] = W[o][i][2 - ky][2 - kx]."""
    return W.flip(2, 3).permute(1, 0, 2, 3).contiguous()


def repack(W):
    """gnx_repack_conv3x3: [N][K][3][3] -> [tap][N][K]."""
    return W.reshape(W.shape[0], W.shape[1], 9).permute(2, 0, 1).contiguous()


def repack_bwd(W):
    """gnx_repack_conv3x3_bwd: [N][K][3][3] -> [8 - tap][K][N]."""
    return W.reshape(W.shape[0], W.shape[1], 9).flip(2).permute(2, 1, 0).contiguous()


def winograd_weights(W):
    """gnx_winograd_conv3x3_weights, operation for operation in W's dtype: [N][K][3][3] -> [row][xi][N][K]."""
    g0, g1, g2 = W[:, :, :, 0], W[:, :, :, 1], W[:, :, :, 2]
    u = torch.stack([g0, 0.5 * ((g0 + g2) + g1), 0.5 * ((g0 + g2) - g1), g2], 0)         # [xi][N][K][row]
    return u.permute(3, 0, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------ references
def conv2(a, W, n, S):
    """The zero-padded 3x3 cross-correlation per image: a [n S S][K], W [N][K][3][3] -> [n S S][N], in a's dtype."""
    out = torch.empty(a.shape[0], W.shape[0], dtype=a.dtype)
    per = max(1, (1 << 22) // (S * S * max(a.shape[1], W.shape[0])))
    for i0 in range(0, n, per):
        i1 = min(n, i0 + per)
        m = a[i0 * S * S:i1 * S * S].view(i1 - i0, S, S, -1).permute(0, 3, 1, 2)
        out[i0 * S * S:i1 * S * S] = F.conv2d(m, W, padding=1).permute(0, 2, 3, 1).reshape(-1, W.shape[0])
    return out


def naive_conv(a, W, n, S):
    """The same by loops over (image, y, x) and the taps, in float64: what conv2 is proven against."""
    a, W = a.double(), W.double()
    out = torch.zeros(n * S * S, W.shape[0], dtype=torch.float64)
    for img in range(n):
        for y in range(S):
            for x in range(S):
                for ky in range(3):
                    for kx in range(3):
                        yy, xx = y + ky - 1, x + kx - 1
                        if 0 <= yy < S and 0 <= xx < S:
                            out[(img * S + y) * S + x] += W[:, :, ky, kx] @ a[(img * S + yy) * S + xx]
    return out


def activate(X, scale, shift):
    """(a, |a| bound): relu(scale x + shift) and |x| |scale| + |shift|, float64."""
    X, scale, shift = X.double(), scale.double(), shift.double()
    return torch.relu(X * scale + shift), X.abs() * scale.abs() + shift.abs()


def wino_pairs(a, n, S):
    """V [n][S + 2][S / 2][4][K]: the input transform of every output pair of every row, one zero row above and below each
    image (a [n S S][K], in a's dtype)."""
    m = F.pad(a.view(n, S, S, -1), (0, 0, 1, 1, 1, 1))                                    # [n][S + 2][S + 2][K]
    d0, d1, d2, d3 = m[:, :, 0:S:2], m[:, :, 1:S + 1:2], m[:, :, 2:S + 2:2], m[:, :, 3:S + 3:2]
    return torch.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], 3)


def wino_T(a, W, n, S):
    """The magnitude sum of the terms as Winograd forms them, [n S S][N] float64."""
    V, Uw = wino_pairs(a.double(), n, S).abs(), winograd_weights(W.double()).abs()        # Uw [row][xi][N][K]
    Tm = torch.zeros(n, S, S // 2, 4, W.shape[0], dtype=torch.float64)
    for dy in range(3):
        Tm += torch.einsum('iypxk,xnk->iypxn', V[:, dy:dy + S], Uw[dy])
    T = torch.stack([Tm[:, :, :, 0] + Tm[:, :, :, 1] + Tm[:, :, :, 2], Tm[:, :, :, 1] + Tm[:, :, :, 2] + Tm[:, :, :, 3]], 3)
    return T.reshape(n * S * S, -1)


def wino_fp32(a, W, n, S):
    """The F(2,3)-along-x algebra in fp32 on the CPU: the input transform in fp32, the weights as winograd_weights_kernel
    forms them, a sequential multiply-add chain over (row, k) per xi, the output transform (m0 + m1) + m2, (m1 - m2) - m3."""
    V, Uw = wino_pairs(a.float(), n, S), winograd_weights(W.float())
    acc = torch.zeros(n, S, S // 2, 4, W.shape[0], dtype=torch.float32)
    for dy in range(3):
        for k in range(a.shape[1]):
            acc = acc + V[:, dy:dy + S, :, :, k, None] * Uw[dy, :, :, k]
    m0, m1, m2, m3 = acc.unbind(3)
    return torch.stack([(m0 + m1) + m2, (m1 - m2) - m3], 3).reshape(n * S * S, -1)


def chain_fp32(a, W, n, S):
    """The convolution as a sequential fp32 multiply-add chain over (tap, k) on the CPU (one rounding for the product, one
    for the sum); a [n S S][K] float32."""
    a, W = a.float(), W.float()
    m = F.pad(a.view(n, S, S, -1), (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(n, S, S, W.shape[0], dtype=torch.float32)
    for ky in range(3):
        for kx in range(3):
            b = m[:, ky:ky + S, kx:kx + S]
            for k in range(a.shape[1]):
                acc = acc + b[:, :, :, k, None] * W[:, k, ky, kx]
    return acc.reshape(n * S * S, -1)


def sampled_tiles(tiles, wgs):
    """The tiles a sampled reference covers: the first and last two, both sides of every round boundary, 8 random others."""
    t = {0, 1, tiles - 2, tiles - 1}
    for b in range(wgs, tiles, wgs):
        t |= {b - 1, b}
    g = torch.Generator().manual_seed(tiles)
    t |= set(torch.randint(0, tiles, (8,), generator=g).tolist())
    return sorted(x for x in t if 0 <= x < tiles)


def is_huge(c):
    return rows(c) >= WIDE_ROWS - 256


def sampled_images(c):
    """None: the whole case.  Else the sorted images whose rows the reference covers (whole images holding the sampled tiles)."""
    if not is_huge(c):
        return None
    f = form_of(c)
    ss = c.S * c.S
    imgs = set()
    for t in sampled_tiles(f.T, f.G):
        imgs |= set(range(t * f.bm // ss, ((t + 1) * f.bm - 1) // ss + 1))
    return sorted(i for i in imgs if i < c.n)


def image_rows(c, imgs):
    ss = c.S * c.S
    return (torch.tensor(imgs)[:, None] * ss + torch.arange(ss)[None, :]).reshape(-1)


@functools.lru_cache(maxsize=3)
def _reference(op, n, S, K, N, act):
    c = Case(op, n, S, K, N, act, 'al', 0)
    r = recipe(c)
    imgs = sampled_images(c)
    idx = None if imgs is None else image_rows(c, imgs)
    X = r.X if idx is None else r.X[idx]
    ni = n if imgs is None else len(imgs)
    W = dgrad_weight(r.W) if op == 'adj' else r.W
    if act:
        a, amag = activate(X, r.scale, r.shift)
        nz = a[a != 0]
        a_min = nz.min().item() if nz.numel() else MIN_TERM / 0.5
    else:
        a = amag = X.double()
        a_min = 0.5
        amag = amag.abs()
    ref = conv2(a, W.double(), ni, S)
    T = wino_T(a, W, ni, S) if op == 'wino' else conv2(amag, W.double().abs(), ni, S)
    return NS(rows=idx, imgs=imgs, n=ni, ref=ref, T=T, term=a_min * 0.5)


def reference(c):
    """NS(rows, imgs, n, ref, T, term) of the convolution of a case (for adj: g = the data gradient before the mask), float64.
    rows: None when ref covers the whole case, else the row indices it covers (whole images, ascending); term: the smallest
    non-zero term.  Shared: do not write to it."""
    return _reference(c.op, c.n, c.S, c.K, c.N, c.act)


@functools.lru_cache(maxsize=None)
def _adjoint_sums(n, S):
    """dbeta, dgamma, their T and the smallest non-zero term of the sums over ALL rows of an adj case, image chunk by image
    chunk (small results: kept for the whole run)."""
    c = adj(n, S)
    r = recipe(c)
    W = dgrad_weight(r.W).double()
    sc, sh, mu, inv = (t.double() for t in (r.scale, r.shift, r.mean, r.invstd))
    ss = S * S
    per = max(1, 32768 // ss)
    o = NS(dbeta=torch.zeros(c.N, dtype=torch.float64), T_dbeta=torch.zeros(c.N, dtype=torch.float64),
           dgamma=torch.zeros(c.N, dtype=torch.float64), T_dgamma=torch.zeros(c.N, dtype=torch.float64), sum_term=MIN_TERM)
    for i0 in range(0, n, per):
        i1 = min(n, i0 + per)
        X, act = r.X[i0 * ss:i1 * ss].double(), r.act[i0 * ss:i1 * ss].double()
        mask = (act > 0).double()
        d, Td = conv2(X, W, i1 - i0, S) * mask, conv2(X.abs(), W.abs(), i1 - i0, S) * mask
        xhat = ((act - sh) / sc - mu) * inv
        xmag = (act.abs() / sc.abs() + sh.abs() / sc.abs() + mu.abs()) * inv.abs()
        o.dbeta += d.sum(0)
        o.T_dbeta += Td.sum(0)
        o.dgamma += (d * xhat).sum(0)
        o.T_dgamma += (Td * xmag).sum(0)
        live = xhat.abs()[act > 0]
        o.sum_term = min(o.sum_term, MIN_TERM * live.min().item())
    return o


def adjoint(c, accumulate=0):
    """The fused data gradient of an adj case: NS(rows, dX, T_dX, term - on the rows `reference` covers - and dbeta, T_dbeta,
    dgamma, T_dgamma, sum_term over all rows)."""
    r, g, s = recipe(c), reference(c), _adjoint_sums(c.n, c.S)
    act = (r.act if g.rows is None else r.act[g.rows]).double()
    sc = r.scale.double()
    mask = (act > 0).double()
    o = NS(rows=g.rows, dX=sc * g.ref * mask, T_dX=sc.abs() * g.T * mask, term=g.term * sc.abs().min().item(),
           dbeta=s.dbeta, T_dbeta=s.T_dbeta, dgamma=s.dgamma, T_dgamma=s.T_dgamma, sum_term=s.sum_term)
    if accumulate:
        o.dbeta, o.T_dbeta = o.dbeta + r.dbeta0.double(), o.T_dbeta + r.dbeta0.double().abs()
        o.dgamma, o.T_dgamma = o.dgamma + r.dgamma0.double(), o.T_dgamma + r.dgamma0.double().abs()
    return o


def half_ulp16(x):
    """Half an fp16 ulp at magnitude x (float64 tensor)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return 0.5 * torch.pow(2.0, e - 10)


def tol(T, g=None):
    return (G if g is None else g) * U * T


def g_of(c):
    return G_WINO if c.op == 'wino' else G


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


# ------------------------------------------------------------------------------------------------------------ dispatch
def _cdiv(a, b):
    return -(-a // b)


def lds_bytes(S):
    """Dynamic LDS of the generic and the register-pipelined bodies."""
    return ((C3_BM + 2 * S + 2) * LDK + 9 * 32 * LDK + LDK) * 4


MAX_S = max(S for S in range(1, 600) if lds_bytes(S) <= LDS_LIMIT)


def _persistent(f, M, S, bm, ragged=False):
    """The tile schedule of a persistent body: T tiles of bm rows over G workgroups, `full` rounds in the XCD-permuted order
    (when xcd) and a last round of `partial` tiles in the plain order; head / tail: the tiles whose strip [t bm - S - 1, + SR)
    leaves the array at its start / end (16-row groups there load from clamped addresses)."""
    f.bm = bm
    f.T = _cdiv(M, bm) if ragged else M // bm
    f.G = min(f.T, MAX_WGS)
    f.gy = 1
    f.full, f.partial = f.T // f.G, f.T % f.G
    f.rounds = f.full + (1 if f.partial else 0)
    f.xcd = f.G % 8 == 0
    f.ragged = M % bm if ragged else 0
    SR = (bm + 2 * S + 2 + 15) // 16 * 16
    f.head = sum(1 for t in range(f.T) if t * bm - S - 1 < 0)
    f.tail = sum(1 for t in range(f.T) if t * bm - S - 1 + SR > M)
    f.one_strip = f.T == 1                      # both array ends in one strip
    return f


def _wide(M, S):
    return S <= 32 and M % 256 == 0 and M >= WIDE_ROWS


def form(M, N, K, S, lda, ldc, act, a_mis=False, ss_mis=False, w_mis=False):
    """What one call of gnx_conv3x3_bnrelu runs: body (None: GNX_ERR_UNSUPPORTED), the grid (G, gy), the tiles T and, for
    the persistent bodies, the schedule of `_persistent`."""
    f = NS(body=None, G=0, gy=0, T=0, bm=C3_BM)
    if lds_bytes(S) > LDS_LIMIT:
        return f
    vec_a = (not a_mis) and lda % 4 == 0 and K % 4 == 0 and not (act and ss_mis)
    vec_w = (not w_mis) and K % 4 == 0
    fast = vec_a and vec_w
    dma = (not act) and fast and M % C3_BM == 0 and M * max(lda, ldc) < (1 << 31) and S in DMA_S
    if dma and N == C3_BN and K % 64 == 0:
        f.body = 'dma8' if _wide(M, S) else 'dma4'
    elif dma and K == 32 and N % 64 == 0:
        f.body = 'dmag8' if _wide(M, S) else 'dmag4'
    if f.body:
        return _persistent(f, M, S, 256 if f.body[-1] == '8' else 128)
    nj = _cdiv(C3_BM + 2 * S + 2, 32)
    f.body = 'generic' if not fast or nj > 9 else 'pipe5' if nj <= 5 else 'pipe6' if nj == 6 else 'pipe7' if nj == 7 else 'pipe9'
    f.G = f.T = _cdiv(M, C3_BM)
    f.gy = _cdiv(N, C3_BN)
    return f


def wino_form(M, N, K, S, lda, ldc, a_mis=False, w_mis=False):
    f = NS(body=None, G=0, gy=0, T=0, bm=256)
    if N != 32 or K % 32 or a_mis or w_mis or lda % 4 or M * max(lda, ldc) >= (1 << 31) or S not in POW2_S:
        return f
    f.body = 'wino'
    return _persistent(f, M, S, 256, ragged=True)


def adj_form(M, N, K, S, lddy, lda, lddx, dy_mis=False, w_mis=False):
    """body: adj4 / adj8 (the waves per workgroup); the slabs the reduction reads: G x waves."""
    f = NS(body=None, G=0, gy=0, T=0, bm=128)
    if K != 32 or N != 128 or M % C3_BM or dy_mis or w_mis or lddy % 4 or M * max(lddy, lda, lddx) >= (1 << 31) or S not in POW2_S:
        return f
    f.waves = 8 if _wide(M, S) else 4
    f.body = 'adj%d' % f.waves
    return _persistent(f, M, S, 32 * f.waves)


def f16_form(M, N, K, S, lda16, ldc, a_mis=False, w_mis=False):
    """body: h4 / h8; resident: the weight images are fetched with the workgroup's first two chunks only (K == 128)."""
    f = NS(body=None, G=0, gy=0, T=0, bm=128)
    if N != 32 or K % 128 or M % C3_BM or lda16 % 8 or a_mis or w_mis or M * max(lda16, ldc) >= (1 << 31) or S not in POW2_S:
        return f
    f.waves = 8 if _wide(M, S) else 4
    f.body = 'h%d' % f.waves
    f.resident = K == 128
    return _persistent(f, M, S, 32 * f.waves)


def form_of(c):
    lo = layout(c)
    M = rows(c)
    if c.op == 'conv':
        return form(M, c.N, c.K, c.S, lo.lda, lo.ldc, c.act, c.lay == 'ash', c.lay == 'ssh', c.lay == 'wsh')
    if c.op == 'wino':
        return wino_form(M, c.N, c.K, c.S, lo.lda, lo.ldc)
    if c.op == 'adj':
        return adj_form(M, c.N, c.K, c.S, lo.lda, lo.ld_act, lo.ldc)
    return f16_form(M, c.N, c.K, c.S, lo.lda, lo.ldc)


# ------------------------------------------------------------------------------------------------------------ the grid
WIDE_N = {4: WIDE_ROWS // 16, 32: WIDE_ROWS // 1024, 64: WIDE_ROWS // 4096}     # images of 262144 rows
FEWEST = ((8, 4), (2, 8), (1, 16), (1, 32), (1, 64))                      # (images, S): the fewest images with 128 | M
ODD_S = ((128, 7), (32, 14), (8, 28), (2, 56))                            # M = 6272 = 49 tiles
DMA_TILES = (1, 7, 8, 9, 255, 256, 257, 512)                               # at S = 4: 8 images a tile
FAST_LOST = ('ash', 'aodd', 'ssh', 'wsh')


def _conv_grid():
    g = []
    # generic / pipe: the strip-rows-per-thread edges, one or two images, with and without the prologue
    for S in (15, 16, 31, 32, 47, 48, 79, 80):
        g += [conv(1 + (S < 40), S, 8, 32, act) for act in (0, 1)]
    g += [conv(2, 8, 36, 33, 1), conv(2, 16, 40, 31, 1, big=1), conv(1, 32, 96, 32, 1), conv(1, 48, 8, 64, 0)]
    # `fast` lost by each single cause (the base runs pipe5 with the prologue, dma4 without), and K % 4 != 0 with the
    # ld4_safe tails of 1, 3 and 1 past a whole chunk
    g += [conv(2, 8, 64, 32, act) for act in (0, 1)]
    g += [conv(2, 8, 64, 32, act, lay) for lay in FAST_LOST for act in (0, 1)]
    g += [conv(2, 8, K, 32, act) for K in (1, 3, 33, 62) for act in (0, 1)]
    # N = 1, 31, 33 and 64 (grid.y = 2); M not a multiple of 128; S = 1
    g += [conv(2, 8, 8, N, 1) for N in (1, 31, 33, 64)] + [conv(2, 8, 6, N, 0) for N in (1, 33)]
    g += [conv(9, 4, 8, 32, 1), conv(3, 5, 8, 32, 0), conv(3, 5, 7, 5, 1), conv(1, 1, 8, 4, 1), conv(1, 1, 1, 1, 0), conv(200, 1, 8, 32, 1),
          conv(130, 1, 5, 33, 0), conv(5, 2, 8, 32, 1)]
    # dma4: one, two and three chunk pairs; every S at the fewest images; the odd sizes at 49 tiles
    g += [conv(2, 8, K, 32) for K in (64, 128, 192)] + [conv(1, 32, K, 32) for K in (128, 192)]
    g += [conv(n, S, 64, 32) for n, S in FEWEST + ODD_S]
    g += [conv(1, 32, 64, 32, big=1), conv(128, 7, 64, 32, big=1)]
    # ... each neighbour that must fall to pipe (or, for S = 12, has no instantiation)
    g += [conv(2, 8, 96, 32), conv(2, 8, 64, 64), conv(8, 12, 64, 32), conv(2, 8, 64, 32, 1), conv(9, 4, 64, 32)]
    # ... tile and round counts
    g += [conv(8 * t, 4, 64, 32) for t in DMA_TILES] + [conv(514, 8, 64, 32), conv(33, 32, 64, 32)]
    # dma8 and beside it: one tile less (4 waves), M % 256 != 0 (4 waves), S = 64 (4 waves by design), a partial round
    g += [conv(WIDE_N[4], 4, 64, 32), conv(WIDE_N[4] + 16, 4, 64, 32), conv(WIDE_N[4] - 8, 4, 64, 32), conv(WIDE_N[4] + 8, 4, 64, 32),
          conv(WIDE_N[32], 32, 64, 32), conv(WIDE_N[32] + 1, 32, 64, 32), conv(WIDE_N[64], 64, 64, 32)]
    # dmag4 / dmag8: K = 32 channels in
    g += [conv(2, 8, 32, N) for N in (64, 128, 192)] + [conv(2, 8, 32, 96), conv(2, 8, 32, 128, 1)]
    g += [conv(n, S, 32, 64) for n, S in FEWEST + ODD_S]
    g += [conv(8 * t, 4, 32, 64) for t in (1, 8, 9, 257)] + [conv(8 * 257, 4, 32, 128, big=1), conv(WIDE_N[32], 32, 32, 64)]
    return list(dict.fromkeys(g))


def _wino_grid():
    g = [wino(n, S, 32) for n, S in FEWEST] + [wino(2, 8, K) for K in (64, 96)] + [wino(1, 32, 96, big=1)]
    g += [wino(1, 4, 32), wino(17, 4, 32), wino(5, 8, 64), wino(1, 16, 32)]                # M = 16; ragged last tiles
    g += [wino(16 * t, 4, 32) for t in (8, 9, 256, 257)] + [wino(16 * 257 + 1, 4, 32), wino(2, 64, 64)]
    return list(dict.fromkeys(g))


def _adj_grid():
    g = [adj(n, S) for n, S in FEWEST] + [adj(8 * t, 4) for t in (8, 9, 257)] + [adj(33, 32, big=1), adj(9, 64), adj(2, 8, big=1)]
    g += [adj(WIDE_N[32], 32)]
    return list(dict.fromkeys(g))


def _f16_grid():
    g = []
    for K in (128, 256):
        g += [f16(8 * t, 4, K) for t in (1, 256, 257)] + [f16(n, S, K) for n, S in FEWEST]
    g += [f16(8 * 257, 4, 128, out16=1), f16(8 * 257, 4, 256, out16=1), f16(2, 8, 256, out16=1), f16(1, 32, 128, out16=1, big=1),
          f16(1, 64, 256, big=1), f16(WIDE_N[32], 32, 128), f16(WIDE_N[4], 4, 128, out16=1)]
    return list(dict.fromkeys(g))


CONV_GRID, WINO_GRID, ADJ_GRID, F16_GRID = _conv_grid(), _wino_grid(), _adj_grid(), _f16_grid()
GRID = CONV_GRID + WINO_GRID + ADJ_GRID + F16_GRID

# (case on one side, case on the other, body, body): the edges between two bodies of gnx_conv3x3_bnrelu
EDGES = [
    (conv(2, 15, 8, 32, 1), conv(2, 16, 8, 32, 1), 'pipe5', 'pipe6'),
    (conv(2, 31, 8, 32, 1), conv(2, 32, 8, 32, 1), 'pipe6', 'pipe7'),
    (conv(1, 47, 8, 32, 1), conv(1, 48, 8, 32, 1), 'pipe7', 'pipe9'),
    (conv(1, 79, 8, 32, 1), conv(1, 80, 8, 32, 1), 'pipe9', 'generic'),
    (conv(2, 8, 64, 32, 1), conv(2, 8, 64, 32, 1, 'ash'), 'pipe5', 'generic'),
    (conv(2, 8, 64, 32, 1), conv(2, 8, 64, 32, 1, 'aodd'), 'pipe5', 'generic'),
    (conv(2, 8, 64, 32, 1), conv(2, 8, 64, 32, 1, 'ssh'), 'pipe5', 'generic'),
    (conv(2, 8, 64, 32, 1), conv(2, 8, 64, 32, 1, 'wsh'), 'pipe5', 'generic'),
    (conv(2, 8, 64, 32, 1), conv(2, 8, 62, 32, 1), 'pipe5', 'generic'),
    (conv(2, 8, 64, 32, 0), conv(2, 8, 64, 32, 0, 'ash'), 'dma4', 'generic'),
    (conv(2, 8, 64, 32, 0), conv(2, 8, 64, 32, 0, 'ssh'), 'dma4', 'dma4'),          # no prologue: scale / shift are not passed
    (conv(2, 8, 64, 32, 0), conv(2, 8, 96, 32, 0), 'dma4', 'pipe5'),
    (conv(2, 8, 64, 32, 0), conv(2, 8, 64, 64, 0), 'dma4', 'pipe5'),
    (conv(2, 8, 64, 32, 0), conv(2, 8, 64, 32, 1), 'dma4', 'pipe5'),
    (conv(8, 4, 64, 32, 0), conv(9, 4, 64, 32, 0), 'dma4', 'pipe5'),
    (conv(2, 8, 64, 32, 0), conv(8, 12, 64, 32, 0), 'dma4', 'pipe5'),
    (conv(WIDE_N[4] - 8, 4, 64, 32), conv(WIDE_N[4], 4, 64, 32), 'dma4', 'dma8'),
    (conv(WIDE_N[4], 4, 64, 32), conv(WIDE_N[4] + 8, 4, 64, 32), 'dma8', 'dma4'),
    (conv(WIDE_N[32], 32, 64, 32), conv(WIDE_N[64], 64, 64, 32), 'dma8', 'dma4'),
    (conv(2, 8, 32, 64), conv(2, 8, 32, 96), 'dmag4', 'pipe5'),
    (conv(2, 8, 32, 128), conv(2, 8, 32, 128, 1), 'dmag4', 'pipe5'),
    (conv(8 * 257, 4, 32, 64), conv(WIDE_N[32], 32, 32, 64), 'dmag4', 'dmag8'),
]
# tile counts (T) that must occur per persistent body
TILE_EDGES = {'dma4': (1, 7, 8, 9, 255, 256, 257, 512), 'dmag4': (1, 8, 9, 257), 'wino': (1, 8, 9, 256, 257, 258), 'adj4': (1, 8, 9, 257),
              'h4': (1, 256, 257)}
