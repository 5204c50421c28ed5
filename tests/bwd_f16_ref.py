"""Float64 references of the fp16 gradient path (csrc/dense_bwd_f16.hip and the two conv1x1_h16 tile forms of
csrc/densenet_f16.hip), its dispatch restated in Python, and the grid of shapes the kernel tests run (test_bwd_f16_ref_host.py
proves it on the CPU, test_gpu_bwd_f16_forms.py uses it).  Not imported by the package.

  wgrad1      dW[n][k]          = 1/s sum_m dY[m][n] a[m][k],  a = fp16(relu(fp32 fma(x, scale, shift))) or x itself
  wgrad3      dW[n][k][ky][kx]  = 1/s sum_p dY[p - (ky - 1, kx - 1)][n] A[p][k]              (pixels outside the map: no term)
  dgrad3      d[p][m] = [A[p][m] > 0] sum_(tap, n) dY[p - (dy, dx)][n] W2[n][m][tap];  dB = fp16(d scale2[m]);
              dbeta2 = 1/s sum_p d,  dgamma2 = 1/s (S1 - beta2 S0) / gamma2 with S0 = sum_p d, S1 = sum_p d A (the stored activation)
  conv3       dgrad3 and wgrad3 of the same operands (gnx_conv3x3_bwd_f16_lb)
  dgrad1      d[p][c] = [fma(x, scale, shift) > 0] sum_m dB[p][m] W1[m][c];  G = fp16(d scale[c] + G0);
              dbeta1 = 1/s sum_p d,  dgamma1 = 1/s invstd sum_p d (x - mean);  dW1[m][c] = 1/s sum_p dB[p][m] a[p][c]
  tail        v = [fma > 0] dfeats[img][c] / S2;  G = fp16(v scale s);  dbeta = sum v,  dgamma = invstd sum v (x - mean)   (true scale)
  trans       v = [fma > 0] dP[pool(p)][c] / 4;   G = fp16(v scale);    dbeta = 1/s sum v,  dgamma = 1/s invstd sum v (x - mean)
  cols        out = G / s, exactly
  h16         out = fp16(relu(oscale y + oshift)) or fp16(y),  y[m][n] = sum_k a[m][k] W[n][k]

The only rounding points are the kernels': the activated operand is fp16(relu(fp32 fma)), masks come from that same fp32 fma,
weights are fp16 values, sums are exact, fp32 results are multiplied by 1/s (a power of two), fp16 results are rounded once.

Tolerance, per element (u = 2^-24):  fp32 outputs |err| <= G u T,  T = the sum of the magnitudes of the element's terms (the prior
value included under `accumulate`; for dgamma2 both sums before the division);  fp16 outputs |err| <= 2^-11 |ref| + G u T' + 2^-25,
T' the fp32 chain feeding the rounding (G0 included for conv1's data gradient).  G = max(8, 4 x the largest ratio |err| / (u T) of
two plain fp32 evaluations of the same contractions over every case of GRID):
    fp32 torch.matmul on the device            4.70572  (recorded rounded up, TORCH_FP32_RATIO = 4.7058; all outputs; conv2's data gradient as a [1024][288] x [288][128] product, one 32 x 32 map;
                                                        4.44 at 4088 maps of 4 x 4, 4.33 at the tail sums of 2 maps of 7 x 7, 4.10 at
                                                        wgrad1 1600 x 512 x 1024; test_gpu_bwd_f16_forms.py)
    sequential fp32 multiply-add chain, CPU    11.5272  (on 16 x 16 evenly spread outputs of every contraction, not on all of
                                                        them: a Python loop over the contraction; the tail's column sums S0, 2 maps of 7 x 7, C 32: one value is added 49
                                                        times over, the rounding errors of equal addends do not cancel; 2.37 at
                                                        wgrad3, 2 maps of 7 x 7; test_bwd_f16_ref_host.py)
G = max(8, 4 x 11.5272) = 46.11.  The kernels take no part in it; both measurements stay runnable and print their figures.

Inputs (`recipe`).  Every operand is an fp16 value.  Gradients (dY, dB, dP, dfeats), activations and priors: magnitude in
[0.5, 1.5] (the conv1 / conv2 passes and long cases [0.5, 0.625], below), random sign; weights [0.5, 0.75]; scale, gamma, invstd [0.75, 1.25] with a random sign
per channel (invstd positive); shift, beta, mean [1/32, 1/16] (`tight`) or [0.125, 0.25], random sign.  |scale x| >= 0.375 > |shift|:
no pre-activation is nearer to 0 than 0.125 = 2^-3 (the host test asserts >= 2^-6 on every case), so the fp32 fma and an exact
evaluation agree on every mask and NO element is left out of any comparison.  The stored activation A of conv2 is exactly 0 or
in [0.5, 0.625].  A term is exactly 0 or bounded away from 0; `detectable` asks each output's smallest non-zero term to be at
least 4 x its largest tolerance.  A chain of n equal terms has T >= n min|term|, so that holds only below 2^24 / (4 G) terms:
the BatchNorm sums of the conv1 and conv2 passes (pixels x 128 and x 288 products) pass it by a thinner mask - the share of
positive pre-activations (`density_for`) is a half up to TERMS products per channel and falls as 1 / M from there, every tile
keeping live elements - and by the narrow magnitudes [0.5, 0.625], as wgrad_ref.stem_recipe does; no tolerance is widened.
A thinned case (`thinned`) leaves most of dB / G without a contraction result (0 or G0 exactly), so it runs a second time on
the `dense` recipe - half of the mask live - with dgamma = dbeta = NULL: dB, G and both weight gradients, whose chains stay
short enough, are then compared on a dense mask at the same shape and slab plan.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from gridnext_amd._lib import CONSTANTS

U, UH, HALF_SUB = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
G_FLOOR = 8.0
# largest |err| / (u T) over GRID, and the case it came from
TORCH_FP32_RATIO = 4.7058
TORCH_FP32_AT = 'conv2 data gradient as a [1024][288] x [288][128] product, one 32 x 32 map (4.44 at 4088 maps of 4 x 4; 4.33 at the tail sums, 2 maps of 7 x 7; 4.10 at wgrad1 1600 x 512 x 1024)'
CHAIN_FP32_RATIO = 11.5272
CHAIN_FP32_AT = 'tail, 2 maps of 7 x 7, C 32: the column sums S0 add one value 49 times over (2.37 at wgrad3, 2 maps of 7 x 7)'
G = max(G_FLOOR, 4 * max(TORCH_FP32_RATIO, CHAIN_FP32_RATIO))

ERR_BAD_ARG, ERR_UNSUPPORTED = CONSTANTS['GNX_ERR_BAD_ARG'], CONSTANTS['GNX_ERR_UNSUPPORTED']
BODIES = ('WG1', 'WG1_ACT', 'WG3', 'WG3_PAD', 'DG3', 'DG3_PAD', 'C3', 'DG1', 'DG1_WG', 'TAIL', 'TRANS')
H16_BODIES = ('M128', 'M256')
CODES = dict({b: CONSTANTS['GNX_B16_' + b] for b in BODIES}, **{b: CONSTANTS['GNX_H16_' + b] for b in H16_BODIES})
NAMES = {v: k for k, v in CODES.items()}
POW2_MAPS = (4, 8, 16, 32, 64)
CAP_DGRAD1, CAP_DGRAD1_WGRAD, CAP_WGRAD1, SLABS_3X3 = 768, 512, 768, 512
C3_WORKGROUPS = 256
H16_M256_FROM = 131072
COLS_MAX_BLOCKS = 4096
NARROW_FROM = 8192           # rows from which on the magnitudes are drawn from [0.5, 0.625]


# --------------------------------------------------------------------------------------------------------- the dispatch
def plan_slabs(M, tile, want):
    """plan_slabs of dense_bwd_f16.hip: (tiles, slabs, per)."""
    tiles = -(-M // tile)
    slabs = max(1, min(max(want, 1), tiles))
    per = -(-tiles // slabs)
    slabs = max(1, -(-tiles // per) if per > 0 else 1)
    return NS(tiles=tiles, slabs=slabs, per=per)


def slabs_for(cap, blocks):
    return max(8, cap // blocks // 8 * 8)


def plan_wgrad1(M, N, K):
    return plan_slabs(M, 64, slabs_for(CAP_WGRAD1, -(-K // 128) * -(-N // 128)))


def plan_dgrad1(M, K, wgrad):
    return plan_slabs(M, 64, slabs_for(CAP_DGRAD1_WGRAD if wgrad else CAP_DGRAD1, -(-K // 128)))


def conv3_bwd_grid(M):
    return max(1, min(M // 128, C3_WORKGROUPS))


def tail_slots(imgs, C):
    return max(1, min(256 * 512 // (C // 8), imgs))


def trans_slots(Mp, C):
    return max(1, min(256 * 2048 // (C // 8), Mp))


def _al16(*ptrs):
    return all(p % 16 == 0 for p in ptrs if p is not None)


def _refused(code):
    return NS(code=code, workgroups=0, slabs=0, per=0, slots=0, blocked=0)


def _slab_form(body, plan, blocks=1):
    return NS(code=CODES[body], body=body, workgroups=-(-plan.slabs // 8) * 8 * blocks if blocks else plan.slabs, slabs=plan.slabs,
              per=plan.per, tiles=plan.tiles)


def form_wgrad1(a):
    """gnx_wgrad1x1_f16 on the arguments `a` (a namespace by the header's parameter names; pointers are addresses or None)."""
    if (not (a.dY16 and a.X16 and a.dW and a.workspace and a.ls) or a.M <= 0 or a.N <= 0 or a.K <= 0 or a.lddy < a.N or a.ldx < a.K
            or (a.scale is None) != (a.shift is None)):
        return _refused(ERR_BAD_ARG)
    if a.N % 8 or a.K % 8 or a.lddy % 8 or a.ldx % 8 or not _al16(a.dY16, a.X16):
        return _refused(ERR_UNSUPPORTED)
    return _slab_form('WG1_ACT' if a.scale else 'WG1', plan_wgrad1(a.M, a.N, a.K), -(-a.K // 128) * -(-a.N // 128))


def _conv2_args_bad(a, extra):
    return (not all(extra) or not (a.dY16 and a.A16 and a.workspace and a.ls) or a.M <= 0 or a.S <= 0 or a.lddy < 32
            or a.M % (a.S * a.S) != 0 or a.lda < 32 or a.bsa < 32)


def form_wgrad3(a):
    if _conv2_args_bad(a, [a.dW]):
        return _refused(ERR_BAD_ARG)
    if a.lddy % 8 or a.lda % 8 or a.bsa % 8 or not _al16(a.dY16, a.A16) or a.S > 64:
        return _refused(ERR_UNSUPPORTED)
    f = _slab_form('WG3_PAD' if a.M % 64 == 0 and a.S in POW2_MAPS else 'WG3', plan_slabs(a.M, 64, SLABS_3X3), 0)
    return f


def form_dgrad3(a):
    if _conv2_args_bad(a, [a.W2b16, a.dB16, a.scale2, a.gamma2, a.beta2]):
        return _refused(ERR_BAD_ARG)
    if a.lddy % 8 or a.lda % 8 or a.bsa % 8 or not _al16(a.dY16, a.A16, a.dB16, a.W2b16) or a.S > 64:
        return _refused(ERR_UNSUPPORTED)
    return _slab_form('DG3_PAD' if a.M % 128 == 0 and a.S in POW2_MAPS else 'DG3', plan_slabs(a.M, 128, SLABS_3X3), 0)


def form_conv3(a):
    if _conv2_args_bad(a, [a.W2b16, a.dB16, a.dW, a.scale2, a.gamma2, a.beta2]):
        return _refused(ERR_BAD_ARG)
    if (a.lddy % 8 or a.lda % 8 or a.bsa % 8 or not _al16(a.dY16, a.A16, a.dB16, a.W2b16) or a.M % 128 != 0
            or a.S not in POW2_MAPS):
        return _refused(ERR_UNSUPPORTED)
    grid, tiles = conv3_bwd_grid(a.M), a.M // 128
    per = -(-tiles // grid)
    used = -(-tiles // per)
    return NS(code=CODES['C3'], body='C3', workgroups=used, slabs=used, per=per, tiles=tiles, grid=grid)


def form_dgrad1(a):
    if (not (a.dB16 and a.W1t16 and a.X16 and a.G16 and a.scale and a.shift and a.mean and a.invstd and a.workspace and a.ls)
            or a.M <= 0 or a.K <= 0 or a.ldx < 32 or a.ldg < 32 or a.bsx < 32 or a.bsg < 32 or (a.bsx == 32 and a.ldx < a.K)
            or (a.bsg == 32 and a.ldg < a.K)):
        return _refused(ERR_BAD_ARG)
    if a.K % 32 or a.ldx % 8 or a.ldg % 8 or a.bsx % 8 or a.bsg % 8 or not _al16(a.dB16, a.W1t16, a.X16, a.G16):
        return _refused(ERR_UNSUPPORTED)
    wg = a.dW is not None
    return _slab_form('DG1_WG' if wg else 'DG1', plan_dgrad1(a.M, a.K, wg), -(-a.K // 128))


def _slot_form(body, slots, blocked, C):
    threads = (-(-slots // 16) * 16 if blocked else slots) * (C // 8)
    return NS(code=CODES[body], body=body, slots=slots, workgroups=-(-threads // 256), blocked=blocked, slabs=slots)


def form_tail(a):
    if (not (a.dfeats and a.X16 and a.G16 and a.scale and a.shift and a.mean and a.invstd and a.workspace and a.ls) or a.imgs <= 0
            or a.C <= 0 or a.S2 <= 0 or a.ldf < a.C or a.ldx < 32 or a.ldg < 32 or a.bsx < 32 or a.bsg < 32
            or (a.bsx == 32 and a.ldx < a.C) or (a.bsg == 32 and a.ldg < a.C)):
        return _refused(ERR_BAD_ARG)
    blocked = int(a.bsx != 32 or a.bsg != 32)
    if (a.C % 8 or a.ldf % 4 or a.ldx % 8 or a.ldg % 8 or a.bsx % 8 or a.bsg % 8 or not _al16(a.dfeats, a.X16, a.G16)
            or (blocked and a.C % 32)):
        return _refused(ERR_UNSUPPORTED)
    return _slot_form('TAIL', tail_slots(a.imgs, a.C), blocked, a.C)


def form_trans(a):
    if (not (a.dP16 and a.X16 and a.G16 and a.scale and a.shift and a.mean and a.invstd and a.workspace and a.ls) or a.imgs <= 0
            or a.C <= 0 or a.S < 2 or a.ldp < 32 or a.ldx < 32 or a.ldg < 32 or a.bsp < 32 or a.bsx < 32 or a.bsg < 32
            or (a.bsp == 32 and a.ldp < a.C) or (a.bsx == 32 and a.ldx < a.C) or (a.bsg == 32 and a.ldg < a.C)):
        return _refused(ERR_BAD_ARG)
    blocked = int(a.bsp != 32 or a.bsx != 32 or a.bsg != 32)
    if (a.C % 8 or a.S % 2 or a.ldp % 8 or a.ldx % 8 or a.ldg % 8 or a.bsp % 8 or a.bsx % 8 or a.bsg % 8
            or not _al16(a.dP16, a.X16, a.G16) or (blocked and a.C % 32)):
        return _refused(ERR_UNSUPPORTED)
    return _slot_form('TRANS', trans_slots(a.imgs * (a.S // 2) ** 2, a.C), blocked, a.C)


def form_h16(a, cb):
    """gnx_conv1x1_bnrelu_h16 (cb = 0: ldc16) / _cb (cb = 1: rows_total): (code, workgroups)."""
    if cb and a.rows_total < a.M:
        return _refused(ERR_BAD_ARG)
    ldc, obs = (32, a.rows_total * 32) if cb else (a.ldc16, 32)
    if (not (a.A16 and a.W16 and a.out16) or (a.scale is None) != (a.shift is None) or (a.out_scale is None) != (a.out_shift is None)
            or a.M < 0 or a.N <= 0 or a.K <= 0 or a.lda16 < a.K or (ldc < a.N if obs == 32 else (ldc != 32 or a.N % 32 != 0))):
        return _refused(ERR_BAD_ARG)
    if not _al16(a.A16, a.W16, a.out16, a.scale, a.shift) or a.lda16 % 8 or a.K % 8 or a.N % 8 or ldc % 8:
        return _refused(ERR_UNSUPPORTED)
    rows = 256 if a.M >= H16_M256_FROM else 128
    body = 'M256' if rows == 256 else 'M128'
    return NS(code=CODES[body], body=body, workgroups=-(-a.M // rows) * -(-a.N // 128))


def cols_blocks(M, C):
    return min(-(-(M * (C // 8)) // 256), COLS_MAX_BLOCKS)


# workspace sizes in floats, from the restated plans (include/gridnext_hip.h documents the formulas)
def ws_wgrad1(M, N, K):
    return plan_wgrad1(M, N, K).slabs * N * K


def ws_wgrad3(M):
    return plan_slabs(M, 64, SLABS_3X3).slabs * 9 * 32 * 128


def ws_dgrad3(M):
    return plan_slabs(M, 128, SLABS_3X3).slabs * 256


def ws_conv3(M):
    return conv3_bwd_grid(M) * (256 + 9 * 32 * 128)


def ws_dgrad1(M, K, wgrad):
    cw = -(-K // 128) * 128
    return plan_dgrad1(M, K, wgrad).slabs * ((2 + 128) if wgrad else 2) * cw


def ws_tail(imgs, C):
    return tail_slots(imgs, C) * 2 * C


def ws_trans(imgs, C, S):
    return trans_slots(imgs * (S // 2) ** 2, C) * 2 * C


# ------------------------------------------------------------------------------------------------------------ inputs
def _h(x):
    return x.half().double()


def _signed(g, lo, hi, *shape):
    """fp16 values (held in float64) with a magnitude in [lo, hi] and a random sign."""
    mag = (torch.rand(*shape, generator=g, dtype=torch.float32) * (hi - lo) + lo).clamp_(lo, hi)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return _h(mag * sign)


def _chan(g, lo, hi, C, positive=False):
    v = _signed(g, lo, hi, C)
    return v.abs() if positive else v


def _live(g, M, C, density):
    """The elements whose pre-activation is positive: a share `density`, drawn per element, and one in every 64-row tile."""
    pos = torch.rand(M, C, generator=g) < density
    t = torch.arange(-(-M // 64))
    pos[torch.minimum(64 * t + t % 64, torch.tensor(M - 1)), (5 * t) % C] = True
    return pos


def _masked_x(g, M, C, scale, density, hi):
    """X with scale x > 0 on the `_live` elements and < 0 elsewhere."""
    mag = _signed(g, 0.5, hi, M, C).abs()
    pos = _live(g, M, C, density)
    return mag * torch.where(pos, 1.0, -1.0).double() * torch.sign(scale)


TERMS = 16384               # the longest BatchNorm chain a case may have: 2^24 / (16 G) holds up to G = 64


def density_for(M, terms_per_row):
    """The share of positive pre-activations: a half, less where M * share * terms_per_row would pass TERMS."""
    return min(0.5, float(TERMS) / (M * terms_per_row))


def thinned(family, c):
    """Whether the case's mask is thinner than a half: it then also runs `dense`, without the BatchNorm sums."""
    if family in ('dgrad3', 'conv3', 'wgrad3'):
        return density_for(c.imgs * c.S * c.S, 288) < 0.5
    return family == 'dgrad1' and density_for(c.M, 128) < 0.5


def _hi(M):
    return 0.625 if M >= NARROW_FROM else 1.5


def _bn(g, C, tight):
    lo, hi = (1 / 32, 1 / 16) if tight else (0.125, 0.25)
    return NS(scale=_chan(g, 0.75, 1.25, C), shift=_chan(g, lo, hi, C), mean=_chan(g, lo, hi, C), invstd=_chan(g, 0.75, 1.25, C, True))


def _seed(*v):
    s = 0
    for x in v:
        s = (s * 1000003 + int(x) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------------------------------------ references
def act16(X, scale, shift):
    """(a, z): z = the fp32 fma(x, scale, shift) (the product and the sum are exact in float64: one rounding), a = fp16(relu(z))."""
    z = (X.double() * scale.double() + shift.double()).float()
    return torch.relu(z).half().double(), z.double()


def shifted(a, imgs, S, ky, kx):
    """b[(img, y, x)] = a[(img, y + ky - 1, x + kx - 1)], zero outside the map; a [imgs * S * S][K]."""
    m = F.pad(a.view(imgs, S, S, -1), (0, 0, 1, 1, 1, 1))
    return m[:, ky:ky + S, kx:kx + S].reshape(imgs * S * S, -1)


def _nz_min(t):
    t = t.abs()
    return t[t != 0].min().item() if bool((t != 0).any()) else 0.0


def out32(ref, T, term, inv=1.0):
    return NS(kind='f32', ref=ref * inv, T=T * inv, term=term * inv)


def out16(ref, T, term):
    return NS(kind='f16', ref=ref, T=T, term=term)


def with_prior(o, prior):
    """An fp32 output under accumulate = 1."""
    p = prior.double().reshape(o.ref.shape)
    return NS(kind=o.kind, ref=o.ref + p, T=o.T + p.abs(), term=min(o.term, p.abs().min().item()))


def tol(o, g=None):
    g = G if g is None else g
    if o.kind == 'f32':
        return g * U * o.T
    return UH * o.ref.abs() + g * U * o.T + HALF_SUB


def detectable(o):
    """The smallest non-zero term of the output is at least four times its largest tolerance."""
    return o.term >= 4 * float(tol(o).max())


def ratio(got, ref, T):
    """The largest |err| / (u T); an element without a term must be exactly 0."""
    err = (got.double() - ref).abs()
    assert bool((err[T == 0] == 0).all())
    live = T > 0
    return (err[live] / (U * T[live])).max().item() if bool(live.any()) else 0.0


def wgrad1(dY, a, s=1.0):
    dY, a = dY.double(), a.double()
    return out32(dY.t() @ a, dY.abs().t() @ a.abs(), _nz_min(dY) * _nz_min(a), 1 / s)


def wgrad3(dY, A, imgs, S, s=1.0):
    dY, A = dY.double(), A.double()
    ref = torch.empty(32, A.shape[1], 3, 3, dtype=torch.float64)
    T = torch.empty_like(ref)
    for ky in range(3):
        for kx in range(3):
            b = shifted(A, imgs, S, ky, kx)
            ref[:, :, ky, kx], T[:, :, ky, kx] = dY.t() @ b, dY.abs().t() @ b
    return out32(ref, T, _nz_min(dY) * _nz_min(A), 1 / s)


def conv2_input_grad(dY, W2, imgs, S):
    """sum_(tap, n) dY[p - (dy, dx)][n] W2[n][m][tap] as [M][128]: the adjoint of a pad-1 cross-correlation."""
    dy = dY.double().view(imgs, S, S, 32).permute(0, 3, 1, 2)
    return F.conv_transpose2d(dy, W2.double(), padding=1).permute(0, 2, 3, 1).reshape(imgs * S * S, -1)


def dgrad3(dY, W2, A, imgs, S, scale2, gamma2, beta2, s=1.0):
    """dict(dB, dgamma, dbeta) of gnx_conv3x3_dgrad_bnrelu_bwd_f16."""
    A, scale2, gamma2, beta2 = A.double(), scale2.double(), gamma2.double(), beta2.double()
    mask = (A > 0).double()
    d = conv2_input_grad(dY, W2, imgs, S) * mask
    Td = conv2_input_grad(dY.abs(), W2.abs(), imgs, S) * mask
    term = _nz_min(dY) * _nz_min(W2)
    S0, T0, S1, T1 = d.sum(0), Td.sum(0), (d * A).sum(0), (Td * A).sum(0)
    live = A[A > 0]
    a_off = (live.min().item() - beta2.abs().max().item()) if live.numel() else 0.0      # |A - beta| of a live element, at least
    return dict(dB=out16(d * scale2, Td * scale2.abs(), term * scale2.abs().min().item()),
                dbeta=out32(S0, T0, term, 1 / s),
                dgamma=out32((S1 - beta2 * S0) / gamma2, (T1 + beta2.abs() * T0) / gamma2.abs(),
                             term * a_off / gamma2.abs().max().item(), 1 / s))


def dgrad1(dB, W1, X, G0, bn, s=1.0, wgrad=True):
    """dict(G, dgamma, dbeta[, dW]) of gnx_conv1x1_dgrad[_wgrad]_bnrelu_bwd_f16; W1 [128][K]."""
    dB, W1, X, G0 = dB.double(), W1.double(), X.double(), G0.double()
    a, z = act16(X, bn.scale, bn.shift)
    mask = (z > 0).double()
    d, Td = (dB @ W1) * mask, (dB.abs() @ W1.abs()) * mask
    term = _nz_min(dB) * _nz_min(W1)
    xm = X - bn.mean.double()
    sc, inv = bn.scale.double(), bn.invstd.double()
    o = dict(G=out16(d * sc + G0, Td * sc.abs() + G0.abs(), min(term * sc.abs().min().item(), G0.abs().min().item())),
             dbeta=out32(d.sum(0), Td.sum(0), term, 1 / s),
             dgamma=out32((d * xm).sum(0) * inv, (Td * xm.abs()).sum(0) * inv, term * xm.abs().min().item() * inv.min().item(), 1 / s))
    if wgrad:
        o['dW'] = wgrad1(dB, a, s)
    return o


def tail(dfeats, X, S2, bn, s=1.0):
    dfeats, X = dfeats.double(), X.double()
    _, z = act16(X, bn.scale, bn.shift)
    v = (dfeats / S2).repeat_interleave(S2, 0) * (z > 0)
    xm = X - bn.mean.double()
    sc, inv = bn.scale.double(), bn.invstd.double()
    term = dfeats.abs().min().item() / S2
    return dict(G=out16(v * sc * s, (v * sc * s).abs(), term * sc.abs().min().item() * s),
                dbeta=out32(v.sum(0), v.abs().sum(0), term),
                dgamma=out32((v * xm).sum(0) * inv, (v * xm).abs().sum(0) * inv, term * xm.abs().min().item() * inv.min().item()))


def trans(dP, X, imgs, S, bn, s=1.0):
    dP, X = dP.double(), X.double()
    So, C = S // 2, X.shape[1]
    _, z = act16(X, bn.scale, bn.shift)
    up = dP.view(imgs, So, So, C).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(imgs * S * S, C) * 0.25
    v = up * (z > 0)
    xm = X - bn.mean.double()
    sc, inv = bn.scale.double(), bn.invstd.double()
    term = dP.abs().min().item() * 0.25
    return dict(G=out16(v * sc, (v * sc).abs(), term * sc.abs().min().item()),
                dbeta=out32(v.sum(0), v.abs().sum(0), term, 1 / s),
                dgamma=out32((v * xm).sum(0) * inv, (v * xm).abs().sum(0) * inv, term * xm.abs().min().item() * inv.min().item(), 1 / s))


def h16(X, W, pro=None, con=None):
    """gnx_conv1x1_bnrelu_h16: W [N][K]; pro = (scale, shift) of the prologue or None; con = (out_scale, out_shift) or None."""
    X, W = X.double(), W.double()
    a = act16(X, *pro)[0] if pro else X
    y, T = a @ W.t(), a.abs() @ W.abs().t()
    term = _nz_min(a) * _nz_min(W)
    if con is None:
        return out16(y, T, term)
    osc, osh = con[0].double(), con[1].double()
    return out16(torch.relu(y * osc + osh), T * osc.abs() + osh.abs(), term * osc.abs().min().item())


# ------------------------------------------------------------------------------------------------------------ the grid
Wg1 = namedtuple('Wg1', 'edge M N K')
Wg3 = namedtuple('Wg3', 'edge imgs S')
Dg3 = namedtuple('Dg3', 'edge imgs S want')                  # want: which of dgamma ('g') and dbeta ('b') are asked for
C3 = namedtuple('C3', 'edge imgs S lay')
Dg1 = namedtuple('Dg1', 'edge M K lay want')
Tail = namedtuple('Tail', 'edge imgs C S2 lay')
Trans = namedtuple('Trans', 'edge imgs C S lay')
Cols = namedtuple('Cols', 'edge M C')
H16 = namedtuple('H16', 'edge M N K cb')

WG1_GRID = ([Wg1('ragged', M, 8, 8) for M in (1, 63, 64, 65)] + [
    Wg1('two-blocks-each-way', 65, 136, 136), Wg1('padding-workgroups', 513, 8, 136), Wg1('per2-short-last', 64 * 770 + 5, 8, 8),
    Wg1('three-blocks-per2', 64 * 257 + 1, 8, 264), Wg1('32-blocks', 1600, 512, 1024)])
WG3_GRID = ([Wg3('padded', n, S) for n, S in ((4, 4), (1, 8), (1, 16), (1, 32), (1, 64))]
            + [Wg3('generic-pow2-ragged', n, 4) for n in (1, 3, 5)]
            + [Wg3('generic', n, S) for n, S in ((70, 1), (17, 2), (8, 3), (2, 6), (2, 7), (1, 63))]
            + [Wg3('per2-padded', 2052, 4), Wg3('per2-generic', 2053, 4)])
DG3_GRID = ([Dg3('padded', n, S, 'gb') for n, S in ((8, 4), (2, 8), (1, 16), (1, 32), (1, 64))]
            + [Dg3('generic-pow2-ragged', n, 8, 'gb') for n in (1, 3)]
            + [Dg3('generic', n, S, 'gb') for n, S in ((130, 1), (33, 2), (15, 3), (3, 7), (1, 63))]
            + [Dg3('per2', 4104, 4, 'gb'), Dg3('dgamma-only', 8, 4, 'g'), Dg3('dbeta-only', 3, 8, 'b'), Dg3('neither', 8, 4, '')])
C3_GRID = ([C3('tiles-%d' % t, 8 * t, 4, 'blocked') for t in (1, 256, 257, 511, 513)]
           + [C3('map', n, S, lay) for n, S, lay in ((2, 8, 'rows'), (1, 16, 'blocked'), (1, 32, 'rows'), (1, 64, 'blocked'))])
DG1_GRID = ([Dg1('blocks', 130, K, 'blocked', 'gb') for K in (32, 96, 128, 160, 288, 992)]
            + [Dg1('ragged', M, 96, 'rows', 'gb') for M in (1, 63, 64, 65)]
            + [Dg1('per1-per2', 64 * 600 + 7, 32, 'blocked', 'gb'), Dg1('slabs-not-8', 64 * 9 + 1, 160, 'rows', 'gb'),
               Dg1('slabs-not-8', 64 * 11 + 3, 288, 'blocked', ''), Dg1('no-bn-sums', 65, 32, 'rows', '')])
TAIL_GRID = ([Tail('rows-C8', 5, 8, 4, 'rows')] + [Tail('blocked-16', n, 32, 4, 'blocked') for n in (1, 15, 16, 17)]
             + [Tail('strided', n, 1024, S2, 'blocked') for n in (1025, 2051) for S2 in (1, 4)]
             + [Tail('strided', 1025, 1024, 1, 'rows'), Tail('map', 3, 32, 16, 'rows'), Tail('map', 2, 32, 49, 'blocked')])
TRANS_GRID = ([Trans('map', 3, 32, S, lay) for S in (2, 4, 6, 14) for lay in ('rows', 'blocked')]
              + [Trans('rows-C8', 5, 8, 4, 'rows'), Trans('strided', 4097, 1024, 2, 'blocked'), Trans('blocked-16', 17, 32, 2, 'blocked')])
COLS_GRID = [Cols('grid-stride', 16400, 512), Cols('C8', 77, 8), Cols('small', 130, 64)]
H16_GRID = ([H16('m128-last', 131071, 8, 40, 0), H16('m256-first', 131072, 136, 8, 0), H16('m256-ragged', 131072 + 129, 32, 72, 0),
             H16('m256-first', 131072, 32, 40, 1), H16('m256-ragged', 131072 + 129, 64, 64, 1)]
            + [H16('small', M, N, K, cb) for M, N, K, cb in ((1, 8, 8, 0), (129, 136, 40, 0), (257, 32, 72, 0), (130, 32, 64, 1),
                                                             (127, 64, 8, 1), (128, 8, 64, 0))])
GRID = dict(wgrad1=WG1_GRID, wgrad3=WG3_GRID, dgrad3=DG3_GRID, conv3=C3_GRID, dgrad1=DG1_GRID, tail=TAIL_GRID, trans=TRANS_GRID,
            cols=COLS_GRID, h16=H16_GRID)
# the edges of DESIGN.md's "fp16 backward forms" that GRID must hold, by family
EDGES = dict(wgrad1={'ragged', 'two-blocks-each-way', 'padding-workgroups', 'per2-short-last', 'three-blocks-per2', '32-blocks'},
             wgrad3={'padded', 'generic-pow2-ragged', 'generic', 'per2-padded', 'per2-generic'},
             dgrad3={'padded', 'generic-pow2-ragged', 'generic', 'per2', 'dgamma-only', 'dbeta-only', 'neither'},
             conv3={'tiles-1', 'tiles-256', 'tiles-257', 'tiles-511', 'tiles-513', 'map'},
             dgrad1={'blocks', 'ragged', 'per1-per2', 'slabs-not-8', 'no-bn-sums'},
             tail={'rows-C8', 'blocked-16', 'strided', 'map'}, trans={'map', 'rows-C8', 'strided', 'blocked-16'},
             cols={'grid-stride', 'C8', 'small'}, h16={'m128-last', 'm256-first', 'm256-ragged', 'small'})


def ids(c):
    return '-'.join(str(v) for v in c)


# ---------------------------------------------------------------------------------------------- operands of the cases
@functools.lru_cache(maxsize=2)
def recipe_wgrad1(c):
    g = _seed(1, c.M, c.N, c.K)
    bn = _bn(g, c.K, tight=c.M >= NARROW_FROM)
    hi = _hi(c.M)
    return NS(dY=_signed(g, 0.5, hi, c.M, c.N), X=_signed(g, 0.5, hi, c.M, c.K), bn=bn, dW0=_signed(g, 0.5, 1.5, c.N, c.K))


@functools.lru_cache(maxsize=2)
def recipe_conv2(imgs, S, dense=False):
    """The operands of the three conv2 entry points on imgs maps of S x S: dY [M][32], A [M][128] (the stored activation: 0 or in
    [0.5, hi]), W2 [32][128][3][3], scale2 / gamma2 (random signs) / beta2, and priors of every fp32 output.  dense: half of A
    is live whatever M (the form in which dB and dW2 are compared where the BatchNorm sums need the thinned mask)."""
    g = _seed(2, imgs, S)
    M = imgs * S * S
    hi = 0.625
    A = _signed(g, 0.5, hi, M, 128).abs() * _live(g, M, 128, 0.5 if dense else density_for(M, 288)).double()
    return NS(dY=_signed(g, 0.5, hi, M, 32), A=A, W2=_signed(g, 0.5, 0.75, 32, 128, 3, 3), scale2=_chan(g, 0.75, 1.25, 128),
              gamma2=_chan(g, 0.75, 1.25, 128), beta2=_chan(g, 1 / 32, 1 / 16, 128), dW0=_signed(g, 0.5, 1.5, 32, 128, 3, 3),
              dg0=_signed(g, 0.5, 1.5, 128), db0=_signed(g, 0.5, 1.5, 128), M=M)


@functools.lru_cache(maxsize=2)
def recipe_dgrad1(M, K, dense=False):
    """dense: as in recipe_conv2 (G and dW1 compared on a half-live mask)."""
    g = _seed(3, M, K)
    bn = _bn(g, K, tight=True)
    hi = 0.625
    return NS(dB=_signed(g, 0.5, hi, M, 128), W1=_signed(g, 0.5, 0.75, 128, K),
              X=_masked_x(g, M, K, bn.scale, 0.5 if dense else density_for(M, 128), hi),
              G0=_signed(g, 0.5, 1.5, M, K), bn=bn, dW0=_signed(g, 0.5, 1.5, 128, K), dg0=_signed(g, 0.5, 1.5, K),
              db0=_signed(g, 0.5, 1.5, K))


@functools.lru_cache(maxsize=2)
def recipe_tail(imgs, C, S2):
    g = _seed(4, imgs, C, S2)
    bn = _bn(g, C, tight=True)
    M = imgs * S2
    return NS(dfeats=_signed(g, 0.5, _hi(M), imgs, C), X=_masked_x(g, M, C, bn.scale, 0.5, _hi(M)), bn=bn,
              dg0=_signed(g, 0.5, 1.5, C), db0=_signed(g, 0.5, 1.5, C), M=M)


@functools.lru_cache(maxsize=2)
def recipe_trans(imgs, C, S):
    g = _seed(5, imgs, C, S)
    bn = _bn(g, C, tight=True)
    M = imgs * S * S
    return NS(dP=_signed(g, 0.5, _hi(M), imgs * (S // 2) ** 2, C), X=_masked_x(g, M, C, bn.scale, 0.5, _hi(M)), bn=bn,
              dg0=_signed(g, 0.5, 1.5, C), db0=_signed(g, 0.5, 1.5, C), M=M)


@functools.lru_cache(maxsize=2)
def recipe_h16(M, N, K):
    g = _seed(6, M, N, K)
    pro, con = _bn(g, K, tight=False), _bn(g, N, tight=False)
    return NS(X=_signed(g, 0.5, 1.5, M, K), W=_signed(g, 0.5, 0.75, N, K), pro=(pro.scale, pro.shift), con=(con.scale, con.shift))


def min_fma(X, bn):
    """The smallest |fp32 fma(x, scale, shift)| of a case."""
    return act16(X, bn.scale, bn.shift)[1].abs().min().item()


@functools.lru_cache(maxsize=2)
def reference_wgrad1(c, pro, s=1.0):
    r = recipe_wgrad1(c)
    return dict(dW=wgrad1(r.dY, act16(r.X, r.bn.scale, r.bn.shift)[0] if pro else r.X, s))


@functools.lru_cache(maxsize=2)
def reference_conv2(imgs, S, s=1.0, dense=False):
    """dict(dW, dB, dgamma, dbeta): every output of the three conv2 entry points."""
    r = recipe_conv2(imgs, S, dense)
    o = dgrad3(r.dY, r.W2, r.A, imgs, S, r.scale2, r.gamma2, r.beta2, s)
    o['dW'] = wgrad3(r.dY, r.A, imgs, S, s)
    return o


@functools.lru_cache(maxsize=2)
def reference_dgrad1(M, K, s=1.0, dense=False):
    r = recipe_dgrad1(M, K, dense)
    return dgrad1(r.dB, r.W1, r.X, r.G0, r.bn, s)


@functools.lru_cache(maxsize=2)
def reference_tail(imgs, C, S2, s=1.0):
    r = recipe_tail(imgs, C, S2)
    return tail(r.dfeats, r.X, S2, r.bn, s)


@functools.lru_cache(maxsize=2)
def reference_trans(imgs, C, S, s=1.0):
    r = recipe_trans(imgs, C, S)
    return trans(r.dP, r.X, imgs, S, r.bn, s)


@functools.lru_cache(maxsize=2)
def reference_h16(M, N, K, act):
    r = recipe_h16(M, N, K)
    return dict(out=h16(r.X, r.W, r.pro if act else None, r.con if act else None))


# ------------------------------------------------------------------------------------------ plans of the cases, by family
def rows_of(family, c):
    if family in ('wgrad3', 'dgrad3', 'conv3'):
        return c.imgs * c.S * c.S
    if family == 'tail':
        return c.imgs * c.S2
    if family == 'trans':
        return c.imgs * c.S * c.S
    return c.M


def plan_of(family, c, wgrad=False):
    """(tiles, slabs, per) of a slab-planned case."""
    M = rows_of(family, c)
    if family == 'wgrad1':
        return plan_wgrad1(M, c.N, c.K)
    if family == 'wgrad3':
        return plan_slabs(M, 64, SLABS_3X3)
    if family == 'dgrad3':
        return plan_slabs(M, 128, SLABS_3X3)
    if family == 'dgrad1':
        return plan_dgrad1(M, c.K, wgrad)
    assert family == 'conv3' and M % 128 == 0
    tiles = M // 128
    per = -(-tiles // conv3_bwd_grid(M))
    return NS(tiles=tiles, slabs=-(-tiles // per), per=per)


# ------------------------------------------------------------------------------------ the plain fp32 evaluations behind G
def sample(n, k):
    """At most k indices spread evenly over range(n), both ends included."""
    return sorted({(i * (n - 1)) // max(k - 1, 1) for i in range(min(n, k))})


def chain_fp32(A, B):
    """A [r][n] @ B [n][c] as a sequential fp32 multiply-add chain over n (product rounded, then added)."""
    A, B = A.float(), B.float()
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for n in range(A.shape[1]):
        acc = acc + A[:, n, None] * B[n, None, :]
    return acc


def conv2_cols(dY, imgs, S):
    """[M][9 * 32]: column tap * 32 + n of row p holds dY[p - (dy, dx)][n]; conv2_weight_matrix is its partner."""
    return torch.cat([shifted(dY.double(), imgs, S, 2 - t // 3, 2 - t % 3) for t in range(9)], 1)


def conv2_weight_matrix(W2):
    return W2.double().permute(2, 3, 0, 1).reshape(9 * 32, -1)


def plain_products(family, c):
    """The contractions of a case as matrix products (name, A [r][n], B [n][c]) of fp32-valued float64 operands, n the
    contraction: what the two plain fp32 evaluations behind G compute."""
    f32 = lambda t: t.float().double()
    ones = lambda M: torch.ones(1, M, dtype=torch.float64)
    out = []
    if family == 'wgrad1':
        r = recipe_wgrad1(c)
        out = [('dW', r.dY.t(), r.X), ('dW act', r.dY.t(), act16(r.X, r.bn.scale, r.bn.shift)[0])]
    elif family in ('wgrad3', 'dgrad3', 'conv3'):
        r = recipe_conv2(c.imgs, c.S)
        if family != 'dgrad3':
            out += [('dW2 tap %d' % t, r.dY.t(), shifted(r.A, c.imgs, c.S, t // 3, t % 3)) for t in range(9)]
        if family != 'wgrad3':
            cols, Wm = conv2_cols(r.dY, c.imgs, c.S), conv2_weight_matrix(r.W2)
            out += [('d2', cols, Wm), ('S0', ones(r.M), f32((cols @ Wm) * (r.A > 0)))]
    elif family == 'dgrad1':
        r = recipe_dgrad1(c.M, c.K)
        a, z = act16(r.X, r.bn.scale, r.bn.shift)
        out = [('d1', r.dB, r.W1), ('S0', ones(c.M), f32((r.dB @ r.W1) * (z > 0))), ('dW1', r.dB.t(), a)]
    elif family == 'tail':
        r = recipe_tail(c.imgs, c.C, c.S2)
        v = (r.dfeats / c.S2).repeat_interleave(c.S2, 0) * (act16(r.X, r.bn.scale, r.bn.shift)[1] > 0)
        out = [('S0', ones(r.M), f32(v))]
    elif family == 'trans':
        r = recipe_trans(c.imgs, c.C, c.S)
        So = c.S // 2
        up = r.dP.view(c.imgs, So, So, c.C).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(r.M, c.C) * 0.25
        out = [('S0', ones(r.M), up * (act16(r.X, r.bn.scale, r.bn.shift)[1] > 0))]
    elif family == 'h16':
        r = recipe_h16(c.M, c.N, c.K)
        out = [('y', r.X, r.W.t()), ('y act', act16(r.X, *r.pro)[0], r.W.t())]
    return out


def plain_ratio(family, c, mm, nrows=None, ncols=None):
    """The largest |err| / (u T) of the fp32 evaluation `mm(A, B)` over the case's contractions, on at most nrows x ncols
    evenly spread outputs each (None: all); (ratio, name of the contraction)."""
    worst = (0.0, '')
    for name, A, B in plain_products(family, c):
        if nrows is not None:
            A = A[sample(A.shape[0], nrows)]
        if ncols is not None:
            B = B[:, sample(B.shape[1], ncols)]
        got = mm(A, B)
        worst = max(worst, (ratio(got.cpu(), A @ B, A.abs() @ B.abs()), name))
    return worst
