"""Float64 references of the fp32 1x1-convolution entry points of csrc/conv1x1.hip and csrc/dgrad_wgrad_f32.hip
(gnx_conv1x1_bnrelu, gnx_conv1x1_bnrelu_ws, gnx_conv1x1_bnrelu_act, gnx_conv1x1_dgrad_bnrelu_bwd,
gnx_conv1x1_dgrad_wgrad_bnrelu_bwd), their dispatch restated in Python, and the grid of shapes the kernel tests run
(test_conv1_ref_host.py proves it on the CPU, test_gpu_conv1_forms.py uses it).  Not imported by the package.

  conv    out = act(A) W^T, act(a) = relu(scale a + shift) evaluated in float64 and not rounded (a = A without the prologue);
          pooled: the row of pooled position (img, oy, ox) is the mean of the four activated source rows (2 oy + {0, 1},
          2 ox + {0, 1}) of an S_in x S_in map, S_in / 2 rounded down (the last row and column of an odd map are not read);
          with the output activation the result is relu(out_scale . + out_shift)
  dgbn    g = (dY Wt^T) [scale X + shift > 0];  dX += scale g;  dbeta (+)= sum_m g;  dgamma (+)= sum_m g (X - mean) invstd
  dgwg    the same with 128 bottleneck channels and K = cin, plus dW[128][K] (+)= dY^T relu(scale X + shift)

Tolerance, per element (u = 2^-24):  |err| <= G u T.  T is the sum of the magnitudes of every term of the element's chain:
  conv    sum_k |a_k| |W_k| with the prologue (|A| |scale| + |shift|) in place of |a| (ReLU-zeroed values included: the bound of
          the activation's own rounding does not know the sign), the pooled mean as a quarter of the four; the output activation
          as |out_scale| T + |out_shift| (the ReLU is 1-Lipschitz: a result near zero needs no special case)
  dgbn    T_g = sum |dY| |Wt|;  dX: |dX0| + |scale| T_g [mask];  dbeta: sum_m T_g [mask] (+ |dbeta0|);  dgamma: sum_m T_g [mask]
          (|X| + |mean|) invstd (+ |dgamma0|)
  dgwg    the same;  dW: sum_m |dY| (|X| |scale| + |shift|) (+ |dW0|)

G = max(8, 4 x the largest ratio |err| / (u T) of plain fp32 evaluations of the *reference operation* against float64 over every
case of GRID), separately for the products (outputs, dX, dW) and the column sums (dbeta, dgamma); the kernels' own error has no
part in it:
                                                                       products            column sums
  fp32 torch on the device (test_gpu_conv1_forms.py: matmul, or         TORCH_FP32_RATIO    TORCH_FP32_SUM_RATIO
  F.conv2d + avg_pool2d for the pooled cases, + fp32 column sums)
  sequential fp32 multiply-add chain on the CPU                        CHAIN_FP32_RATIO    CHAIN_FP32_SUM_RATIO
  measured:  products 4.6721 (device) and 4.3957 (chain): G = 18.688;  column sums 0.3439 and 0.3241: G_SUMS = 8 (the floor)
(where each occurred: the constants below).  The CPU measurement runs in test_conv1_ref_host.py, the device one in
test_gpu_conv1_forms.py; each prints its figures and holds them to G / 4.

Detectability.  Activations, gradients and weights: magnitude in [0.5, 1.5], random sign - every product term is at least 0.25.
Prologue: |scale| in [1.5, 2], |shift| in [0.125, 0.25], random signs (half the scales are negative): |scale a| >= 0.75, so a
pre-activation is at least 0.5 from zero (fp32 rounding cannot flip the ReLU) and an activated value is exactly 0 or at least 0.5;
a pooled term is a quarter of an unpooled one.  Output activation: |out_scale| in [0.5, 1], |out_shift| in [0.125, 0.25], random
signs: a term reaches the result times at least 0.5 wherever the output ReLU is open (about half the elements; where it is shut the
reference is 0 and the result must be within the tolerance of 0).  The adjoints take conv3_ref's ranges: |scale|, invstd in
[0.875, 1.125], |shift|, |mean| in [1/32, 1/16], X in [0.5, 1.5] with random sign: a pre-activation is at least 0.375 from zero,
|X - mean| invstd >= 0.38, an activated value is 0 or at least 0.375.
`detectable` asks the smallest non-zero term of a case to be at least 4 x its largest tolerance: one dropped, doubled or misplaced
term fails.  It holds for every output map and every dX of every case, K = 2048 and K = 2176 included.  For dbeta / dgamma it is
asserted up to SUMS_DETECT_TERMS = rows x contraction length per column, for dW up to DW_DETECT_ROWS rows: a sum over more rows
cannot see one term in fp32 (T grows with the rows).  Above, the sums still detect the loss of one wave's share of one tile - 32
or 64 rows of |g| around K - or of one slab, and each single term is seen through dX.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import torch

from conv3_ref import _signed, ratio, detectable, flagged, U, G_FLOOR, MIN_TERM   # noqa: F401
from gridnext_amd._lib import CONSTANTS

# largest |err| / (u T) over GRID and the case it came from
TORCH_FP32_RATIO = 4.6721           # fp32 torch on the device (test_gpu_conv1_forms.py)
TORCH_FP32_AT = '65664 rows, N 32, K 32, no prologue (4.24 at dgwg, 19232 rows, K 128; 4.20 at dX of dgbn, 32896 rows, N 160, K 32)'
CHAIN_FP32_RATIO = 4.3957           # sequential fp32 multiply-add chain on the CPU (test_conv1_ref_host.py)
CHAIN_FP32_AT = '32896 rows, N 160, K 32, no prologue (3.995 at dW of dgwg, 32992 rows, K 64; 3.92 at dX of dgbn, 32896 rows, N 160, K 32)'
TORCH_FP32_SUM_RATIO = 0.3439       # dbeta / dgamma: the device's fp32 product, mask and fp32 column sums
TORCH_FP32_SUM_AT = 'dgwg, 32 rows, K 288 (0.284 at dgwg, 32 rows, K 224; 0.260 at dgwg, 32 rows, K 32)'
CHAIN_FP32_SUM_RATIO = 0.3241       # ... the CPU chain and a sequential fp32 sum over the rows
CHAIN_FP32_SUM_AT = 'dgwg, 32 rows, K 288 (0.312 at dgbn, 32896 rows, N 160, K 32; 0.297 at dgbn, 384 rows, N 352, K 32)'
G = max(G_FLOOR, 4 * max(TORCH_FP32_RATIO, CHAIN_FP32_RATIO))
G_SUMS = max(G_FLOOR, 4 * max(TORCH_FP32_SUM_RATIO, CHAIN_FP32_SUM_RATIO))

C1_BM, C1_BN, C1_KMAX = 128, 128, 2048             # csrc/conv1x1.hip
LD_LIMIT = 1 << 16
WS_MAX_WGS, DGBN_MAX_WGS = 512, 512
DGBN_R = 128
OK, BAD_ARG, UNSUPPORTED = 0, -1, -3
# include/gridnext_hip.h: GNX_C1_*, in the header's order (generic ... ws_pool)
CODES = {k[len('GNX_C1_'):].lower(): v for k, v in CONSTANTS.items() if k.startswith('GNX_C1_')}
BODIES = tuple(CODES)
DGWG_SHAPES = ('dgwg full', 'dgwg rest1', 'dgwg rest2', 'dgwg idle wave')
SUMS_DETECT_TERMS = 256 * 128
DW_DETECT_ROWS = 8192


# ------------------------------------------------------------------------------------------------------------ the cases
# op: conv | dgbn | dgwg.  conv: M output rows (pooled: n images of S x S give M = n (S / 2)^2), act: BN+ReLU prologue, oact: the
# output activation (gnx_conv1x1_bnrelu_act), ws: 0 = no workspace argument, 1 = gnx_conv1x1_bnrelu_ws with the queried workspace,
# 2 = gnx_conv1x1_bnrelu_ws with a NULL workspace.
# lay: al = every operand 16-B aligned; ash = A one float off; aodd = lda % 4 == 1; ssh = scale and shift one float off; wsh = the
#      weights one float off; codd = ldc % 4 == 1 (where the split form is wanted); wmis = the workspace one float off.
# big: 'lda' / 'ldc' = that leading dimension is 65536.  dgbn: N = cin, K = the bottleneck's channels.  dgwg: K = cin, N = 128.
Case = namedtuple('Case', 'op M N K act pool S oact lay ws big')


def conv(M, N, K, act=1, oact=0, lay='al', ws=0, big=''):
    return Case('conv', M, N, K, act, 0, 0, oact, lay, ws, big)


def pconv(n, S, N, K, act=1, lay='al'):
    return Case('conv', n * (S // 2) ** 2, N, K, act, 1, S, 0, lay, 0, '')


def dgbn(M, N, K=128):
    return Case('dgbn', M, N, K, 1, 0, 0, 0, 'al', 0, '')


def dgwg(M, K):
    return Case('dgwg', M, 128, K, 1, 0, 0, 0, 'al', 0, '')


def images(c):
    return c.M // (c.S // 2) ** 2 if c.pool else 0


def rows_in(c):
    """Rows of A: the source positions of a pooled case."""
    return images(c) * c.S * c.S if c.pool else c.M


def _r4(v):
    return (v + 3) // 4 * 4


def layout(c):
    """How a case lies in memory.  conv: A is the window [pad : pad + rows_in, 4 : 4 + K] of a sentinel-filled [..][lda] tensor
    that starts a_shift floats into 16-B aligned storage; out the window [pad : pad + M, c_off : c_off + N] of a [..][ldc] tensor:
    c_off 1 or 3 floats and ldc odd, except where the split form is wanted (ws == 1: it takes a 16-B aligned output with 4 | ldc
    only; codd makes ldc odd there).  dgbn: dY as A; X and dX windows of their own with different odd leading dimensions at
    column offsets 1 and 3.  dgwg: dB, X and G aligned windows (the entry point takes no others), ldx != ldg."""
    lo = NS(pad=3, a_off=4, a_shift=1 if c.lay == 'ash' else 0, ss_shift=1 if c.lay == 'ssh' else 0,
            w_shift=1 if c.lay == 'wsh' else 0, ws_shift=1 if c.lay == 'wmis' else 0)
    if c.op == 'conv':
        lo.lda = LD_LIMIT if c.big == 'lda' else _r4(c.K) + 8 + (c.lay == 'aodd')
        lo.out_aligned = c.ws == 1
        if c.ws == 1:
            lo.ldc, lo.c_off = _r4(c.N) + 8 + (c.lay == 'codd'), 4
        else:
            lo.ldc, lo.c_off = (c.N + 4) | 1, 1 if c.N % 3 else 3
        if c.big == 'ldc':
            lo.ldc = LD_LIMIT
    elif c.op == 'dgbn':
        lo.lda = _r4(c.K) + 8                                # lddy
        lo.ldx, lo.x_off, lo.ldc, lo.c_off = (c.N + 6) | 1, 1, (c.N + 12) | 1, 3
    else:
        lo.lda = 128 + 8                                     # lddb
        lo.ldx, lo.x_off, lo.ldc, lo.c_off = _r4(c.K) + 8, 4, _r4(c.K) + 12, 8
    return lo


# ------------------------------------------------------------------------------------------------------------ inputs
def _seed(c):
    return 7919 * c.M + 131 * c.S + 1000003 * c.K + 31 * c.N + {'conv': 1, 'dgbn': 2, 'dgwg': 3}[c.op] + 17 * c.pool


@functools.lru_cache(maxsize=3)
def _recipe(op, M, N, K, pool, S):
    c = Case(op, M, N, K, 1, pool, S, 0, 'al', 0, '')
    g = torch.Generator().manual_seed(_seed(c))
    if op == 'conv':
        return NS(X=_signed(g, 0.5, 1.5, rows_in(c), K), W=_signed(g, 0.5, 1.5, N, K), scale=_signed(g, 1.5, 2.0, K),
                  shift=_signed(g, 0.125, 0.25, K), oscale=_signed(g, 0.5, 1.0, N), oshift=_signed(g, 0.125, 0.25, N))
    C, B = (N, K) if op == 'dgbn' else (K, 128)              # channels in (the gradient's columns), bottleneck channels
    r = NS(dY=_signed(g, 0.5, 1.5, M, B), Wt=_signed(g, 0.5, 1.5, C, B), X=_signed(g, 0.5, 1.5, M, C), dX0=_signed(g, 0.5, 1.5, M, C),
           scale=_signed(g, 0.875, 1.125, C), shift=_signed(g, 0.03125, 0.0625, C), mean=_signed(g, 0.03125, 0.0625, C),
           invstd=_signed(g, 0.875, 1.125, C).abs_(), dbeta0=_signed(g, 0.5, 1.5, C), dgamma0=_signed(g, 0.5, 1.5, C))
    if op == 'dgwg':
        r.dW0 = _signed(g, 0.5, 1.5, 128, C)
    return r


def recipe(c):
    """The operands of a case as float32 tensors (layout-independent; shared between tests: do not write to them).
    conv: X [rows_in][K], W [N][K], scale / shift [K], oscale / oshift [N].  dgbn / dgwg: dY [M][B], Wt [C][B] (conv1's weight
    transposed), X / dX0 [M][C], scale / shift / mean / invstd / dbeta0 / dgamma0 [C], dW0 [128][C] (dgwg); C = the channels in
    (N of dgbn, K of dgwg), B = the bottleneck's channels (K of dgbn, 128 of dgwg)."""
    return _recipe(c.op, c.M, c.N, c.K, c.pool, c.S)


# ------------------------------------------------------------------------------------------------------------ references
def pool4(a, n, S):
    """The mean of the four source rows of every pooled position: a [n S S][K] -> [n (S / 2)^2][K], in a's dtype, summed in the
    order ((r0 + r1) + r2) + r3."""
    So = S // 2
    m = a.view(n, S, S, -1)[:, :2 * So, :2 * So].reshape(n, So, 2, So, 2, -1)
    return ((((m[:, :, 0, :, 0] + m[:, :, 0, :, 1]) + m[:, :, 1, :, 0]) + m[:, :, 1, :, 1]) * 0.25).reshape(n * So * So, -1)


def activate(X, scale, shift):
    """(a, |a| bound): relu(scale x + shift) and |x| |scale| + |shift|, float64."""
    X, scale, shift = X.double(), scale.double(), shift.double()
    return torch.relu(X * scale + shift), X.abs() * scale.abs() + shift.abs()


def naive_conv(X, W, scale, shift, pool, S, oscale, oshift):
    """gnx_conv1x1_bnrelu by loops over (row, column) in float64: what `reference` is proven against."""
    X, W = X.double(), W.double()
    act = (lambda v: torch.relu(v * scale.double() + shift.double())) if scale is not None else (lambda v: v)
    if pool:
        So, n = S // 2, X.shape[0] // (S * S)
        rows = []
        for img in range(n):
            for oy in range(So):
                for ox in range(So):
                    src = [(img * S + 2 * oy + dy) * S + 2 * ox + dx for dy in (0, 1) for dx in (0, 1)]
                    rows.append(sum(act(X[s]) for s in src) / 4)
    else:
        rows = [act(X[m]) for m in range(X.shape[0])]
    out = torch.zeros(len(rows), W.shape[0], dtype=torch.float64)
    for m, a in enumerate(rows):
        for n_ in range(W.shape[0]):
            out[m, n_] = (a * W[n_]).sum()
            if oscale is not None:
                out[m, n_] = max(out[m, n_] * oscale[n_].double() + oshift[n_].double(), 0.0)
    return out


@functools.lru_cache(maxsize=3)
def _reference(M, N, K, act, pool, S, oact):
    c = Case('conv', M, N, K, act, pool, S, oact, 'al', 0, '')
    r = recipe(c)
    if act:
        a, amag = activate(r.X, r.scale, r.shift)
        nz = a[a != 0]
        a_min = nz.min().item() if nz.numel() else 0.5
    else:
        a = r.X.double()
        amag, a_min = a.abs(), 0.5
    if pool:
        a, amag, a_min = pool4(a, images(c), S), pool4(amag, images(c), S), a_min / 4
    W = r.W.double()
    ref, T, term = a @ W.t(), amag @ W.abs().t(), a_min * 0.5
    if oact:
        osc, osh = r.oscale.double(), r.oshift.double()
        ref, T, term = torch.relu(ref * osc + osh), T * osc.abs() + osh.abs(), term * osc.abs().min().item()
    return NS(ref=ref, T=T, term=term)


def reference(c):
    """NS(ref, T, term) of a conv case, float64 [M][N]; term: the smallest non-zero term.  Shared: do not write to it."""
    return _reference(c.M, c.N, c.K, c.act, c.pool, c.S, c.oact)


@functools.lru_cache(maxsize=2)
def _adjoint(op, M, N, K):
    c = Case(op, M, N, K, 1, 0, 0, 0, 'al', 0, '')
    r = recipe(c)
    dY, Wt, X = r.dY.double(), r.Wt.double(), r.X.double()
    sc, sh, mu, inv = (t.double() for t in (r.scale, r.shift, r.mean, r.invstd))
    mask = (X * sc + sh > 0).double()
    g, Tg = (dY @ Wt.t()) * mask, (dY.abs() @ Wt.abs().t()) * mask
    xhat, xmag = (X - mu) * inv, (X.abs() + mu.abs()) * inv
    o = NS(mask=mask, g=g, Tg=Tg, dX=r.dX0.double() + sc * g, T_dX=r.dX0.double().abs() + sc.abs() * Tg,
           term=MIN_TERM * sc.abs().min().item(), dbeta=g.sum(0), T_dbeta=Tg.sum(0), dgamma=(g * xhat).sum(0),
           T_dgamma=(Tg * xmag).sum(0), sum_term=MIN_TERM * min(1.0, xhat.abs()[mask > 0].min().item()))
    if op == 'dgwg':
        a, amag = activate(r.X, r.scale, r.shift)
        o.dW, o.T_dW = dY.t() @ a, dY.abs().t() @ amag
        o.dw_term = 0.5 * a[a != 0].min().item()
    return o


def adjoint(c, accumulate=0):
    """The fused gradients of a dgbn / dgwg case, float64: NS(dX, T_dX, term, dbeta, T_dbeta, dgamma, T_dgamma, sum_term and, for
    dgwg, dW, T_dW, dw_term); accumulate: dbeta0 / dgamma0 / dW0 are added (dX always accumulates onto dX0)."""
    s, r = _adjoint(c.op, c.M, c.N, c.K), recipe(c)
    o = NS(**vars(s))
    if accumulate:
        o.dbeta, o.T_dbeta = s.dbeta + r.dbeta0.double(), s.T_dbeta + r.dbeta0.double().abs()
        o.dgamma, o.T_dgamma = s.dgamma + r.dgamma0.double(), s.T_dgamma + r.dgamma0.double().abs()
        if c.op == 'dgwg':
            o.dW, o.T_dW = s.dW + r.dW0.double(), s.T_dW + r.dW0.double().abs()
    return o


def sums_detectable_case(c):
    """Whether one term of dbeta / dgamma is asserted detectable at this case (rows x contraction length per column)."""
    return c.M * (c.K if c.op == 'dgbn' else 128) <= SUMS_DETECT_TERMS


def tol(T, g=None):
    return (G if g is None else g) * U * T


# ---- plain fp32 evaluations of the reference operation on the CPU (what G is measured from)
def act_fp32(c):
    """The A operand of a conv case in fp32: one multiply-add and a max, the pooled mean as ((a0 + a1) + a2) + a3 times 1/4."""
    r = recipe(c)
    a = torch.relu(torch.addcmul(r.shift, r.X, r.scale)) if c.act else r.X
    return pool4(a, images(c), c.S) if c.pool else a


def chain_fp32(a, W):
    """a W^T as a sequential fp32 multiply-add chain over k (one rounding for the product, one for the sum)."""
    a, W = a.float(), W.float()
    acc = torch.zeros(a.shape[0], W.shape[0], dtype=torch.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * W[:, k]
    return acc


def chain_fp32_t(dY, a):
    """dY^T a as a sequential fp32 multiply-add chain over the rows."""
    acc = torch.zeros(dY.shape[1], a.shape[1], dtype=torch.float32)
    for m in range(dY.shape[0]):
        acc = acc + dY[m, :, None] * a[m]
    return acc


def seq_sum(v):
    acc = torch.zeros(v.shape[1], dtype=torch.float32)
    for m in range(v.shape[0]):
        acc = acc + v[m]
    return acc


# ------------------------------------------------------------------------------------------------------------ dispatch
def _cdiv(a, b):
    return -(-a // b)


def small_splits(M, N, K):
    """conv1x1_small_splits: the planned K splits of the small-M form, 0 = not its shape."""
    if M > 8192 or K < 256 or K % 32 or N % 4:
        return 0
    tiles = _cdiv(M, C1_BM) * _cdiv(N, C1_BN)
    s = K // 128
    while s > 1 and tiles * s > 256:
        s -= 1
    if tiles * s < 32 and K // 64 <= 16:
        s = K // 64
    s = min(s, 16)
    return 0 if s < 2 else s


def conv_form(M, N, K, lda, ldc, act=1, pool=0, S=0, oact=0, mis=(), null=(), ws=0):
    """What one call of conv1x1_launch runs.  mis / null: the operands that are one float off 16 B / NULL, of A, W, out, scale
    (= scale and shift), oscale (= both), ws; ws: a workspace is passed.  NS(err, body, code, wgs, gy, nz, splits, ksplit and, for
    the persistent bodies, tilesN, T, full, partial, jmap)."""
    f = NS(err=OK, body='generic', code=0, wgs=0, gy=0, nz=0, splits=0, ksplit=0, tilesN=0, T=0, full=0, partial=0, jmap=False)
    has = lambda name, on=True: bool(on) and name not in null                      # noqa: E731
    scale, shift = has('scale', act), has('shift', act)
    oscale, oshift = has('oscale', oact), has('oshift', oact)
    if (not has('A') or not has('W') or not has('out') or M < 0 or N <= 0 or K <= 0 or lda < K or ldc < N or scale != shift
            or oscale != oshift or (pool and S < 2)):
        f.err, f.body = BAD_ARG, None
        return f
    if M == 0:
        return f
    al = lambda name: name not in mis                                              # noqa: E731
    vec_a = al('A') and lda % 4 == 0 and K % 4 == 0 and (not scale or al('scale'))
    vec_w = al('W') and K % 4 == 0
    fast = vec_a and vec_w
    f.wgs, f.gy = _cdiv(M, C1_BM), _cdiv(N, C1_BN)
    if has('ws', ws) and fast and not pool and al('out') and ldc % 4 == 0 and al('ws') and (not oscale or al('oscale')):
        f.splits = small_splits(M, N, K)
    if f.splits > 1:
        f.body = 'split'
        f.ksplit = _cdiv(K // 32, f.splits) * 32
        f.nz = _cdiv(K, f.ksplit)
    elif (fast and M % 128 == 0 and N % 32 == 0 and K % 32 == 0 and K <= C1_KMAX and (not pool or (S % 2 == 0 and scale))
          and 4 * M < (1 << 31) and lda < LD_LIMIT and ldc < LD_LIMIT):
        f.splits = 0
        f.body = 'ws_pool' if pool else 'ws_act' if scale else 'ws'
        f.tilesN = _cdiv(N, 128)
        f.T = (M // 128) * f.tilesN
        f.wgs, f.gy = min(f.T, WS_MAX_WGS), 1
        f.full, f.partial = f.T // f.wgs, f.T % f.wgs
        f.jmap = f.tilesN > 1 and f.wgs % (8 * f.tilesN) == 0
    else:
        f.splits = 0
        f.body = ('pool' if pool else 'generic') + ('_vec' if fast else '')
    f.code = CODES[f.body]
    return f


def ws_tile(f, bx, rnd):
    """The tile workgroup bx of a persistent conv form takes in round rnd (None: none): the XCD-grouped map in the full rounds,
    the plain one in a partial last round."""
    base = rnd * f.wgs
    if base + f.wgs <= f.T:
        t = f.tilesN * ((bx & 7) + 8 * (bx // (8 * f.tilesN))) + (bx >> 3) % f.tilesN if f.jmap else bx
    else:
        t = bx
    return base + t if base + t < f.T else None


def dgbn_form(M, N, K, lddy, ldx, lddx, mis=(), null=()):
    """gnx_conv1x1_dgrad_bnrelu_bwd: NS(err, body, wgs, tilesN, T, runs = (shortest, longest) tile list of a workgroup)."""
    f = NS(err=OK, body='dgbn', wgs=0, tilesN=0, T=0, runs=(0, 0))
    if null or M < 0 or N <= 0 or K <= 0 or lddy < K or ldx < N or lddx < N:
        f.err, f.body = BAD_ARG, None
    elif (M % 128 or N % 32 or K % 32 or K > C1_KMAX or 'dY' in mis or 'Wt' in mis or lddy % 4 or 4 * M >= (1 << 31)
          or lddy >= LD_LIMIT or ldx >= LD_LIMIT or lddx >= LD_LIMIT):
        f.err, f.body = UNSUPPORTED, None
    elif M > 0:
        f.tilesN = _cdiv(N, 128)
        f.T = (M // 128) * f.tilesN
        f.wgs = min(f.T, DGBN_MAX_WGS)
        if f.tilesN > 1:                                     # contiguous runs of the column-fastest tile list
            n = [(b + 1) * f.T // f.wgs - b * f.T // f.wgs for b in range(f.wgs)]
        else:                                                # round-robin
            n = [(f.T - b + f.wgs - 1) // f.wgs for b in range(f.wgs)]
        f.runs = (min(n), max(n))
    return f


def dgbn_workspace(M, N):
    return (2 * (M // 128) * 2 + DGBN_R * 2) * N


def _plan32(M, want):
    tiles = M // 32
    slabs = max(1, min(max(want, 1), tiles))
    per = _cdiv(tiles, slabs)
    return _cdiv(tiles, per), per


def dgwg_plan(M, K):
    """The slab plan of gnx_conv1x1_dgrad_wgrad_bnrelu_bwd: full 128-channel blocks (a three-column rest runs as one more full
    block with an idle wave), the rest columns (0, 1 or 2), (slabs, tiles per slab) of either launch, the workspace floats."""
    q = (K % 128) // 32
    p = NS(full=K // 128 + (q == 3), rest=0 if q == 3 else q, idle=q == 3, slabs_full=0, per_full=0, slabs_rest=0, per_rest=0, floats=0)
    if M < 32 or K < 32:                                     # (the workspace query: 0)
        return p
    if p.full:
        p.slabs_full, p.per_full = _plan32(M, _cdiv(512, p.full))
    if p.rest:
        p.slabs_rest, p.per_rest = _plan32(M, 2048 // p.rest)
    p.floats = (p.slabs_full + p.slabs_rest) * (2 + 128) * _cdiv(K, 128) * 128
    return p


def dgwg_form(M, K, lddb, ldx, ldg, mis=(), null=()):
    """NS(err, shapes): the launch shapes one call runs, of DGWG_SHAPES."""
    f = NS(err=OK, shapes=set())
    if null or M <= 0 or K <= 0 or lddb < 128 or ldx < K or ldg < K:
        f.err = BAD_ARG
    elif K % 32 or M % 32 or lddb % 4 or ldx % 4 or ldg % 4 or ldg >= (1 << 20) or mis:
        f.err = UNSUPPORTED
    else:
        p = dgwg_plan(M, K)
        if K // 128:
            f.shapes.add('dgwg full')
        if p.idle:
            f.shapes.add('dgwg idle wave')
        if p.rest:
            f.shapes.add('dgwg rest%d' % p.rest)
    return f


def form_of(c):
    lo = layout(c)
    if c.op == 'conv':
        mis = {'ash': ('A',), 'ssh': ('scale',), 'wsh': ('W',), 'wmis': ('ws',)}.get(c.lay, ())
        if not lo.out_aligned:
            mis = mis + ('out',)                             # (only the split form asks)
        return conv_form(c.M, c.N, c.K, lo.lda, lo.ldc, c.act, c.pool, c.S, c.oact, mis, (), c.ws == 1)
    if c.op == 'dgbn':
        return dgbn_form(c.M, c.N, c.K, lo.lda, lo.ldx, lo.ldc)
    return dgwg_form(c.M, c.K, lo.lda, lo.ldx, lo.ldc)


def bodies_of(c):
    f = form_of(c)
    return f.shapes if c.op == 'dgwg' else {f.body}


# ------------------------------------------------------------------------------------------------------------ the grid
ROUNDS_M = 128 * 513                                        # one tile more than the persistent grid at one column tile
ROUNDS2_M = 128 * 257                                       # two column tiles: 514 tiles on 512 workgroups


def _conv_grid():
    g = []
    # generic: each of A, W, scale / shift one float off and lda % 4 != 0 (the base runs ws_act / ws), K % 4 != 0, the smallest and
    # the ragged extents, with and without the prologue, the output activation, pooled with S_in = 7 and 2
    g += [conv(128, 32, 32, act) for act in (0, 1)]
    g += [conv(128, 32, 32, act, lay=lay) for lay in ('ash', 'wsh', 'ssh', 'aodd') for act in (0, 1)]
    g += [conv(130, 34, K, act) for K in (3, 22, 37) for act in (0, 1)]
    g += [conv(1, 1, 1, act) for act in (0, 1)] + [conv(127, 127, 31), conv(129, 129, 33), conv(129, 129, 33, 0)]
    g += [conv(129, 130, 22, 1, oact=1), conv(5, 3, 2, 0, oact=1)]
    g += [pconv(3, 7, 5, 10), pconv(3, 7, 5, 10, 0), pconv(5, 2, 12, 22), pconv(2, 6, 130, 33, 1), pconv(32, 4, 32, 32, lay='ash')]
    # generic_vec: ragged M, N or K % 32; interior and edge tiles in one launch; K past C1_KMAX; a leading dimension of 65536
    g += [conv(300, 130, 36), conv(300, 130, 36, 0), conv(300, 200, 64), conv(300, 200, 64, 0, oact=1), conv(129, 128, 96, 0)]
    g += [conv(128, 32, 2080), conv(128, 32, 32, big='lda'), conv(128, 32, 32, 0, big='ldc'), conv(256, 128, 64, 1, oact=1, big='ldc')]
    # pool_vec: no prologue (the persistent kernel declines), odd S_in at whole tiles, ragged everything
    g += [pconv(32, 4, 32, 32, 0), pconv(128, 7, 32, 32), pconv(3, 8, 20, 24), pconv(9, 6, 130, 36, 0), pconv(64, 5, 160, 64)]
    # split (gnx_conv1x1_bnrelu_ws with the queried workspace): both sides of M = 8192, K = 256 and 4 | N; the K / 64 branch and its
    # 16 | 17 edge; the 256-workgroup cap (33 row tiles at K = 1024: 7 splits, the last shorter); the cap of 16 at K = 2176; nz < splits
    # (K = 416: 6 planned, 5 launched); a ragged M; no prologue; what falls through: workspace off 16 B, ldc % 4 != 0, NULL
    g += [conv(8192, 32, 256, ws=1), conv(8320, 32, 256, ws=1), conv(256, 128, 224, ws=1), conv(256, 128, 256, ws=1)]
    g += [conv(256, 132, 256, ws=1), conv(256, 130, 256, ws=1), conv(128, 128, 1024, ws=1), conv(128, 128, 1088, ws=1)]
    g += [conv(4224, 128, 1024, ws=1), conv(128, 128, 2176, ws=1), conv(128, 128, 416, ws=1), conv(300, 128, 512, ws=1)]
    g += [conv(128, 128, 416, 0, ws=1), conv(128, 128, 416, lay='wmis', ws=1), conv(128, 128, 416, lay='codd', ws=1)]
    g += [conv(256, 132, 256, lay='codd', ws=1), conv(128, 128, 416, ws=2), conv(128, 128, 2176, ws=2)]
    # ws / ws_act: one tile; odd and even chunk counts; K = 2048; a ragged last column tile of 32, 64 and 96 columns; two and three
    # column tiles with the XCD-grouped map (16 or 24 | workgroups) and without; more than 512 tiles at one and at two column tiles
    # (there the XCD map of the full round and the plain map of the partial one meet); the output activation
    g += [conv(128, 128, K, act) for K in (32, 64, 96) for act in (0, 1)] + [conv(128, 128, 2048), conv(256, 32, 2048, 0)]
    g += [conv(256, N, 64, act) for N in (32, 64, 96, 128, 160, 192, 352) for act in (0, 1)]
    g += [conv(1024, N, 32, act) for N in (160, 256, 352) for act in (0, 1)]
    g += [conv(ROUNDS_M, 32, 32), conv(ROUNDS_M, 32, 32, 0), conv(ROUNDS2_M, 160, 32), conv(ROUNDS2_M, 160, 32, 0), conv(128 * 1024, 32, 32)]
    g += [conv(256, 128, 64, 1, oact=1), conv(256, 96, 64, 0, oact=1), conv(1024, 160, 96, 1, oact=1)]
    # ws_pool: S_in = 4 (one tile spans 32 images), 64 (a tile is a fraction of one image); every last tile ends exactly at rows_in;
    # two and three column tiles; K = 2048; more than 512 tiles
    g += [pconv(32, 4, 32, 32), pconv(64, 4, 128, 64), pconv(1, 64, 32, 32), pconv(8, 8, 256, 96), pconv(2, 16, 160, 64)]
    g += [pconv(32, 4, 32, 2048), pconv(256, 4, 352, 32), pconv(8, 16, 96, 64), pconv(32 * 513, 4, 32, 32)]
    return list(dict.fromkeys(g))


def _dgbn_grid():
    g = [dgbn(128, N) for N in (32, 96, 128, 160, 992)] + [dgbn(1024, 160, 64), dgbn(256, 128, 2048), dgbn(384, 352, 32)]
    g += [dgbn(ROUNDS_M, 32, 32), dgbn(ROUNDS2_M, 160, 32)]
    return list(dict.fromkeys(g))


def _dgwg_grid():
    g = [dgwg(96, K) for K in (32, 64, 96, 128, 160, 192, 224, 288)] + [dgwg(32, 32), dgwg(32, 224), dgwg(32, 288)]
    g += [dgwg(32 * 601, 128), dgwg(32 * 1031, 64), dgwg(32 * 40, 352)]
    return list(dict.fromkeys(g))


CONV_GRID, DGBN_GRID, DGWG_GRID = _conv_grid(), _dgbn_grid(), _dgwg_grid()
GRID = CONV_GRID + DGBN_GRID + DGWG_GRID

# (case on one side, case on the other, body, body): the edges between two bodies of conv1x1_launch
EDGES = [
    (conv(128, 32, 32), conv(128, 32, 32, lay='ash'), 'ws_act', 'generic'),
    (conv(128, 32, 32), conv(128, 32, 32, lay='wsh'), 'ws_act', 'generic'),
    (conv(128, 32, 32), conv(128, 32, 32, lay='ssh'), 'ws_act', 'generic'),
    (conv(128, 32, 32), conv(128, 32, 32, lay='aodd'), 'ws_act', 'generic'),
    (conv(128, 32, 32, 0), conv(128, 32, 32, 0, lay='ash'), 'ws', 'generic'),
    (conv(128, 32, 32, 0), conv(128, 32, 32, 0, lay='ssh'), 'ws', 'ws'),                   # no prologue: scale / shift are not passed
    (conv(128, 128, 96, 0), conv(129, 128, 96, 0), 'ws', 'generic_vec'),
    (conv(256, 128, 64), conv(300, 130, 36), 'ws_act', 'generic_vec'),
    (conv(128, 128, 2048), conv(128, 32, 2080), 'ws_act', 'generic_vec'),
    (conv(128, 32, 32), conv(128, 32, 32, big='lda'), 'ws_act', 'generic_vec'),
    (conv(128, 32, 32, 0), conv(128, 32, 32, 0, big='ldc'), 'ws', 'generic_vec'),
    (pconv(32, 4, 32, 32), pconv(32, 4, 32, 32, 0), 'ws_pool', 'pool_vec'),
    (pconv(32, 4, 32, 32), pconv(32, 4, 32, 32, lay='ash'), 'ws_pool', 'pool'),
    (pconv(32, 4, 32, 32), pconv(128, 7, 32, 32), 'ws_pool', 'pool_vec'),
    (conv(8192, 32, 256, ws=1), conv(8320, 32, 256, ws=1), 'split', 'ws_act'),
    (conv(256, 128, 256, ws=1), conv(256, 128, 224, ws=1), 'split', 'ws_act'),
    (conv(256, 132, 256, ws=1), conv(256, 130, 256, ws=1), 'split', 'generic_vec'),
    (conv(128, 128, 416, ws=1), conv(128, 128, 416, lay='wmis', ws=1), 'split', 'ws_act'),
    (conv(128, 128, 416, ws=1), conv(128, 128, 416, lay='codd', ws=1), 'split', 'ws_act'),
    (conv(256, 132, 256, ws=1), conv(256, 132, 256, lay='codd', ws=1), 'split', 'generic_vec'),
    (conv(128, 128, 416, ws=1), conv(128, 128, 416, ws=2), 'split', 'ws_act'),
    (conv(128, 128, 2176, ws=1), conv(128, 128, 2176, ws=2), 'split', 'generic_vec'),
]
# case -> (planned splits, launched nz) that must hold
SPLIT_EDGES = {conv(8192, 32, 256, ws=1): (2, 2), conv(256, 128, 256, ws=1): (4, 4), conv(256, 132, 256, ws=1): (4, 4),
               conv(128, 128, 1024, ws=1): (16, 16), conv(128, 128, 1088, ws=1): (8, 7), conv(4224, 128, 1024, ws=1): (7, 7),
               conv(128, 128, 2176, ws=1): (16, 14), conv(128, 128, 416, ws=1): (6, 5), conv(300, 128, 512, ws=1): (8, 8)}

# the calls every entry point must refuse, as overrides of a base call: (overrides, code).  mis / null: operands one float off 16 B
# / passed as NULL
CONV_REFUSALS = [(dict(lda=31), BAD_ARG), (dict(ldc=31), BAD_ARG), (dict(null=('scale',)), BAD_ARG), (dict(null=('shift',)), BAD_ARG),
                 (dict(null=('A',)), BAD_ARG), (dict(null=('W',)), BAD_ARG), (dict(null=('out',)), BAD_ARG), (dict(K=0), BAD_ARG),
                 (dict(N=0), BAD_ARG), (dict(M=-1), BAD_ARG), (dict(pool=1, S=1), BAD_ARG), (dict(oact=1, null=('oshift',)), BAD_ARG)]
DGBN_REFUSALS = [(dict(M=128 - 64), UNSUPPORTED), (dict(N=48), UNSUPPORTED), (dict(K=2080, lddy=2088), UNSUPPORTED),
                 (dict(K=48), UNSUPPORTED), (dict(mis=('dY',)), UNSUPPORTED), (dict(mis=('Wt',)), UNSUPPORTED), (dict(lddy=137), UNSUPPORTED),
                 (dict(lddy=LD_LIMIT), UNSUPPORTED), (dict(ldx=LD_LIMIT), UNSUPPORTED), (dict(lddx=LD_LIMIT), UNSUPPORTED),
                 (dict(M=1 << 29), UNSUPPORTED), (dict(lddy=127), BAD_ARG), (dict(ldx=31), BAD_ARG), (dict(lddx=31), BAD_ARG),
                 (dict(M=-128), BAD_ARG), (dict(N=0), BAD_ARG), (dict(K=0), BAD_ARG)]
DGBN_NULLS = ('dY', 'Wt', 'X', 'dX', 'scale', 'shift', 'mean', 'invstd', 'ws')
DGWG_REFUSALS = [(dict(K=48, ldx=56, ldg=56), UNSUPPORTED), (dict(M=96 - 8), UNSUPPORTED), (dict(lddb=137), UNSUPPORTED),
                 (dict(ldx=73), UNSUPPORTED), (dict(ldg=77), UNSUPPORTED), (dict(ldg=1 << 20), UNSUPPORTED), (dict(mis=('dB',)), UNSUPPORTED),
                 (dict(mis=('W1t',)), UNSUPPORTED), (dict(mis=('X',)), UNSUPPORTED), (dict(mis=('G',)), UNSUPPORTED), (dict(M=0), BAD_ARG),
                 (dict(K=0), BAD_ARG), (dict(lddb=124), BAD_ARG), (dict(ldx=60), BAD_ARG), (dict(ldg=60), BAD_ARG)]
DGWG_NULLS = ('dB', 'W1t', 'X', 'G', 'scale', 'shift', 'mean', 'invstd', 'dW', 'ws')
