"""Float64 reference of the fp32 GEMM entry points of csrc/gemm_f32.hip (gnx_gemm_f32 / gnx_gemm_f32_ws), the dispatch of
gemm_f32_impl restated in Python, and the grid of shapes the kernel tests run (test_gemm_ref_host.py proves it on the CPU,
test_gpu_gemm_forms.py uses it).  Not imported by the package.

  C[M][N] = A[M][K] B[N][K]^T (+ bias[N]) (+ C0[M][N])

Tolerance, per element (u = 2^-24):  |err_mn| <= G u T_mn,  T = |A| |B|^T + |bias| + |C0|  (the magnitude sum of every term
of the element's chain).  G = max(8, 4 x the largest ratio |err| / (u T) of two plain fp32 evaluations - torch.matmul on the
device, a sequential multiply-add chain on the CPU - over every shape of GRID): measured on references only, see
test_gpu_gemm_forms.py.
Detectability: `recipe` draws every operand with a magnitude in [0.5, 1.5] and a random sign, so every product term is at
least 0.25 in magnitude; `detectable` asks 0.25 >= 4 x the largest tolerance of the case, so that one dropped, doubled or
misplaced K term of any element is an error of at least four tolerances.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import torch

from gridnext_amd._lib import CONSTANTS

U = 2.0 ** -24
MIN_TERM = 0.25
G_FLOOR = 8.0
TORCH_FP32_RATIO = 5.9579        # torch.matmul, fp32, on the device: largest |err| / (u T) over GRID (test_gpu_gemm_forms.py)
CHAIN_FP32_RATIO = 3.6419        # sequential fp32 multiply-add chain on the CPU, the same figure (test_gemm_ref_host.py)
G = max(G_FLOOR, 4 * max(TORCH_FP32_RATIO, CHAIN_FP32_RATIO))
HOLD_F32_ABOVE = 1 << 26      # operands with more elements stay float32 tensors (the values are float32 either way)


# ------------------------------------------------------------------------------------------------------------ inputs
def _signed(g, *shape):
    """float32 values with a magnitude in [0.5, 1.5] and a random sign."""
    u = torch.rand(*shape, generator=g, dtype=torch.float32).mul_(2).sub_(1)
    return u.add_(torch.copysign(torch.tensor(0.5), u))


@functools.lru_cache(maxsize=2)
def recipe(M, N, K, seed=0):
    """The operands of one case: A [M][K], B [N][K], bias [N], C0 [M][N]; float32 values held in float64 (an operand of more
    than HOLD_F32_ABOVE elements stays a float32 tensor).  Shared between tests: do not write to them."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 131 * N + K)

    def hold(t):
        return t if t.numel() > HOLD_F32_ABOVE else t.double()
    return NS(M=M, N=N, K=K, A=hold(_signed(g, M, K)), B=hold(_signed(g, N, K)), bias=hold(_signed(g, N)),
              C0=hold(_signed(g, M, N)))


def product(A, B, bias=None, C0=None, parts=None):
    """(ref, T): ref = A B^T (+ bias) (+ C0) in float64 and the per-element magnitude sum T = |A| |B|^T + |bias| + |C0|.
    `parts`: (A B^T, |A| |B|^T) in float64 from an earlier call on the same A and B."""
    if parts is None:
        A, B = A.double(), B.double()
        parts = (A @ B.t(), A.abs() @ B.abs().t())
    ref, T = parts
    if bias is not None:
        ref, T = ref + bias.double(), T + bias.double().abs()
    if C0 is not None:
        ref, T = ref + C0.double(), T + C0.double().abs()
    return ref, T


def tol(T, g=None):
    return (G if g is None else g) * U * T


def detectable(t):
    """The smallest product term of the recipe is at least four times the largest tolerance of the case."""
    return MIN_TERM >= 4 * float(t.max())


def chain_fp32(A, B):
    """A B^T as a sequential fp32 multiply-add chain over k (one rounding for the product, one for the sum)."""
    A, B = A.float(), B.float()
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    for k in range(A.shape[1]):
        acc = acc + A[:, k, None] * B[None, :, k]
    return acc


def sample(n, most):
    """At most `most` indices of range(n), evenly spread, both ends included."""
    if n <= most:
        return torch.arange(n)
    return torch.unique(torch.linspace(0, n - 1, most).round().long())


# ------------------------------------------------------------------------------------------------------------ dispatch
def _cdiv(a, b):
    return -(-a // b)


def wide_splits(M, N, K):
    """gemm_wide_splits: 0 = not a wide shape."""
    if M < 2048 or N < 256 or K < 512:
        return 0
    tiles, nkt = _cdiv(M, 256) * _cdiv(N, 128), _cdiv(K, 32)
    return max(1, min(512 // tiles, nkt // 4, 16))


def tall_splits(M, N, K):
    """gemm_tall_splits."""
    if N > 128 or K < 1024:
        return 1
    s = min(_cdiv(K, 64) // 8, 3)
    return 1 if s < 1 or s * M * N > (1 << 26) else s


def workspace_floats(M, N, K):
    """gnx_gemm_f32_workspace."""
    s, t = wide_splits(M, N, K), tall_splits(M, N, K)
    return s * M * N if s > 1 else (t * M * N if s == 0 and t > 1 else 0)


def form(M, N, K, lda, ldb, a_kmajor, b_kmajor, a_misaligned, b_misaligned, has_ws):
    """(body, S, a_vec, b_vec) of one call: body in {wide, big, tall, plain}, S the K splits, *_vec whether the operand goes
    through 16-B buffer loads (always, on the wide and big bodies).  The 32-bit offset limits of gemm_f32_impl are far above
    every shape here and are asserted, not modelled."""
    assert (K + 128) * max(lda, ldb) < (1 << 29) and (M + 128) * lda < (1 << 29) and (N + 128) * ldb < (1 << 29)
    a_vec = (not a_misaligned) and lda % 4 == 0 and (M % 4 == 0 if a_kmajor else K % 4 == 0)
    b_vec = (not b_misaligned) and ldb % 4 == 0 and (N % 4 == 0 if b_kmajor else K % 4 == 0)
    t_ok = a_vec and b_vec
    S = wide_splits(M, N, K) if t_ok else 0
    if S > 1 and not has_ws:
        S = 1
    if S >= 1:
        return 'wide', S, True, True
    if t_ok and M >= 2048 and N >= 256:
        return 'big', 1, True, True
    s = tall_splits(M, N, K) if has_ws else 1
    return ('tall' if s > 1 else 'plain'), s, a_vec, b_vec


BODIES = ('wide', 'big', 'tall', 'plain')
CODES = {b: CONSTANTS['GNX_GEMM_' + b.upper()] for b in BODIES}         # what gnx_gemm_f32_form answers
BAD_ARG, UNSUPPORTED = CONSTANTS['GNX_ERR_BAD_ARG'], CONSTANTS['GNX_ERR_UNSUPPORTED']


def workgroups(M, N, K, body, S):
    """The grid of the product's launch: wide - (m tile, split) units in whole rounds of 8, per column tile of 128; big - m tiles
    of 128 in whole rounds of 8, per column tile of 64; tall / plain - 64 x 64 tiles x splits."""
    if body == 'wide':
        return _cdiv(_cdiv(M, 256) * S, 8) * 8 * _cdiv(N, 128)
    if body == 'big':
        return _cdiv(_cdiv(M, 128), 8) * 8 * _cdiv(N, 64)
    return _cdiv(M, 64) * _cdiv(N, 64) * S


def wide_units(M, S):
    """(m tile, split) units of the wide body; its grid rounds them up to whole rounds of 8."""
    return _cdiv(M, 256) * S


def wide_split_tiles(K, S):
    """K tiles of each split of the wide body."""
    nkt = _cdiv(K, 32)
    per = _cdiv(nkt, S)
    return [max(0, min(nkt, (s + 1) * per) - s * per) for s in range(S)]


# ------------------------------------------------------------------------------------------------------------ layouts
LAYS = ('aligned', 'shifted', 'oddld')


def lay(name, cols):
    """(ld, off, shift) of an operand whose rows hold `cols` floats, as a window [0:rows, off:off+cols] of a [rows + 3][ld]
    tensor that starts `shift` floats into 16-B aligned storage.  aligned: pointer and rows 16-B aligned; shifted: the same
    rows one float further (pointer misaligned, 4 | ld); oddld: pointer aligned, ld = 1 mod 4.  ld > cols everywhere."""
    ld = (cols + 3) // 4 * 4 + 8
    return {'aligned': (ld, 4, 0), 'shifted': (ld, 4, 1), 'oddld': (ld + 1, 4, 0)}[name]


def ld_of(c, which):
    """Leading dimension of operand 'a' / 'b' of a case."""
    if which == 'a':
        return lay(c.alay, c.M if c.ak else c.K)[0]
    return lay(c.blay, c.N if c.bk else c.K)[0]


def form_of(c):
    return form(c.M, c.N, c.K, ld_of(c, 'a'), ld_of(c, 'b'), c.ak, c.bk, c.alay == 'shifted', c.blay == 'shifted', c.ws)


# ------------------------------------------------------------------------------------------------------------ the grid
Case = namedtuple('Case', 'M N K ak bk alay blay bias acc ws')
PAIRS = ((0, 0), (1, 0), (0, 1), (1, 1))                  # (a_kmajor, b_kmajor)
FLAGS = ((0, 0), (1, 0), (0, 1), (1, 1))                  # (bias, accumulate)


def lite(M, N, K, ws=1, alay='aligned', blay='aligned', rot=0):
    """The four layout pairs, (bias, accumulate) rotating."""
    return [Case(M, N, K, ak, bk, alay, blay, *FLAGS[(i + rot) % 4], ws) for i, (ak, bk) in enumerate(PAIRS)]


def full(M, N, K, ws=1):
    """The four layout pairs x bias NULL / present x accumulate 0 / 1."""
    return [Case(M, N, K, ak, bk, 'aligned', 'aligned', bias, acc, ws) for ak, bk in PAIRS for bias, acc in FLAGS]


def vec_pairs(M, N, K):
    """Every (A, B) pair of the three operand layouts x the four layout pairs; (bias, accumulate) fixed per layout pair, so
    that the runs of one pair differ in the loaders alone."""
    return [Case(M, N, K, ak, bk, al, bl, *FLAGS[i], 1) for i, (ak, bk) in enumerate(PAIRS) for al in LAYS for bl in LAYS]


WIDE, WIDE_PAST = (2048, 256, 512), (2052, 256, 512)      # M N = 2048 * 256: one round of the reduce kernel's grid; past it
BIG = (2048, 256, 36)
TALL, PLAIN_VEC, TALL_VEC = (130, 128, 1024), (132, 68, 132), (132, 68, 1028)
TALL_ROUND, TALL_ROUND_PAST = (4096, 128, 1024), (4097, 128, 1024)
WORKLOAD = (4992, 500, 2000)
EMPTY_SPLIT = (2048, 512, 1312)                            # 41 K tiles over 10 splits of 5: split 9 gets none, split 8 one
CAP_BELOW, CAP_ABOVE = (174762, 128, 1536), (174763, 128, 1536)       # 3 M N <= 2^26 < 3 M N: the slab workspace's cap
HUGE = (CAP_BELOW, CAP_ABOVE)                              # run by a test of their own, reference on sampled rows
RAGGED_MN, RAGGED_K = (1, 63, 64, 65, 130), (1, 3, 4, 63, 64, 65, 130)


def _grid():
    g = []
    # wide / big / plain: each dimension around its threshold, the other two at theirs
    for M in (2044, 2047, 2052):
        g += lite(M, 256, 512, rot=M)
    for N in (252, 255, 257, 260):
        g += lite(2048, N, 512, rot=N)
    for K in (508, 516):
        g += lite(2048, 256, K, rot=K)
    g += [Case(2048, 256, 513, 1, 1, 'aligned', 'aligned', 1, 0, 1),          # K off 4: only K-major operands stay 16-B
          Case(2048, 256, 513, 0, 1, 'aligned', 'aligned', 1, 1, 1)]
    # wide: S = 4 with and without workspace (S = 1), S = 15 and the cap 16, a split without a K tile and its neighbour
    g += full(*WIDE) + full(*WIDE, ws=0)
    g += lite(2048, 256, 2016) + lite(2048, 256, 2048, rot=1)
    g += lite(*EMPTY_SPLIT, rot=2) + lite(2048, 512, 1280, rot=3) + lite(*EMPTY_SPLIT, ws=0)
    g += [Case(*WORKLOAD, 1, 0, 'aligned', 'aligned', 1, 0, 1)]
    # big: one, two and sixteen K tiles; 16 and 17 row tiles; a ragged column tile; below it in M and in N
    for K in (4, 36, 508):
        for M in (2048, 2049):
            for N in (256, 257):
                if (M, N, K) != BIG:
                    g += lite(M, N, K, rot=M + N + K)
    g += full(*BIG) + lite(2047, 256, 36) + lite(2048, 255, 36) + lite(2048, 256, 37)
    # a wide and a big shape with one operand off 16 B: the 64 x 64 body
    for shape in (WIDE, BIG):
        g += lite(*shape, alay='shifted') + lite(*shape, blay='oddld', rot=1)
        g += lite(*shape, alay='oddld', rot=2) + lite(*shape, blay='shifted', rot=3)
    # tall: N and K around the thresholds of gemm_tall_splits, no workspace, one round of the reduce kernel's grid and past it
    for N in (128, 129, 132):
        for K in (1020, 1024):
            if (130, N, K) != TALL:
                g += lite(130, N, K, rot=N + K)
    g += lite(130, 128, 1472) + lite(130, 128, 1473, rot=1)
    g += full(*TALL) + lite(*TALL, ws=0)
    g += lite(*TALL_ROUND)[:2] + lite(*TALL_ROUND_PAST, rot=2)[:2]
    # the 64 x 64 body's four loader pairs, each scalar side both by pointer and by leading dimension: plain and tall
    g += vec_pairs(*PLAIN_VEC) + vec_pairs(*TALL_VEC)
    # plain: ragged tiles in every dimension; the operand layouts rotate
    i = 0
    for M in RAGGED_MN:
        for N in RAGGED_MN:
            for K in RAGGED_K:
                for j, (ak, bk) in enumerate(PAIRS):
                    g.append(Case(M, N, K, ak, bk, LAYS[(i + j) % 3], LAYS[(i // 3 + 2 * j) % 3], *FLAGS[(i + j) % 4], (i + j) % 2))
                i += 1
    # the slab workspace's cap, once
    g += [Case(*CAP_BELOW, 0, 0, 'aligned', 'aligned', 1, 0, 1), Case(*CAP_ABOVE, 0, 0, 'aligned', 'aligned', 1, 0, 1)]
    return list(dict.fromkeys(g))


def recipe_of(shape):
    """recipe(*shape); CAP_BELOW is the first rows of CAP_ABOVE's operands (one gigabyte of A serves both)."""
    if shape != CAP_BELOW:
        return recipe(*shape)
    r, M = recipe(*CAP_ABOVE), CAP_BELOW[0]
    return NS(M=M, N=r.N, K=r.K, A=r.A[:M], B=r.B, bias=r.bias, C0=r.C0[:M])


def t_bound(K):
    """An upper bound of T for the recipe: K terms of at most 1.5 * 1.5, bias and C0 of at most 1.5 each."""
    return 2.25 * K + 3.0


GRID = _grid()
SHAPES = list(dict.fromkeys((c.M, c.N, c.K) for c in GRID))              # in GRID's order, each once

# (shape below, shape above, (body, S) below, (body, S) above): both row-major, aligned, with workspace unless said
EDGES = [
    ((2047, 256, 512), WIDE, ('plain', 1), ('wide', 4)),
    ((2048, 255, 512), WIDE, ('plain', 1), ('wide', 4)),
    ((2048, 256, 508), WIDE, ('big', 1), ('wide', 4)),
    ((2047, 256, 36), BIG, ('plain', 1), ('big', 1)),
    ((2048, 255, 36), BIG, ('plain', 1), ('big', 1)),
    ((2048, 256, 2016), (2048, 256, 2048), ('wide', 15), ('wide', 16)),
    ((2048, 512, 1280), EMPTY_SPLIT, ('wide', 10), ('wide', 10)),
    (WIDE, WIDE_PAST, ('wide', 4), ('wide', 4)),
    (TALL, (130, 129, 1024), ('tall', 2), ('plain', 1)),
    ((130, 128, 1020), TALL, ('plain', 1), ('tall', 2)),
    ((130, 128, 1472), (130, 128, 1473), ('tall', 2), ('tall', 3)),
    (TALL_ROUND, TALL_ROUND_PAST, ('tall', 2), ('tall', 2)),
    (CAP_BELOW, CAP_ABOVE, ('tall', 3), ('plain', 1)),
]
