"""Float64 restatement of the BatchNorm (+ReLU) entry points of csrc/bn.hip, written out from the formulas, with the figures
the kernel tests build their tolerances from (test_bn_ref_host.py proves it, test_gpu_bn_forms.py uses it).  Not imported by
the package; no nn.BatchNorm* in here.

Every function takes torch tensors of any float type, computes in float64 and returns a SimpleNamespace.  Next to each REDUCED
quantity q_c = sum_r t_rc it returns `<q>_abs` = sum_r |t_rc| and `<q>_min` = min_r |t_rc| over the rows that contribute (rows the
ReLU or the pooling window mask out do not; a channel without contributing rows has min = +inf).  Next to each element-wise
output it returns `<name>_mag`: the magnitude sum of the terms of its last multiply-add chain.

Tolerances (u = 2^-24, K chosen in test_gpu_bn_forms.py from a plain fp32 torch evaluation, never from the kernels):
  reduced        |err_c| <= K u sum_r |t_rc|                      (+ what the reconstruction of relu = 2 adds, analytically)
  element-wise   the bound of the reductions it depends on, propagated to first order, + 8 u * <name>_mag
Detectability: min_r |t_rc| >= 4 * tolerance_c, so that one dropped, doubled or mis-masked row of any channel is an error of at
least four tolerances.  It is scale-free - min / mean(|t|) >= 4 K u M - and decides the input recipe below: x = 4 + U(-2, 2) cannot
meet it for the centred terms (x - mean)^2 and dy * xhat at any M (some x lies next to the mean), so `recipe` leaves the middle
out: x = 4 + off_c +- U(1, 2); and with the measured K the right side is 0.74 at M = 131 329, so the spreads narrow up there.
"""
from types import SimpleNamespace as NS

import torch

from gridnext_amd._lib import CONSTANTS

U = 2.0 ** -24
EW = 8.0                      # roundings granted to the last multiply-add chain of an element-wise output
INF = float('inf')


def f32(v):
    """The value a C float argument carries."""
    return float(torch.tensor(v, dtype=torch.float32))


def _d(t):
    return None if t is None else t.detach().double()


def _min_over(t_abs, keep):
    """min over rows of t_abs[r][c] where keep[r][c]; +inf for a channel that keeps none."""
    return torch.where(keep, t_abs, torch.full_like(t_abs, INF)).min(0).values


# ------------------------------------------------------------------------------------------------------------ forward
def stats(x, gamma, beta, running_mean, running_var, momentum, eps):
    """Training-mode statistics of x[M][C]: mean, invstd of the biased variance, the folded affine, torch's running update
    (unbiased variance; M = 1 keeps the biased one, as the kernels do)."""
    x = _d(x)
    M, C = x.shape
    g = torch.ones(C, dtype=torch.float64) if gamma is None else _d(gamma)
    b = torch.zeros(C, dtype=torch.float64) if beta is None else _d(beta)
    s = x.sum(0)
    mean = s / M
    d2 = (x - mean) ** 2
    m2 = d2.sum(0)
    var = m2 / M
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = g * invstd
    shift = b - mean * scale
    r = NS(M=M, C=C, gamma=g, beta=b, momentum=momentum, eps=eps, sum=s, sum_abs=x.abs().sum(0), sum_min=x.abs().min(0).values,
           m2=m2, m2_abs=m2.clone(), m2_min=d2.min(0).values, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift,
           running_mean=None, running_var=None, rm_old=_d(running_mean), rv_old=_d(running_var))
    r.unbiased = m2 / (M - 1) if M > 1 else var
    if running_mean is not None:
        r.running_mean = (1.0 - momentum) * r.rm_old + momentum * mean
    if running_var is not None:
        r.running_var = (1.0 - momentum) * r.rv_old + momentum * r.unbiased
    return r


def stats_tol(r, K):
    """Per-channel tolerances of everything gnx_bn_train_stats writes.  The second moment is taken about the ROUNDED mean:
    sum (x - mean - e)^2 = m2 + M e^2 exactly (the first-order term is e * sum (x - mean) = 0)."""
    M = r.M
    t = NS()
    t.sum = K * U * r.sum_abs
    t.mean = t.sum / M + U * r.mean.abs()
    t.m2 = K * U * r.m2_abs + M * t.mean ** 2
    t.var = t.m2 / M + U * r.var
    t.invstd = 0.5 * r.invstd ** 3 * t.var + EW * U * r.invstd
    t.scale = r.gamma.abs() * t.invstd + EW * U * r.scale.abs()
    t.shift = r.gamma.abs() * (t.mean * r.invstd + r.mean.abs() * t.invstd) + EW * U * (r.beta.abs() + (r.mean * r.scale).abs())
    if r.running_mean is not None:
        t.running_mean = r.momentum * t.mean + EW * U * (((1 - r.momentum) * r.rm_old).abs() + (r.momentum * r.mean).abs())
    if r.running_var is not None:
        t.running_var = (r.momentum * t.m2 / max(M - 1, 1) +
                         EW * U * (((1 - r.momentum) * r.rv_old).abs() + (r.momentum * r.unbiased).abs()))
    return t


def fold_eval(gamma, beta, running_mean, running_var, eps):
    """Eval-mode fold: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale."""
    rm, rv = _d(running_mean), _d(running_var)
    C = rm.numel()
    g = torch.ones(C, dtype=torch.float64) if gamma is None else _d(gamma)
    b = torch.zeros(C, dtype=torch.float64) if beta is None else _d(beta)
    invstd = 1.0 / torch.sqrt(rv + eps)
    scale = g * invstd
    shift = b - rm * scale
    return NS(C=C, gamma=g, beta=b, mean=rm, invstd=invstd, scale=scale, shift=shift)


def fold_tol(f):
    """As stats_tol, with exact inputs: invstd is the end of its own chain (add, sqrt, divide); scale = gamma invstd carries
    invstd's bound, shift = beta - mean scale carries scale's."""
    t = NS()
    t.invstd = EW * U * f.invstd
    t.scale = f.gamma.abs() * t.invstd + EW * U * f.scale.abs()
    t.shift = f.mean.abs() * t.scale + EW * U * (f.beta.abs() + (f.mean * f.scale).abs())
    return t


def apply(x, scale, shift, relu):
    """y = [relu](scale x + shift); y_mag = |scale x| + |shift|."""
    x, scale, shift = _d(x), _d(scale), _d(shift)
    y = x * scale + shift
    if relu:
        y = y.clamp_min(0.0)
    return NS(y=y, y_mag=(x * scale).abs() + shift.abs())


def apply_tol(a, x, tol_scale=None, tol_shift=None):
    """Element-wise tolerance of y: the statistics' bounds pushed through the (1-Lipschitz) ReLU, + 8 u y_mag."""
    t = EW * U * a.y_mag
    if tol_scale is not None:
        t = t + _d(x).abs() * tol_scale + tol_shift
    return t


def colsum(x, out_old=None):
    x = _d(x)
    s = x.sum(0)
    r = NS(M=x.shape[0], sum=s, sum_abs=x.abs().sum(0), sum_min=x.abs().min(0).values, out=s, out_mag=None)
    if out_old is not None:
        r.out = _d(out_old) + s
        r.out_mag = _d(out_old).abs() + s.abs()
    return r


def colsum_tol(r, K):
    t = K * U * r.sum_abs
    return t if r.out_mag is None else t + EW * U * r.out_mag


# ------------------------------------------------------------------------------------------------------------ backward
def bwd(dy, x, scale, shift, mean, invstd, relu, training, dx_old=None, dgamma_old=None, dbeta_old=None, rows=None):
    """Backward of y = [relu](bn(x)).  relu: 0 = none; 1 = x is the BatchNorm input, mask = scale x + shift > 0; 2 = x holds the
    ACTIVATED map a = relu(scale x + shift): mask = a > 0 and x = (a - shift) / scale (include/gridnext_hip.h).  training: batch
    statistics (dx = scale (dz - s1 / M - xhat s2 / M)) or running ones (dx = scale dz).  `rows` [M] bool: rows that carry a
    gradient at all (pooled form); the others count as masked."""
    dy, x, scale, shift, mean, invstd = [_d(t) for t in (dy, x, scale, shift, mean, invstd)]
    M, C = x.shape
    extra = torch.zeros_like(x)
    if relu == 2:
        mask = x > 0
        extra = U * (x.abs() + shift.abs()) / scale.abs()            # what rounding (a - shift) / scale moves x by
        x = (x - shift) / scale
    elif relu:
        mask = (x * scale + shift) > 0
    else:
        mask = torch.ones_like(x, dtype=torch.bool)
    if rows is not None:
        mask = mask & rows[:, None]
    dz = torch.where(mask, dy, torch.zeros_like(dy))
    xhat = (x - mean) * invstd
    t1, t2 = dz, dz * xhat
    s1, s2 = t1.sum(0), t2.sum(0)
    g = dz - s1 / M - xhat * s2 / M if training else dz
    dx_new = scale * g
    r = NS(M=M, C=C, training=bool(training), scale=scale, xhat=xhat, mask=mask,
           s1=s1, s1_abs=t1.abs().sum(0), s1_min=_min_over(t1.abs(), mask),
           s2=s2, s2_abs=t2.abs().sum(0), s2_min=_min_over(t2.abs(), mask),
           s2_extra=(dz.abs() * invstd.abs() * extra).sum(0),
           dx=dx_new, dgamma=s2, dbeta=s1, dgamma_mag=None, dbeta_mag=None)
    r.dx_mag = scale.abs() * (dz.abs() + ((s1.abs() + (xhat * s2).abs()) / M if training else 0.0))
    if dx_old is not None:
        r.dx = dx_new + _d(dx_old)
        r.dx_mag = r.dx_mag + _d(dx_old).abs() + dx_new.abs()
    if dgamma_old is not None:
        r.dgamma = _d(dgamma_old) + s2
        r.dgamma_mag = _d(dgamma_old).abs() + s2.abs()
    if dbeta_old is not None:
        r.dbeta = _d(dbeta_old) + s1
        r.dbeta_mag = _d(dbeta_old).abs() + s1.abs()
    return r


def bwd_tol(r, K):
    t = NS()
    t.s1 = K * U * r.s1_abs
    t.s2 = K * U * r.s2_abs + r.s2_extra
    t.dbeta = t.s1 if r.dbeta_mag is None else t.s1 + EW * U * r.dbeta_mag
    t.dgamma = t.s2 if r.dgamma_mag is None else t.s2 + EW * U * r.dgamma_mag
    t.dx = EW * U * r.dx_mag
    if r.training:
        t.dx = t.dx + r.scale.abs() * (t.s1 + r.xhat.abs() * t.s2) / r.M
    return t


def _unpool(dYp, imgs, S):
    """The gradient of the S x S map under a floor 2x2 average pool: a quarter of the window's value; rows and columns the
    pool does not reach (odd S) get none.  Returns the full-size gradient [imgs S S][C] and the rows that are pooled."""
    dYp = _d(dYp)
    C = dYp.shape[1]
    So = S // 2
    full = torch.zeros(imgs, S, S, C, dtype=torch.float64)
    full[:, :2 * So, :2 * So] = 0.25 * dYp.view(imgs, So, So, C).repeat_interleave(2, 1).repeat_interleave(2, 2)
    rows = torch.zeros(imgs, S, S, dtype=torch.bool)
    rows[:, :2 * So, :2 * So] = True
    return full.view(imgs * S * S, C), rows.view(-1)


def pooled_bwd(dYp, x, scale, shift, mean, invstd, S, dgamma_old=None, dbeta_old=None):
    """gnx_bn_relu_bwd_pooled: norm (eval statistics) -> relu adjoint from the gradient dYp [imgs (S//2)^2][C] of the POOLED map."""
    imgs = x.shape[0] // (S * S)
    dy, rows = _unpool(dYp, imgs, S)
    return bwd(dy, x, scale, shift, mean, invstd, 1, 0, None, dgamma_old, dbeta_old, rows=rows)


def bnrelu_avgpool2(x, scale, shift, S):
    """[imgs (S//2)^2][C]: the 2x2 floor average pool of relu(scale x + shift) over each S x S map."""
    x = _d(x)
    C = x.shape[1]
    imgs, So = x.shape[0] // (S * S), S // 2
    a = apply(x, scale, shift, 1)

    def pool(t):
        t = t.view(imgs, S, S, C)[:, :2 * So, :2 * So].reshape(imgs, So, 2, So, 2, C)
        return t.sum((2, 4)).reshape(imgs * So * So, C) * 0.25
    return NS(out=pool(a.y), out_mag=pool(a.y_mag))


# ------------------------------------------------------------------------------------------------------------ inputs
def recipe(M, C, seed=0):
    """The operands of one case, float32.  x = 4 + off_c +- U(1, 2) (off_c in [-1, 1]); |dy| in [0.5, 1.5], random sign; gamma in
    +-[0.5, 1.5], about a third negative; beta ~ N(0, 1); running statistics off their defaults and next to the batch's, so that
    the eval-mode xhat keeps away from zero as the training-mode one does.  Above NARROW_ABOVE rows the spreads narrow to
    x = 4 + off_c +- U(0.4, 0.45), |dy| in [0.95, 1.05]: detectability asks min / mean of the terms >= 4 K u M, 0.74 at M = 131 329
    with the measured K, and the narrow recipe gives 0.85 (x: 2.55 / 3), 0.88 ((x - mean)^2: 0.16 / 0.181) and 0.88 (dy xhat).  Rows 0 and M - 1 carry dy times 3 and x times 3 on
    the upper branch (x = 3 (4 + off_c + U(1, 2))): a boundary row that is dropped or counted twice is the largest error a row
    can make."""
    g = torch.Generator().manual_seed(1000003 * seed + 131 * M + C)

    def rnd(*s):
        return torch.rand(*s, generator=g, dtype=torch.float64)

    def sgn(*s, p=0.5):
        return torch.where(rnd(*s) < p, -1.0, 1.0).double()
    (d_lo, d_hi), (dy_lo, dy_hi), jitter = ((0.4, 0.45), (0.95, 1.05), 0.01) if M > NARROW_ABOVE else ((1.0, 2.0), (0.5, 1.5), 0.2)
    off = 2 * rnd(C) - 1
    x = 4 + off + sgn(M, C) * (d_lo + (d_hi - d_lo) * rnd(M, C))
    dy = sgn(M, C) * (dy_lo + (dy_hi - dy_lo) * rnd(M, C))
    for row in {0, M - 1}:
        x[row] = 3 * (4 + off + (x[row] - 4 - off).abs())       # the upper branch: 3 x of the lower one can sit ON the mean
        dy[row] *= 3
    r = NS(M=M, C=C, x=x, dy=dy, gamma=sgn(C, p=1 / 3) * (0.5 + rnd(C)), beta=torch.randn(C, generator=g, dtype=torch.float64),
           running_mean=4 + off + jitter * (rnd(C) - 0.5), running_var=1.5 + rnd(C),
           dx_old=torch.randn(M, C, generator=g, dtype=torch.float64), dgamma_old=torch.randn(C, generator=g, dtype=torch.float64),
           dbeta_old=torch.randn(C, generator=g, dtype=torch.float64))
    for k, v in vars(r).items():
        if torch.is_tensor(v):
            setattr(r, k, v.float())
    return r


def away_from_relu_kink(x, scale_shift_of, thresh=1e-4):
    """Nudge the entries of x (float32) whose BatchNorm output lies within `thresh` of zero: there the fp32 kernel and the
    float64 reference may take different sides of the ReLU, which says nothing about either.  scale_shift_of(x) returns the
    folded affine that x would be normalised with.  Batch statistics move with x, hence the loop - and hence nudges of
    alternating sign: where the kink runs through a dense cluster (the narrow recipe), a hundred nudges one way move the mean
    by about `thresh` and push as many new entries onto the kink."""
    x = x.clone()
    for _ in range(6):
        sc, sh = scale_shift_of(x)
        near = (x.double() * sc.double() + sh.double()).abs() < thresh
        n = int(near.sum())
        if n == 0:
            return x
        x[near] += 0.02 * (1 - 2 * (torch.arange(n) % 2)).float()
    raise AssertionError("could not move x off the ReLU kink")


def bwd_operands(rec, relu, training, eps):
    """x (moved off the kink for relu cases) and the fp32 per-channel operands of gnx_bn_relu_bwd for one recipe: batch
    statistics (training) or the fold of the recipe's running ones.  For relu = 2 also `a`: relu(scale x + shift) in float64,
    rounded to float32 - the operand that form reads in place of x."""
    def fold(x):
        if training:
            return stats(x, rec.gamma, rec.beta, None, None, 0.1, eps)
        return fold_eval(rec.gamma, rec.beta, rec.running_mean, rec.running_var, eps)

    def scale_shift_of(x):
        s = fold(x)
        return s.scale.float(), s.shift.float()
    x = away_from_relu_kink(rec.x, scale_shift_of) if relu else rec.x
    s = fold(x)
    o = NS(x=x, scale=s.scale.float(), shift=s.shift.float(), mean=s.mean.float(), invstd=s.invstd.float(), a=None)
    if relu == 2:
        o.a = apply(x, o.scale, o.shift, 1).y.float()
    return o


def detectable(r_min, tol):
    """min_r |t_rc| >= 4 tol_c in every channel (channels without a contributing row have nothing to detect)."""
    return bool((r_min >= 4 * tol).all())


# ------------------------------------------------------------------------------------------------------------ dispatch
# bn_train_stats_plan / bn_relu_bwd_plan of csrc/bn.hip restated ("BatchNorm forms"); gnx_bn_train_stats_form and
# gnx_bn_relu_bwd_form answer with CODES[body].
BN_SL, BN_SMALL_M, BN_R, BN_MULTI_M = 256, 4992, 4, 8192
ROWS_PER_BLOCK, MAX_SLABS = 256, 512
CODES = {k[len('GNX_BN_'):].lower(): v for k, v in CONSTANTS.items() if k.startswith('GNX_BN_')}
FORMS = tuple(sorted(CODES, key=CODES.get))                   # multi, small_keep, small_strip, slab_vec, slab, eval_fused
BAD_ARG, UNSUPPORTED = CONSTANTS['GNX_ERR_BAD_ARG'], CONSTANTS['GNX_ERR_UNSUPPORTED']


def _cdiv(a, b):
    return -(-a // b)


def slab_count(M):
    return min(_cdiv(M, ROWS_PER_BLOCK), MAX_SLABS)


def rows_form(M, C):
    """The form the row count allows when every operand is 16-B (bn_rows_form)."""
    if 8 * BN_SL < M <= BN_MULTI_M and C % 4 == 0 and _cdiv(C, 16) * BN_R <= 256:
        return 'multi'
    if M <= BN_SMALL_M:
        return 'small_keep' if M <= 8 * BN_SL else 'small_strip'
    return 'slab'


def _workgroups(body, M, C):
    """Workgroups of the first launch."""
    if body in ('multi', 'small_keep', 'small_strip'):
        return _cdiv(C, 16) * (BN_R if body == 'multi' else 1)
    return slab_count(M) * _cdiv(C, 64)


def form(M, C, ld, x_al, ldy=None, y_al=True, ws_al=True):
    """gnx_bn_train_stats[_apply]: the statistics body (chosen on x alone: its pointer 16-B aligned `x_al`, its leading
    dimension), whether the apply rides on that launch (`fused`; ldy None: no y), the workgroups of the first launch."""
    xv = C % 4 == 0 and ld % 4 == 0 and x_al
    body = rows_form(M, C) if xv else 'slab'
    if body == 'slab' and xv and ws_al:
        body = 'slab_vec'
    fused = ldy is not None and ldy % 4 == 0 and y_al and body not in ('slab', 'slab_vec')
    return NS(body=body, fused=int(fused), workgroups=_workgroups(body, M, C))


def bwd_form(M, C, ld, al, lddx, dx_al, relu, training, ws_al=True):
    """gnx_bn_relu_bwd: dy and x share `ld` and the alignment `al` (the per-channel vectors are 16-B); lddx None: no dx.  body
    None: GNX_ERR_UNSUPPORTED.  dx_vec4: on the two slab forms, dx through the 16-B kernel (it also reads the reduced sums, which
    sit 2 slabs C floats into the workspace)."""
    pv = C % 4 == 0 and ld % 4 == 0 and al
    v4all = pv and (lddx is None or (lddx % 4 == 0 and dx_al))
    if relu == 2 and (training or not v4all):
        return NS(body=None, dx_vec4=0, workgroups=0)
    body = rows_form(M, C) if v4all and relu != 2 else 'slab'
    dx_vec4 = False
    if body == 'slab':
        if not training and v4all:
            body = 'eval_fused'
        else:
            body = 'slab_vec' if pv else 'slab'
            dx_vec4 = lddx is not None and v4all and ws_al and (2 * slab_count(M) * C) % 4 == 0
    return NS(body=body, dx_vec4=int(dx_vec4), workgroups=_workgroups(body, M, C))


# ------------------------------------------------------------------------------------------------------------ shape grid
# The smallest shapes at which each kernel form of csrc/bn.hip and each of its edges exists ("BatchNorm forms"), each
# group under the form it is there for: the forward's on 16-B operands (`window`; `misaligned` where 4 does not divide C).
GRID_GROUPS = (
    ('small_keep', [(M, C) for M in (2, 255, 257, 2047, 2048) for C in (4, 12, 68)]),    # single workgroup, rows kept in registers
    ('multi', [(2049, C) for C in (4, 36, 1024)]),                               # first row count of the four-workgroup form
    ('multi', [(M, C) for M in (4993, 8191, 8192) for C in (12, 100)]),          # four workgroups, ragged rows / channel block
    ('small_strip', [(M, 1040) for M in (2049, 4992)]),                          # single workgroup walking its strip (C > 1024)
    ('slab_vec', [(8193, C) for C in (8, 64, 68)]),                              # first row count of the slab form, 16-B loads
    ('slab', [(M, C) for M in (8193, 300) for C in (3, 50, 67)]),                # scalar slabs
    ('slab_vec', [(131329, 12)]),                                                # > 512 slabs; > 4096 element-wise workgroups
    ('slab_vec', [(4993, 1040)]),                                                # ... and its first row count where C > 1024
)
GRID = [mc for _, group in GRID_GROUPS for mc in group]
GRID_FORM = {mc: body for body, group in GRID_GROUPS for mc in group}
# (case below, case above, body below, body above): each row threshold of the dispatch, 16-B operands
ROW_EDGES = [((2048, 4), (2049, 4), 'small_keep', 'multi'), ((4992, 1040), (4993, 1040), 'small_strip', 'slab_vec'),
             ((8192, 12), (8193, 8), 'multi', 'slab_vec')]
LAYOUTS = ('contiguous', 'window', 'misaligned')


def layout(name, C):
    """(ld, off) of the window [0:M, off:off+C] inside an [M + 3][ld] tensor."""
    if name == 'contiguous':
        return C, 0
    if name == 'window':
        return C + 32, 16
    return C + 7, 1                      # neither the pointer nor (for even C) the row stride is a multiple of 16 B


# gnx_colsum: both kernels (16-B loads / scalar), one row, a ragged block, more than 512 slabs; two workgroups in y (C = 68)
COLSUM_CASES = ([(M, C, lay) for M in (1, 257, 131329) for C, lay in ((12, 'window'), (7, 'misaligned'), (12, 'misaligned'))] +
                [(M, 68, 'contiguous') for M in (1, 257)])
COLSUM_FORM = {'window': 'slab_vec', 'misaligned': 'slab', 'contiguous': 'slab_vec'}     # gnx_colsum runs the slab kernels only
# the 16-B dx pass beyond 4096 workgroups (its grid-stride loop): M C / 4 > 4096 * 256 needs C >= 32 at 131 329 rows
DX_VEC4_LOOP = (131329, 36)
ACT_GRID = [(M, C) for M in (257, 2049, 8193) for C in (12, 64)]                 # relu = 2
ACT_FORM = 'eval_fused'                                                          # ... whatever the row count
POOL_GRID = [(S, imgs, C) for S in (4, 5, 7) for imgs in (1, 3) for C in (12, 68)]
POOL_FORM = 'eval_fused'                                                         # gnx_bn_relu_bwd_pooled has no other body
NARROW_ABOVE = 32768
# K = max(8, 4 x the largest rounding ratio of a plain fp32 torch evaluation on the device): measured, see test_gpu_bn_forms.py
K_FLOOR = 8.0
TORCH_FP32_RATIO = 5.9181
K = max(K_FLOOR, 4 * TORCH_FP32_RATIO)


def mom_eps(i):
    """momentum / eps alternate over the cases: torch's defaults and (0.3, 1e-3), as the C floats the kernels receive."""
    return (f32(0.1), f32(1e-5)) if i % 2 == 0 else (f32(0.3), f32(1e-3))


def aligned(name):
    """The window of a layout starts on a 16-B boundary (the tensor it is cut from does)."""
    return layout(name, 4)[1] % 4 == 0


def form_of(M, C, lay, ylay=None):
    """`form` of a case of test_gpu_bn_forms.py: x in layout `lay`; y (ylay None: none) in its own, 4 floats more per row."""
    ld = layout(lay, C)[0]
    return form(M, C, ld, aligned(lay), None if ylay is None else layout(ylay, C)[0] + 4, ylay is None or aligned(ylay))


BWD_LAYOUTS = LAYOUTS + ('dx_misaligned',)
#               relu training accumulate dx_accumulate dx_null dgamma_null also_sync: what test_backward runs on every case
BWD_COMBOS = [(0, 1, 0, 0, False, False, True),
              (1, 1, 1, 1, False, False, True),
              (1, 0, 0, 1, False, False, False),
              (0, 0, 1, 0, False, False, True),
              (1, 1, 0, 0, True, False, False),
              (1, 0, 1, 0, True, False, True),
              (0, 1, 0, 1, False, True, False)]


def bwd_layouts(name):
    """(layout of dy and x, layout of dx).  dx_misaligned: everything 16-B aligned but dx - 16-B partial sums, scalar dx pass."""
    return ('window', 'misaligned') if name == 'dx_misaligned' else (name, name)


def bwd_form_of(M, C, lay, dxlay, relu, training):
    """`bwd_form` of a case: dy and x in layout `lay`, dx (dxlay None: NULL) in `dxlay`."""
    return bwd_form(M, C, layout(lay, C)[0], aligned(lay), None if dxlay is None else layout(dxlay, C)[0],
                    dxlay is None or aligned(dxlay), relu, training)
