"""Float64 references of the stem and pool kernels (csrc/stem_pool.hip), a mirror of their launchers' dispatch, and the grid of
cases the kernel tests run (test_stem_ref_host.py proves all of it on the CPU, test_gpu_stem_forms.py uses it).  Not imported by
the package.  The mirror is held to the library: query_answer is what the gnx_*_form queries of stem_pool.hip must answer, code
and workgroups, and both tests ask them.

  conv      out[(i Ho + oy) Wo + ox][o] = sum_(c, ky, kx) x[i][c][oy s + ky - p][ox s + kx - p] w[o][c][ky][kx], zeros outside
  act       relu(pre * scale[o] + shift[o])
  maxpool   3x3 s2 p1 over the valid elements of the window, and the index 0..8 (3 row + column) of the FIRST maximal valid
            element of the row-major scan (torch's rule)
  avgpool   mean over the S2 positions of an image
  u8        ToTensor (u8 / 255) and Normalize ((v - mean) / std) in float32, as torchvision does them: the kernels promise
            those bits; the fp16-operand stem rounds patches and weights to fp16 first
all written from the definitions in float64 (the tap loop of `conv`, the scan of `maxpool`), with the wrong variants
(`dy`, `dx`, `twice`, `edge`, `padval`, `ge`, `carry`, `block`) the host test must see the comparator flag.

Inputs.  Kind 1 ('int'): patches and weights integers in [-2, 2] (uint8 patches: bytes 0 and 255 without Normalize, the floats
0 and 1), scale in {1, -1, 0.5, 2}, shift an integer in [-8, 8]: every product and partial sum is an integer of magnitude at
most 588, exact in fp32, as fp16 operands and (|conv| <= 128 on these seeds, asserted) in fp16 storage whatever the order of
the sum - the kernel must give the float64 reference bit for bit, window indices included, ties and all.
Kind 2 ('mag'): magnitudes in [0.5, 1.5] with a random sign (uint8: random bytes under Normalize); scale a magnitude in
[0.25, 0.75] with a random sign and shift in [2, 6], so that about a quarter of the map is cut by the ReLU while a window of
zeros only (an index tie kind 2 cannot judge) stays rare.

Tolerance of kind 2, per element (u = 2^-24, T = conv(|x|, |w|)):  |err_pre| <= G u T;  after act: |scale| G u T + u |act|;
after the max pool: the largest of the window;  after an fp16 store: + 2^-11 |ref| + 2^-25;  the fp16-operand stem: T and the
reference on the fp16-rounded operands.  The stand-alone pools see one fp32 rounding of act: u |act| (max pool), and the sum
of S2 / 4 terms per lane, the tree and the division: (ceil(S2 / 4) + 4) u mean(act) (average pool).
G = max(8, 4 x the largest |err| / (u T) of two plain fp32 evaluations of the convolutions of GRID against float64); the
kernel's own error has no part in it:
  torch's fp32 F.conv2d on the CPU                                    TORCH_FP32_RATIO
  a sequential fp32 multiply-add chain over (c, ky, kx) on the CPU     CHAIN_FP32_RATIO
(where each occurred: the constants below; measured by test_stem_ref_host.py, which prints its figures).

The window index of kind 2 is compared only where the reference's two largest window values differ by more than the sum of
their tolerances (`comparable`): a condition on the reference alone, at most MAX_EXCLUDED of the elements of any case
(asserted on the host); kind 1 covers the ties.
"""
import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

U = 2.0 ** -24
G_FLOOR = 8.0
MIN_TERM = 0.25
MAX_EXCLUDED = 0.01
# largest |err| / (u T) over the convolutions of GRID (kind 2) and the case it came from: G = 17.456.  The chain is elementwise IEEE
# arithmetic and is pinned by the host test; torch's blocking follows its build (the host test measures it on one thread, prints
# it and holds it to G / 4)
TORCH_FP32_RATIO = 4.3640        # torch's fp32 F.conv2d on the CPU, one thread
TORCH_FP32_AT = 'fused-f32-256-256-64-64-1'
CHAIN_FP32_RATIO = 4.1771        # sequential fp32 multiply-add chain on the CPU
CHAIN_FP32_AT = 'fused-f32-128-36-64-72-3'
G = max(G_FLOOR, 4 * max(TORCH_FP32_RATIO, CHAIN_FP32_RATIO))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DISTINCT = 7                     # a batch above a launch cap cycles this many patches: the caps 512, 256, 768 are 1, 4, 5 mod 7
CAP = {('f32', 128): 512, ('f32', 256): 256, ('f16', 128): 768, ('f16', 256): 768}        # workgroups of a fused launch
STEM_CAP, POOL_CAP, POOL4_CAP, U8_CAP = 768, 8192, 16384, 4096

# ------------------------------------------------------------------------------------------------------------ cases
# entry: which C entry point (ENTRY_POINT);  imgs > DISTINCT: a cycled batch;  ldo > O: a window, 4 columns in, of a wider buffer
# (channel-blocked entries: rows_total = rows + 5 instead)
Fused = namedtuple('Fused', 'entry W H O ldo imgs')
Stem = namedtuple('Stem', 'imgs Cin H W O ldc KH KW stride pad')
# off: '' or the one part of the 16-byte condition that is broken by a pointer offset ('in', 'out', 'scale', 'shift': one float;
# 'amax': one byte)
Pool = namedtuple('Pool', 'imgs C Hi Wi ldi ldo argmax off')
# entry: f32 | idx | h16 | h16_cb;  extra: rows of the buffer beyond imgs * S2 (h16_cb), rows of out beyond imgs (idx)
Avg = namedtuple('Avg', 'entry imgs C S2 ldi ldo extra')
U8 = namedtuple('U8', 'imgs C H W norm')

ENTRY_POINT = {
    'f32': 'gnx_conv_stem_bnrelu_maxpool', 'idx': 'gnx_conv_stem_bnrelu_maxpool_idx',
    'argmax': 'gnx_conv_stem_bnrelu_maxpool_argmax', 'h16': 'gnx_conv_stem_bnrelu_maxpool_h16',
    'u8': 'gnx_conv_stem_bnrelu_maxpool_u8', 'u8_h16': 'gnx_conv_stem_bnrelu_maxpool_u8',
    'u8_idx': 'gnx_conv_stem_bnrelu_maxpool_u8_idx', 'f16mul': 'gnx_conv_stem_bnrelu_maxpool_f16mul',
    'f16mul_u8': 'gnx_conv_stem_bnrelu_maxpool_f16mul', 'cb': 'gnx_conv_stem_bnrelu_maxpool_f16mul_cb',
    'cb_u8': 'gnx_conv_stem_bnrelu_maxpool_f16mul_cb'}
FUSED_ENTRIES = tuple(ENTRY_POINT)
IS_U8 = {'u8', 'u8_h16', 'u8_idx', 'f16mul_u8', 'cb_u8'}
IS_F16MUL = {'f16mul', 'f16mul_u8', 'cb', 'cb_u8'}
IS_H16 = {'h16', 'u8_h16'} | IS_F16MUL
IS_IDX = {'idx', 'u8_idx'}
IS_CB = {'cb', 'cb_u8'}
# the entry whose output an entry must reproduce bit for bit (on the gathered / torch-converted patches, re-laid / .half())
COUNTERPART = {'idx': 'f32', 'argmax': 'f32', 'h16': 'f32', 'u8': 'f32', 'u8_h16': 'h16', 'u8_idx': 'idx', 'f16mul_u8': 'f16mul',
               'cb': 'f16mul', 'cb_u8': 'cb'}

FORMS = (['stem.generic', 'stem.patch7', 'stem.patch3']
         + ['fused.%d.%s' % (wo, f) for wo in (64, 128) for f in ('f32.float.plain', 'f32.float.idx', 'f32.float.argmax',
                                                                  'f32.u8.plain', 'f32.u8.idx', 'h16.float.plain', 'h16.u8.plain')]
         + ['fused16.%d.%s.%s' % (wo, x, o) for wo in (64, 128) for x in ('float', 'u8') for o in ('rows', 'cb')]
         + ['maxpool.%s.%s' % (v, a) for v in ('scalar', 'vec4') for a in ('plain', 'argmax')]
         + ['avgpool.f32', 'avgpool.idx', 'avgpool.h16', 'avgpool.h16_cb', 'u8_to_f32'])
REFUSED = ('unsupported', 'bad_arg')
EMPTY = 'empty'                  # imgs == 0: GNX_OK and nothing launched (not a kernel form)


def ids(c):
    return type(c).__name__.lower() + '-' + '-'.join(str(v) for v in c)


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def pooled(n):
    return (n + 2 - 3) // 2 + 1


def fused_sizes(c):
    """(Ho, Wo, Hp, Wp): the conv0 map and the pooled map of a fused case."""
    ho, wo = conv_out(c.H, 7, 2, 3), conv_out(c.W, 7, 2, 3)
    return ho, wo, pooled(ho), pooled(wo)


def distinct(c):
    return min(c.imgs, DISTINCT) if c.entry not in IS_IDX else (3 if c.imgs <= 5 else DISTINCT)      # idx: the patches x holds


def src_list(c):
    """The index list of an _idx case: c.imgs entries over `distinct(c)` patches, with repeats and with entries below 0 and at
    or above src_imgs (which the kernel clamps into the range)."""
    d = distinct(c)
    lst = [(5 * i + 3) % d for i in range(c.imgs)]
    for at, v in ((0, -1), (1, d), (c.imgs // 2, -7), (c.imgs - 1, d + 93)):
        if at < c.imgs and c.imgs >= 3:
            lst[at] = v
    return lst


def image_map(c):
    """Per output image, which of the case's distinct patches it shows (the clamp of an index list applied)."""
    d = distinct(c)
    if c.entry in IS_IDX:
        return [min(max(v, 0), d - 1) for v in src_list(c)]
    return [i % d for i in range(c.imgs)]


def rows_total(c):
    _, _, hp, wp = fused_sizes(c)
    return c.imgs * hp * wp + (5 if c.ldo > c.O else 0)


# ------------------------------------------------------------------------------------------------------------ the dispatch mirror
def _al(a, name, mask):
    return (a[name] & mask) == 0


def _null(a, *names):
    return any(a[n] is None for n in names)


def _stem_pool(a, h16, u8, amax=False, idx=False):
    if _null(a, 'x', 'w', 'out', 'scale', 'shift') or a['imgs'] < 0 or a['Cin'] <= 0 or a['O'] <= 0 or a['H'] <= 0 or a['W'] <= 0 \
            or a['ldo'] < a['O']:
        return 'bad_arg'
    if idx and a['src_imgs'] <= 0:
        return 'bad_arg'
    if amax and not _al(a, 'amax', 3):
        return 'unsupported'
    if (a['Cin'], a['KH'], a['KW'], a['stride'], a['pad']) != (3, 7, 7, 2, 3) or a['O'] > 64 or a['O'] % 4 or a['ldo'] % 4 \
            or not _al(a, 'out', 7 if h16 else 15):
        return 'unsupported'
    ho, wo = (a['H'] - 1) // 2 + 1, (a['W'] - 1) // 2 + 1
    if wo not in (64, 128) or a['W'] != 2 * wo or ho % 2 or not _al(a, 'x', 3 if u8 else 15):
        return 'unsupported'
    if a['imgs'] == 0:
        return EMPTY
    return 'fused.%d.%s.%s.%s' % (wo, 'h16' if h16 else 'f32', 'u8' if u8 else 'float', 'argmax' if amax else 'idx' if idx else 'plain')


def _stem_pool_f16(a, u8, cb):
    ldo = 32 if cb else a['ldo']
    if cb:
        if a['rows_total'] <= 0 or a['O'] % 32:
            return 'bad_arg'
        if a['imgs'] > 0 and a['H'] > 0 and a['W'] > 0:
            hp, wp = ((a['H'] - 1) // 2 + 1) // 2, ((a['W'] - 1) // 2 + 1) // 2
            if hp > 0 and wp > 0 and a['rows_total'] < a['imgs'] * hp * wp:
                return 'bad_arg'
    if not u8 and a['norm'] is not None:
        return 'bad_arg'
    if _null(a, 'x', 'w', 'out', 'scale', 'shift') or a['imgs'] < 0 or a['Cin'] <= 0 or a['O'] <= 0 or a['H'] <= 0 or a['W'] <= 0 \
            or (not cb and ldo < a['O']):
        return 'bad_arg'
    if (a['Cin'], a['KH'], a['KW'], a['stride'], a['pad']) != (3, 7, 7, 2, 3) or a['O'] > 64 or a['O'] % 4 or ldo % 4 \
            or not _al(a, 'out', 7):
        return 'unsupported'
    ho, wo = (a['H'] - 1) // 2 + 1, (a['W'] - 1) // 2 + 1
    if wo not in (64, 128) or a['W'] != 2 * wo or ho % 2 or not _al(a, 'x', 3 if u8 else 15):
        return 'unsupported'
    if a['imgs'] == 0:
        return EMPTY
    return 'fused16.%d.%s.%s' % (wo, 'u8' if u8 else 'float', 'cb' if cb else 'rows')


def _conv_stem(a):
    if _null(a, 'x', 'w', 'out') or a['imgs'] < 0 or a['Cin'] <= 0 or a['O'] <= 0 or not 0 < a['KH'] <= 7 or not 0 < a['KW'] <= 8 \
            or a['stride'] <= 0 or a['ldc'] < a['O']:
        return 'bad_arg'
    ho, wo = _cdiv_trunc(a['H'] + 2 * a['pad'] - a['KH'], a['stride']) + 1, _cdiv_trunc(a['W'] + 2 * a['pad'] - a['KW'], a['stride']) + 1
    if ho <= 0 or wo <= 0:
        return 'bad_arg'
    if a['imgs'] == 0:
        return EMPTY
    if a['O'] <= 64 and a['Cin'] == 3:
        if (a['stride'], a['KH'], a['KW']) == (2, 7, 7):
            return 'stem.patch7'
        if (a['stride'], a['KH'], a['KW']) == (1, 3, 3):
            return 'stem.patch3'
    return 'stem.generic'


def _cdiv_trunc(n, d):
    """C's integer division (towards zero)."""
    q = abs(n) // d
    return q if n >= 0 else -q


def _maxpool(a, amax):
    if amax and a['amax'] is None:
        return 'bad_arg'
    if _null(a, 'in', 'out', 'scale', 'shift') or a['imgs'] < 0 or a['C'] <= 0 or a['Hi'] <= 0 or a['Wi'] <= 0 or a['ldi'] < a['C'] \
            or a['ldo'] < a['C']:
        return 'bad_arg'
    if a['imgs'] == 0:
        return EMPTY
    vec = a['C'] % 4 == 0 and a['ldi'] % 4 == 0 and a['ldo'] % 4 == 0 and all(_al(a, n, 15) for n in ('in', 'out', 'scale', 'shift')) \
        and (not amax or _al(a, 'amax', 3))
    return 'maxpool.%s.%s' % ('vec4' if vec else 'scalar', 'argmax' if amax else 'plain')


def _avgpool(a, entry):
    cb = entry == 'h16_cb'
    if _null(a, 'in', 'out', 'scale', 'shift') or a['imgs'] < 0 or a['C'] <= 0 or a['S2'] <= 0 or a['ldo'] < a['C']:
        return 'bad_arg'
    if cb and (a['rows_total'] < a['imgs'] * a['S2'] or a['C'] % 32):
        return 'bad_arg'
    if not cb and a['ldi'] < a['C']:
        return 'bad_arg'
    if entry == 'idx' and (a['idx'] is None or a['dst_rows'] <= 0):
        return 'bad_arg'
    if a['imgs'] == 0:
        return EMPTY
    return 'unsupported' if a['imgs'] > 2147483647 else 'avgpool.' + entry


def _u8(a):
    if _null(a, 'x', 'out') or a['imgs'] < 0 or a['C'] <= 0 or a['H'] <= 0 or a['W'] <= 0 or (a['norm'] is not None and a['C'] != 3):
        return 'bad_arg'
    if a['H'] * a['W'] % 4 or not _al(a, 'x', 3) or not _al(a, 'out', 15):
        return 'unsupported'
    return EMPTY if a['imgs'] == 0 else 'u8_to_f32'


def form_of_call(entry, a):
    """The kernel instance (a name of FORMS), 'unsupported', 'bad_arg' or EMPTY that the launcher of `entry` answers a call with,
    written from the launchers' conditions.  `a`: the call's scalars by name; a pointer is its byte offset from a 16-B
    boundary, or None for NULL."""
    if entry in ('f32', 'h16'):
        return _stem_pool(a, entry == 'h16', False)
    if entry == 'argmax':
        return 'bad_arg' if a['amax'] is None else _stem_pool(a, False, False, amax=True)
    if entry in ('idx', 'u8_idx'):
        return 'bad_arg' if a['idx'] is None else _stem_pool(a, False, entry == 'u8_idx', idx=True)
    if entry in ('u8', 'u8_h16'):
        return _stem_pool(a, entry == 'u8_h16', True)
    if entry in IS_F16MUL:
        return _stem_pool_f16(a, entry in IS_U8, entry in IS_CB)
    if entry == 'conv_stem':
        return _conv_stem(a)
    if entry in ('maxpool', 'maxpool_argmax'):
        return _maxpool(a, entry == 'maxpool_argmax')
    if entry.startswith('avgpool.'):
        return _avgpool(a, entry[8:])
    if entry == 'u8_to_f32':
        return _u8(a)
    raise KeyError(entry)


def call_of(c):
    """(entry, arguments) of a case of GRID as form_of_call takes them."""
    if isinstance(c, Fused):
        a = dict(x=0, w=0, out=0, scale=0, shift=0, norm=0 if c.entry in IS_U8 else None, amax=0, idx=0, imgs=c.imgs, Cin=3, H=c.H,
                 W=c.W, O=c.O, KH=7, KW=7, stride=2, pad=3, ldo=c.ldo, src_imgs=distinct(c), rows_total=rows_total(c))
        return c.entry, a
    if isinstance(c, Stem):
        return 'conv_stem', dict(c._asdict(), x=0, w=0, out=0)
    if isinstance(c, Pool):
        a = dict(c._asdict(), scale=0, shift=0, amax=0 if c.argmax else None, out=0)
        a['in'] = 0
        if c.off:
            a[c.off] = 1 if c.off == 'amax' else 4
        return ('maxpool_argmax' if c.argmax else 'maxpool'), a
    if isinstance(c, Avg):
        a = dict(c._asdict(), scale=0, shift=0, out=0, idx=0, dst_rows=c.imgs + c.extra, rows_total=c.imgs * c.S2 + c.extra)
        a['in'] = 0
        return 'avgpool.' + c.entry, a
    if isinstance(c, U8):
        return 'u8_to_f32', dict(x=0, out=0, imgs=c.imgs, C=c.C, H=c.H, W=c.W, norm=0 if c.norm else None)
    raise TypeError(c)


def form_of(c):
    """The name of the kernel instance that the launchers in stem_pool.hip pick for a case."""
    return form_of_call(*call_of(c))


# ------------------------------------------------------------------------------------------------------------ the queries
# The library's own statement of the dispatch: gnx_conv_stem_form, gnx_conv_stem_pool_form, gnx_conv_stem_pool_f16mul_form and
# gnx_bnrelu_maxpool_form return the launcher's plan without launching.  A query sees the launch arguments only, so the one
# condition an entry point checks on its own (a NULL src_idx / argmax; rows_total == 0 of the channel-blocked entry, which the
# query reads as the row-major entry) is not the query's to answer: it then answers for the entry it is left with.
POINTERS = ('x', 'w', 'in', 'out', 'scale', 'shift', 'norm', 'amax', 'idx')
ERROR_CODE = {'bad_arg': 'GNX_ERR_BAD_ARG', 'unsupported': 'GNX_ERR_UNSUPPORTED'}
FIRST_CODE = {'gnx_conv_stem_form': 'GNX_STEM_GENERIC', 'gnx_conv_stem_pool_form': 'GNX_SP_64',
              'gnx_conv_stem_pool_f16mul_form': 'GNX_SP16_64', 'gnx_bnrelu_maxpool_form': 'GNX_MP_SCALAR'}
QUERY_CODES = ('GNX_STEM_GENERIC', 'GNX_STEM_PATCH7', 'GNX_STEM_PATCH3', 'GNX_SP_64', 'GNX_SP_128', 'GNX_SP16_64', 'GNX_SP16_128',
               'GNX_MP_SCALAR', 'GNX_MP_VEC4')


def query_call(entry, a, P):
    """(the query's name, its arguments in front of `workgroups`) for the call `entry` with the scalars `a` and the pointers `P`
    (by name; None: NULL) - which setting of a query's flags is which entry point; None: the entry has one body and no query."""
    if entry in FUSED_ENTRIES:
        geo = (a['imgs'], a['Cin'], a['H'], a['W'], a['O'], a['KH'], a['KW'], a['stride'], a['pad'], P['scale'], P['shift'])
        if entry in IS_F16MUL:
            ld = (0, a['rows_total']) if entry in IS_CB else (a['ldo'], 0)
            return 'gnx_conv_stem_pool_f16mul_form', (P['x'], int(entry in IS_U8), P['w'], P['out']) + ld + geo + (P['norm'],)
        tail = (P['amax'] if entry == 'argmax' else None,) + ((P['idx'], a['src_imgs']) if entry in IS_IDX else (None, 0))
        return 'gnx_conv_stem_pool_form', (P['x'], int(entry in IS_U8), P['w'], P['out'], int(entry in IS_H16), a['ldo']) + geo + tail
    if entry == 'conv_stem':
        return 'gnx_conv_stem_form', (P['x'], P['w'], P['out'], a['ldc'], a['imgs'], a['Cin'], a['H'], a['W'], a['O'], a['KH'], a['KW'],
                                      a['stride'], a['pad'])
    if entry in ('maxpool', 'maxpool_argmax'):
        return 'gnx_bnrelu_maxpool_form', (P['in'], a['ldi'], P['out'], a['ldo'], P['amax'] if entry == 'maxpool_argmax' else None,
                                           a['imgs'], a['C'], a['Hi'], a['Wi'], P['scale'], P['shift'])
    return None


def _cdiv(n, d):
    return -(-n // d)


def query_answer(entry, a):
    """(the GNX_* constant's name, *workgroups) that the query of query_call answers with; `a` as form_of_call takes it.  The
    workgroups are the grid's x size: a row of tiles (gnx_conv_stem's generic form), else the items up to the launch's cap."""
    name = query_call(entry, a, dict.fromkeys(POINTERS))[0]
    if entry in IS_IDX and a['idx'] is None:
        entry = 'u8' if entry == 'u8_idx' else 'f32'
    elif entry in ('argmax', 'maxpool_argmax') and a['amax'] is None:
        entry = 'f32' if entry == 'argmax' else 'maxpool'
    elif entry in IS_CB and a['rows_total'] == 0:
        entry, a = ('f16mul_u8' if entry == 'cb_u8' else 'f16mul'), dict(a, ldo=0)
    f = form_of_call(entry, a)
    if f in ERROR_CODE:
        return ERROR_CODE[f], 0
    if f == EMPTY:
        return FIRST_CODE[name], 0
    kind = f.split('.')
    if kind[0] == 'stem':
        ho, wo = conv_out(a['H'], a['KH'], a['stride'], a['pad']), conv_out(a['W'], a['KW'], a['stride'], a['pad'])
        if kind[1] == 'generic':
            return 'GNX_STEM_GENERIC', _cdiv(a['imgs'] * ho * wo, 128)
        return 'GNX_STEM_' + kind[1].upper(), min(a['imgs'] * _cdiv(ho, 8) * _cdiv(wo, 16), STEM_CAP)
    if kind[0] in ('fused', 'fused16'):
        f16 = kind[0] == 'fused16'
        return 'GNX_SP%s_%s' % ('16' if f16 else '', kind[1]), min(a['imgs'], CAP['f16' if f16 else 'f32', a['W']])
    assert kind[0] == 'maxpool'
    items = a['imgs'] * pooled(a['Hi']) * pooled(a['Wi']) * a['C']
    if kind[1] == 'vec4':
        return 'GNX_MP_VEC4', min(_cdiv(items // 4, 256), POOL4_CAP)
    return 'GNX_MP_SCALAR', min(_cdiv(items, 256), POOL_CAP)


# ------------------------------------------------------------------------------------------------------------ GRID
FUSED_H = {128: (3, 4, 7, 8, 16, 36), 256: (3, 4, 7, 8, 16)}       # Ho = 2, 2, 4, 4, 8, 18: one tile with both edges in one window,
# odd H, every slot of the fp16 kernel's ring of 9 (7) rows: nine tiles at 128 wide (H = 36), sixteen at 256 wide (H = 16)


def _fused_grid():
    g = []
    for e in FUSED_ENTRIES:
        cb, n3 = e in IS_CB, 5 if e in IS_IDX else 3               # (an index list: 5 entries over 3 patches)
        for W in (128, 256):
            for k, H in enumerate(FUSED_H[W]):
                g.append(Fused(e, W, H, 64, 64 if (cb or k % 2 == 0) else 72, n3))
                g.append(Fused(e, W, H, 64, 72 if k % 2 == 0 else 64, 1))
            for O in ((32,) if cb else (4, 36)):                   # (the channel-blocked layout needs 32 | O)
                g += [Fused(e, W, 7, O, O, n3), Fused(e, W, 8, O, O + 8, 1), Fused(e, W, 16, O, O + 8, n3)]
    # the shipping geometry; three more images (index-list entries) than the launch's workgroups, at H == 8
    g += [Fused('f32', 128, 128, 64, 64, 1), Fused('f32', 256, 256, 64, 64, 1), Fused('f16mul', 128, 128, 64, 64, 1),
          Fused('f16mul', 256, 256, 64, 64, 1)]
    for W in (128, 256):
        g += [Fused(e, W, 8, 64, 64, CAP['f32', W] + 3) for e in ('f32', 'idx', 'u8_idx', 'argmax')]
        g += [Fused(e, W, 8, 64, 64, CAP['f16', W] + 3) for e in ('f16mul', 'cb_u8')]
    return g


def _stem_grid():
    g = []
    for O, ldc in ((8, 12), (10, 11), (33, 40), (64, 66)):                         # patch forms: ldc > O
        g += [Stem(2, 3, 20, 44, O, ldc, 7, 7, 2, 3),                              # 10 x 22 map: ragged 8 x 16 tiles both ways
              Stem(2, 3, 11, 19, O, ldc, 3, 3, 1, 1)]                              # 11 x 19
    g += [Stem(1, 3, 21, 39, 64, 64, 7, 7, 2, 0), Stem(1, 3, 10, 18, 33, 40, 3, 3, 1, 0),      # pad 0
          Stem(1, 3, 16, 32, 8, 8, 7, 7, 2, 3), Stem(3, 3, 8, 16, 64, 64, 3, 3, 1, 1),         # whole tiles
          Stem(STEM_CAP + 2, 3, 16, 16, 64, 64, 7, 7, 2, 3), Stem(STEM_CAP // 2 + 1, 3, 16, 16, 10, 12, 3, 3, 1, 1)]  # > 768 tiles
    g += [Stem(2, 3, 16, 16, 65, 65, 7, 7, 2, 3), Stem(2, 3, 20, 44, 96, 100, 7, 7, 2, 3),     # generic: a 96-channel stem, grid.y = 2
          Stem(2, 1, 9, 13, 8, 8, 3, 3, 1, 1), Stem(2, 4, 9, 13, 10, 12, 3, 3, 1, 1),          # Cin 1, 4
          Stem(2, 3, 12, 15, 16, 16, 5, 3, 1, 1), Stem(2, 2, 9, 20, 64, 64, 2, 8, 1, 3),       # KH != KW; KW == 8: every kx slot live
          Stem(2, 3, 17, 23, 33, 33, 3, 3, 3, 0), Stem(1, 3, 16, 16, 64, 64, 7, 7, 1, 3),      # stride 3 pad 0; 7x7 s1 (not a patch form)
          Stem(1, 3, 7, 18, 8, 8, 1, 1, 1, 0), Stem(1, 3, 8, 16, 8, 8, 1, 1, 1, 0),            # M = 126, 128, 129, 257
          Stem(1, 3, 3, 43, 8, 8, 1, 1, 1, 0), Stem(1, 3, 1, 257, 70, 70, 1, 1, 1, 0)]
    return g


def _pool_grid():
    g = []
    for am in (0, 1):
        g += [Pool(2, 1, 1, 5, 3, 2, am, ''), Pool(2, 6, 7, 4, 9, 6, am, ''), Pool(3, 8, 5, 9, 8, 12, am, ''),
              Pool(2, 64, 6, 3, 68, 64, am, ''), Pool(2, 8, 1, 1, 8, 8, am, '')]
        # the 16-byte condition, each part broken alone (C % 4; ldi % 4; ldo % 4; a pointer one float / argmax one byte off)
        g += [Pool(2, 6, 5, 9, 8, 8, am, ''), Pool(2, 8, 5, 9, 9, 8, am, ''), Pool(2, 8, 5, 9, 8, 9, am, '')]
        g += [Pool(2, 8, 5, 9, 8, 8, am, off) for off in ('in', 'out', 'scale', 'shift')]
        # just above the block caps, at Hi == 2, Wi == 3 (2 pooled positions per image)
        g += [Pool(POOL_CAP * 256 // 2 + 3, 1, 2, 3, 1, 1, am, ''), Pool(POOL4_CAP * 256 // 4 + 3, 8, 2, 3, 8, 8, am, '')]
    g.append(Pool(2, 8, 5, 9, 8, 8, 1, 'amax'))
    return g


def _avg_grid():
    g = []
    for S2 in (1, 3, 4, 5, 49, 1024):
        for C in (1, 63, 64, 65, 130):
            g += [Avg('f32', 3, C, S2, C + 3, C + (S2 & 1), 0), Avg('idx', 5, C, S2, C + 1, C + 2, 2), Avg('h16', 3, C, S2, C + 2, C, 0)]
        g += [Avg('h16_cb', 3, C, S2, 32, C + 1, extra) for C, extra in ((64, 0), (64, 7), (96, 3))]
    return g


def _u8_grid():
    g = [U8(imgs, C, H, W, norm) for imgs, C, H, W in ((3, 3, 6, 10), (2, 1, 2, 2), (3, 4, 5, 4), (5, 3, 16, 16)) for norm in (0, 1)
         if not (norm and C != 3)]
    return g + [U8(U8_CAP * 256 * 4 // (3 * 256) + 3, 3, 16, 16, 1)]               # more 4-pixel items than 4096 blocks of 256


GRID = _fused_grid() + _stem_grid() + _pool_grid() + _avg_grid() + _u8_grid()


def avg_dst(c):
    """dst_idx of an avgpool idx case: a permutation of the rows of out [imgs + extra], two entries out of range."""
    n, rows = c.imgs, c.imgs + c.extra
    lst = [(3 * i + 1) % rows for i in range(n)]
    lst[1], lst[n - 1] = -1, rows
    return lst


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def signed(g, lo, hi, *shape):
    """float32 values with a magnitude in [lo, hi] and a random sign."""
    u = torch.rand(*shape, generator=g, dtype=torch.float32)
    s = torch.randint(0, 2, shape, generator=g, dtype=torch.int8)
    return u.mul_(hi - lo).add_(lo).clamp_(lo, hi).mul_(s.float().mul_(2).sub_(1))


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def bn(g, kind, C):
    """(scale, shift) float32 [C] of a kind."""
    if kind == 'int':
        return torch.tensor([1.0, -1.0, 0.5, 2.0])[torch.randint(0, 4, (C,), generator=g)], ints(g, -8, 8, C)
    return signed(g, 0.25, 0.75, C), torch.rand(C, generator=g) * 4 + 2


def norm_vector():
    """{mean[3], std[3], 1 / std[3]} float32, as the model builds it for the uint8 entry points."""
    m, sd = torch.tensor(MEAN, dtype=torch.float32), torch.tensor(STD, dtype=torch.float32)
    return torch.cat([m, sd, 1.0 / sd])


def to_tensor(x8, norm):
    """torchvision's ToTensor (+ Normalize) of uint8 [n][C][H][W], in float32 as torch does it."""
    v = x8.to(torch.float32).div(255)
    if norm:
        v = v.sub(torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)).div(torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1))
    return v


# kind 1 must make every position of the conv0 map a recorded winner at O == 64 (asserted on the host): with 64 channels a position
# that lies in one window only is missed with probability (8 / 9)^64 = 5e-4, a few tenths per geometry - those get another seed
INT_SALT = {(128, 7, 3): 1, (128, 8, 3): 1, (128, 36, 3): 4, (256, 8, 3): 1, (256, 16, 3): 5}        # (W, H, patches) -> salt


@functools.lru_cache(maxsize=8)
def _fused_inputs(u8, W, H, O, d, kind):
    g = _gen('fused', u8, W, H, O, d, kind, *([INT_SALT[W, H, d]] if kind == 'int' and not u8 and (W, H, d) in INT_SALT else []))
    if u8:
        x = (torch.randint(0, 2, (d, 3, H, W), generator=g) * 255 if kind == 'int'
             else torch.randint(0, 256, (d, 3, H, W), generator=g)).to(torch.uint8)
    else:
        x = ints(g, -2, 2, d, 3, H, W) if kind == 'int' else signed(g, 0.5, 1.5, d, 3, H, W)
    w = ints(g, -2, 2, O, 3, 7, 7) if kind == 'int' else signed(g, 0.5, 1.5, O, 3, 7, 7)
    scale, shift = bn(g, kind, O)
    return NS(x=x, w=w, scale=scale, shift=shift, norm=bool(u8 and kind == 'mag'))


def fused_inputs(c, kind):
    """The operands of a fused case (shared: do not write to them): x [distinct(c)][3][H][W] float32 or uint8, w [O][3][7][7],
    scale, shift [O]; norm: whether the uint8 patches go through Normalize."""
    return _fused_inputs(c.entry in IS_U8, c.W, c.H, c.O, distinct(c), kind)


def fused_floats(c, kind):
    """The float32 patches the convolution of a case sees (uint8: torch's conversion)."""
    r = fused_inputs(c, kind)
    return to_tensor(r.x, r.norm) if c.entry in IS_U8 else r.x


# ------------------------------------------------------------------------------------------------------------ references
def conv(x, w, stride, pad, dy=0, dx=0, twice=None, edge=False, padval=None):
    """The convolution from its definition, one tap (c, ky, kx) after the other, in the operands' dtype (float64: the reference;
    float32: the sequential multiply-add chain, one rounding for the product and one for the sum).  x [n][Cin][H][W], w [O][Cin]
    [KH][KW] -> [n][O][Ho][Wo].  Wrong variants: dy, dx: the window one row / column off; twice = (c, ky): that group of taps counted
    twice; edge: the border pixel instead of the zero padding; padval [Cin]: that value instead."""
    n, cin, H, W = x.shape
    O, _, KH, KW = w.shape
    ho, wo = conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad)
    m, far = pad + 1, pad + 1 + stride + max(KH, KW)
    if edge:
        xp = F.pad(x, (m, far, m, far), mode='replicate')
    else:
        xp = torch.zeros(n, cin, H + m + far, W + m + far, dtype=x.dtype)
        if padval is not None:
            xp += padval.to(x.dtype).view(1, cin, 1, 1)
        xp[:, :, m:m + H, m:m + W] = x
    acc = torch.zeros(n, O, ho, wo, dtype=x.dtype)
    for c in range(cin):
        for ky in range(KH):
            for kx in range(KW):
                y0, x0 = 1 + dy + ky, 1 + dx + kx
                win = xp[:, c, y0:y0 + stride * (ho - 1) + 1:stride, x0:x0 + stride * (wo - 1) + 1:stride]
                term = win[:, None] * w[:, c, ky, kx].view(1, O, 1, 1)
                acc = acc + term
                if twice == (c, ky):
                    acc = acc + term
    return acc


def act(pre, scale, shift):
    return (pre * scale.to(pre.dtype).view(1, -1, 1, 1) + shift.to(pre.dtype).view(1, -1, 1, 1)).clamp_min(0)


def _windows(m, fill):
    """[9][n][C][Ho][Wo]: the 3x3 s2 p1 window elements in row-major order, `fill` where the window leaves the map."""
    n, C, hi, wi = m.shape
    ho, wo = pooled(hi), pooled(wi)
    p = torch.full((n, C, 2 * ho + 1, 2 * wo + 1), fill, dtype=m.dtype)
    p[:, :, 1:1 + hi, 1:1 + wi] = m
    return p, [(k // 3, k % 3) for k in range(9)], ho, wo


def maxpool(a, tol=None, ge=False, carry=False):
    """3x3 s2 p1 max pool of a [n][C][Hi][Wi] (>= 0) by the scan of the definition.  NS(val, idx [n][C][Ho][Wo]; with tol (the
    elements' tolerances): tol, the largest of each window, and comparable, where the two largest window values differ by more
    than the sum of their tolerances).  Wrong variants: ge: the LAST maximal element; carry: row -1 of an image is the previous
    image's last row (a carry that is not reset)."""
    NEG = float('-inf')
    p, taps, ho, wo = _windows(a, NEG)
    if carry:
        p[1:, :, 0, 1:1 + a.shape[3]] = a[:-1, :, -1, :]
    vals = torch.stack([p[:, :, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] for dy, dx in taps])
    best = torch.full_like(vals[0], NEG)
    idx = torch.zeros(vals[0].shape, dtype=torch.int64)
    for k in range(9):
        better = ((vals[k] >= best) if ge else (vals[k] > best)) & (vals[k] > NEG)
        best = torch.where(better, vals[k], best)
        idx = torch.where(better, k, idx)
    out = NS(val=best, idx=idx)
    if tol is not None:
        tp, _, _, _ = _windows(tol, 0.0)
        tols = torch.stack([tp[:, :, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] for dy, dx in taps])
        out.tol = tols.max(0).values
        tv, ti = vals.topk(2, dim=0)
        tt = tols.gather(0, ti)
        out.comparable = (tv[0] - tv[1]) > (tt[0] + tt[1])
    return out


def as_rows(m):
    """NCHW [n][C][H][W] -> rows [n H W][C]."""
    return m.permute(0, 2, 3, 1).reshape(-1, m.shape[1])


def as_map(rows, n, H, W):
    """rows [n H W][C] -> NCHW [n][C][H][W]."""
    return rows.reshape(n, H, W, -1).permute(0, 3, 1, 2)


def half_round(t):
    """The operand rounding of the fp16-operand stem."""
    return t.half().to(t.dtype)


def fused_operands(c, kind):
    """(x, w) float64 as the convolution of the entry multiplies them."""
    x, w = fused_floats(c, kind).double(), fused_inputs(c, kind).w.double()
    return (half_round(x), half_round(w)) if c.entry in IS_F16MUL else (x, w)


def fused_eval(c, kind, g=None, **wrong):
    """The fused stem of a case's distinct patches in float64: NS(val, tol, idx, comparable), each [d][Hp][Wp][O] (rows of an
    image in (y, x) order); tol includes the fp16 store's share for the entries that store fp16.  `wrong`: the variants of
    conv / maxpool."""
    r = fused_inputs(c, kind)
    x, w = fused_operands(c, kind)
    cw = {k: v for k, v in wrong.items() if k in ('dy', 'dx', 'twice', 'edge', 'padval')}
    pw = {k: v for k, v in wrong.items() if k in ('ge', 'carry')}
    pre = conv(x, w, 2, 3, **cw)
    T = conv(x.abs(), w.abs(), 2, 3)
    a = act(pre, r.scale.double(), r.shift.double())
    t = r.scale.double().abs().view(1, -1, 1, 1) * (G if g is None else g) * U * T + U * a
    p = maxpool(a, t, **pw)
    if c.entry in IS_H16:
        p.tol = p.tol + 2.0 ** -11 * p.val.abs() + 2.0 ** -25
    nhwc = lambda m: m.permute(0, 2, 3, 1).contiguous()
    return NS(val=nhwc(p.val), tol=nhwc(p.tol), idx=nhwc(p.idx), comparable=nhwc(p.comparable), pre=pre, T=T)


@functools.lru_cache(maxsize=4)
def _fused_reference(key, kind):
    return fused_eval(Fused(*key), kind)


def fused_reference(c, kind):
    """fused_eval of a case, shared among the cases with the same operands (do not write to it)."""
    rep = 'f16mul' if c.entry in ('f16mul', 'cb') else 'f16mul_u8' if c.entry in IS_F16MUL else \
        'u8_h16' if c.entry == 'u8_h16' else 'u8' if c.entry in IS_U8 else 'h16' if c.entry == 'h16' else 'f32'
    d = distinct(c)
    return _fused_reference((rep, c.W, c.H, c.O, c.O, d), kind)


def stem_inputs(c, kind):
    g = _gen('stem', c.Cin, c.H, c.W, c.O, c.KH, c.KW, kind)
    d = min(c.imgs, DISTINCT)
    mk = (lambda *s: ints(g, -2, 2, *s)) if kind == 'int' else (lambda *s: signed(g, 0.5, 1.5, *s))
    return NS(x=mk(d, c.Cin, c.H, c.W), w=mk(c.O, c.Cin, c.KH, c.KW))


def stem_reference(c, kind, g=None):
    """gnx_conv_stem of a case's distinct images: NS(val, tol [d Ho Wo][O] float64, T)."""
    r = stem_inputs(c, kind)
    T = conv(r.x.double().abs(), r.w.double().abs(), c.stride, c.pad)
    return NS(val=as_rows(conv(r.x.double(), r.w.double(), c.stride, c.pad)), tol=as_rows((G if g is None else g) * U * T), T=T)


def pool_inputs(c, kind):
    g = _gen('pool', c.C, c.Hi, c.Wi, kind)
    d = min(c.imgs, DISTINCT)
    x = ints(g, -2, 2, d, c.C, c.Hi, c.Wi) if kind == 'int' else signed(g, 0.5, 1.5, d, c.C, c.Hi, c.Wi)
    scale, shift = bn(g, kind, c.C)
    if kind == 'mag':
        shift = shift * 0.25                               # |x scale| <= 1.125: keep about a quarter of the map under the ReLU
    return NS(x=x, scale=scale, shift=shift)


def pool_reference(c, kind):
    """gnx_bnrelu_maxpool(_argmax) of a case's distinct images: NS(val, tol, idx, comparable) [d][Ho][Wo][C]."""
    r = pool_inputs(c, kind)
    a = act(r.x.double(), r.scale.double(), r.shift.double())
    p = maxpool(a, U * a)
    nhwc = lambda m: m.permute(0, 2, 3, 1).contiguous()
    return NS(val=nhwc(p.val), tol=nhwc(p.tol), idx=nhwc(p.idx), comparable=nhwc(p.comparable))


def avg_inputs(c, kind):
    g = _gen('avg', c.entry, c.C, c.S2, c.imgs, kind)
    x = ints(g, -2, 2, c.imgs * c.S2, c.C) if kind == 'int' else signed(g, 0.5, 1.5, c.imgs * c.S2, c.C)
    if c.entry in ('h16', 'h16_cb'):
        x = half_round(x)
    scale, shift = bn(g, kind, c.C)
    return NS(x=x, scale=scale, shift=shift * (1.0 if kind == 'int' else 0.25))


def avg_reference(c, kind):
    """The BN + ReLU + global average pool of a case: NS(val, tol [imgs][C])."""
    r = avg_inputs(c, kind)
    a = (r.x.double() * r.scale.double() + r.shift.double()).clamp_min(0).view(c.imgs, c.S2, c.C)
    val = a.sum(1) / c.S2
    return NS(val=val, tol=(-(-c.S2 // 4) + 4) * U * val)


# ------------------------------------------------------------------------------------------------------------ layouts
def to_ld(rows, ld, col0, fill=float('nan')):
    """rows [M][C] as the window [:, col0 : col0 + C] of a `fill`-ed [M][ld] matrix."""
    out = torch.full((rows.shape[0], ld), fill, dtype=rows.dtype)
    out[:, col0:col0 + rows.shape[1]] = rows
    return out


def from_ld(buf, C, col0):
    return buf[:, col0:col0 + C]


def to_cb(rows, total, fill=float('nan'), block=None):
    """rows [M][C] (32 | C) -> the channel-blocked buffer [C / 32][total][32], flat; element (row, c) at (c >> 5) * total * 32 +
    row * 32 + (c & 31).  Wrong variant: block = the stride of a 32-channel block in elements (the kernel's: total * 32)."""
    M, C = rows.shape
    flat = torch.full(((C // 32) * total * 32,), fill, dtype=rows.dtype)
    stride = total * 32 if block is None else block
    for b in range(C // 32):
        flat[b * stride:b * stride + M * 32] = rows[:, 32 * b:32 * b + 32].reshape(-1)
    return flat


def from_cb(flat, M, C, total):
    return torch.cat([flat[b * total * 32:b * total * 32 + M * 32].view(M, 32) for b in range(C // 32)], dim=1)


def gather(x, lst):
    """x[src_idx] with the kernel's clamp."""
    n = x.shape[0]
    return x[torch.tensor([min(max(v, 0), n - 1) for v in lst])]


def scatter(vals, lst, rows, fill=float('nan')):
    """out [rows][C]: vals[i] at row lst[i]; an entry outside [0, rows) is skipped."""
    out = torch.full((rows, vals.shape[1]), fill, dtype=vals.dtype)
    for i, v in enumerate(lst):
        if 0 <= v < rows:
            out[v] = vals[i]
    return out


# ------------------------------------------------------------------------------------------------------------ comparators
def tol_conv(T, g=None):
    return (G if g is None else g) * U * T


def detectable(t):
    """The smallest term of kind 2, MIN_TERM, is at least four times the largest tolerance of the case."""
    return MIN_TERM >= 4 * float(t.max())


def ratio(got, ref, T):
    """The largest |err| / (u T); an element without a term must be exactly 0."""
    err = (got.double() - ref).abs()
    r = torch.where(T > 0, err / (U * T.clamp_min(1e-300)), torch.where(err == 0, 0.0, float('inf')).double())
    return torch.nan_to_num(r, nan=float('inf')).max().item()


def flagged(got, ref, t):
    """The comparator of the kernel tests: any element off by more than its tolerance, or not finite."""
    return bool((~((got.double() - ref.double()).abs() <= t)).any())


def idx_flagged(got, ref, comparable=None):
    """Window indices: any comparable element (all of them: kind 1) that differs from the reference's."""
    bad = got.to(torch.int64) != ref
    return bool((bad if comparable is None else bad & comparable).any())


def excluded(comparable):
    return 1.0 - comparable.double().mean().item()


def winners(idx, ho, wo):
    """[d][Ho][Wo] bool: the conv positions that some window of some channel records as its maximum (idx [d][Hp][Wp][O])."""
    d, hp, wp, O = idx.shape
    py = torch.arange(hp).view(1, hp, 1, 1)
    px = torch.arange(wp).view(1, 1, wp, 1)
    y, x = 2 * py - 1 + idx // 3, 2 * px - 1 + idx % 3
    seen = torch.zeros(d, ho, wo, dtype=torch.bool)
    i = torch.arange(d).view(d, 1, 1, 1).expand_as(idx)
    seen[i.reshape(-1), y.reshape(-1), x.reshape(-1)] = True
    return seen


# ------------------------------------------------------------------------------------------------------------ refusals
# Per entry: an accepted base case and the refusing conditions of its launcher, each broken ALONE: ({argument: value}, answer).
# A pointer's value is its byte offset from a 16-B boundary, or None for NULL.  ('O': 68 carries ldo with it: ldo < O is another
# condition.)
def _fused_refusals(e):
    h16, u8, cb = e in IS_H16, e in IS_U8, e in IS_CB
    r = [({p: None}, 'bad_arg') for p in ('x', 'w', 'out', 'scale', 'shift')]
    r += [({'imgs': -1}, 'bad_arg'), ({'Cin': 0}, 'bad_arg'), ({'O': 0}, 'bad_arg'), ({'H': 0}, 'bad_arg'), ({'W': 0}, 'bad_arg')]
    r += [({'Cin': 4}, 'unsupported'), ({'KH': 5}, 'unsupported'), ({'KW': 5}, 'unsupported'), ({'stride': 1}, 'unsupported'),
          ({'pad': 2}, 'unsupported'), ({'H': 10}, 'unsupported'), ({'H': 2}, 'unsupported'), ({'W': 64}, 'unsupported'),
          ({'W': 130}, 'unsupported'), ({'W': 127}, 'unsupported'), ({'x': 1 if u8 else 4}, 'unsupported'),
          ({'out': 4 if h16 else 8}, 'unsupported')]
    if cb:
        r += [({'rows_total': 0}, 'bad_arg'), ({'O': 36}, 'bad_arg'), ({'rows_total': 2 * 32 - 1}, 'bad_arg'),
              ({'rows_total': 2 * 32 - 1, 'imgs': 1}, 'bad_arg'), ({'O': 96}, 'unsupported')]
    else:
        r += [({'ldo': 60}, 'bad_arg'), ({'O': 68, 'ldo': 68}, 'unsupported'), ({'O': 6}, 'unsupported'), ({'ldo': 66}, 'unsupported')]
    if e in IS_IDX:
        r += [({'idx': None}, 'bad_arg'), ({'src_imgs': 0}, 'bad_arg')]
    if e == 'argmax':
        r += [({'amax': None}, 'bad_arg'), ({'amax': 1}, 'unsupported')]
    if e in ('f16mul', 'cb'):
        r += [({'norm': 0}, 'bad_arg')]
    return r


_PTR5 = ('in', 'out', 'scale', 'shift')
REFUSAL_BASE = dict({e: Fused(e, 128, 8, 64, 64, 2) for e in FUSED_ENTRIES}, conv_stem=Stem(1, 3, 16, 16, 8, 8, 7, 7, 2, 3),
                    maxpool=Pool(1, 8, 4, 4, 8, 8, 0, ''), maxpool_argmax=Pool(1, 8, 4, 4, 8, 8, 1, ''),
                    u8_to_f32=U8(1, 3, 4, 4, 0),
                    **{'avgpool.' + e: Avg(e, 2, 64, 4, 32 if e == 'h16_cb' else 64, 64, 1) for e in ('f32', 'idx', 'h16', 'h16_cb')})
REFUSALS = dict({e: _fused_refusals(e) for e in FUSED_ENTRIES})
REFUSALS['conv_stem'] = [({p: None}, 'bad_arg') for p in ('x', 'w', 'out')] + [
    ({k: v}, 'bad_arg') for k, v in (('imgs', -1), ('Cin', 0), ('O', 0), ('KH', 0), ('KH', 8), ('KW', 0), ('KW', 9), ('stride', 0),
                                     ('ldc', 7), ('pad', -8))]
for _e in ('maxpool', 'maxpool_argmax'):
    REFUSALS[_e] = [({p: None}, 'bad_arg') for p in _PTR5] + [
        ({k: v}, 'bad_arg') for k, v in (('imgs', -1), ('C', 0), ('Hi', 0), ('Wi', 0), ('ldi', 7), ('ldo', 7))]
REFUSALS['maxpool_argmax'].append(({'amax': None}, 'bad_arg'))
for _e in ('f32', 'idx', 'h16', 'h16_cb'):
    REFUSALS['avgpool.' + _e] = [({p: None}, 'bad_arg') for p in _PTR5] + [
        ({k: v}, 'bad_arg') for k, v in (('imgs', -1), ('C', 0), ('S2', 0), ('ldo', 63))]
    REFUSALS['avgpool.' + _e] += [({'rows_total': 7}, 'bad_arg'), ({'C': 48}, 'bad_arg')] if _e == 'h16_cb' else [({'ldi': 63}, 'bad_arg')]
REFUSALS['avgpool.idx'] += [({'idx': None}, 'bad_arg'), ({'dst_rows': 0}, 'bad_arg')]
REFUSALS['u8_to_f32'] = [({'x': None}, 'bad_arg'), ({'out': None}, 'bad_arg'), ({'imgs': -1}, 'bad_arg'), ({'C': 0}, 'bad_arg'),
                         ({'H': 0}, 'bad_arg'), ({'W': 0}, 'bad_arg'), ({'C': 4, 'norm': 0}, 'bad_arg'),
                         ({'H': 3, 'W': 3}, 'unsupported'), ({'x': 1}, 'unsupported'), ({'out': 4}, 'unsupported')]
