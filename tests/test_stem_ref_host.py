"""CPU proofs of tests/stem_ref.py, which test_gpu_stem_forms.py holds the stem and pool kernels (csrc/stem_pool.hip) to: the
float64 references against torch's own float64 operators, the layout helpers' round trips, the dispatch mirror (every form
name reached by an accepted case of GRID, every refusing condition produced alone; the library's own gnx_*_form queries, which
touch no device, answering as the mirror on every case and every refusal), the fp32 ratios G was set from, the
properties the two kinds of input promise (exact integers, every conv position a recorded winner, the excluded share of index
comparisons), and that the comparator flags each wrong variant of the reference."""
import pytest
import torch
import torch.nn.functional as F

import stem_ref as R

FUSED = [c for c in R.GRID if isinstance(c, R.Fused)]
STEMS = [c for c in R.GRID if isinstance(c, R.Stem)]
POOLS = [c for c in R.GRID if isinstance(c, R.Pool)]
AVGS = [c for c in R.GRID if isinstance(c, R.Avg)]
U8S = [c for c in R.GRID if isinstance(c, R.U8)]
# one fused case per distinct set of float operands / per distinct reference (layout, list and batch length do not reach them)
FLOAT_GEO = list({(c.W, c.H, c.O, R.distinct(c)): c for c in FUSED if c.entry == 'f32'}.values())
PER_REF = list({(c.entry in R.IS_U8, c.entry in R.IS_F16MUL, c.entry in R.IS_H16, c.W, c.H, c.O, R.distinct(c)): c
                for c in FUSED}.values())
STEM_GEO = list({c[1:]: c for c in STEMS}.values())
SEEN = {}


def note(kind, ratio, c):
    if ratio > SEEN.get(kind, (0.0, None))[0]:
        SEEN[kind] = (ratio, c)


# ------------------------------------------------------------------------------------------------------------ the grid itself
def test_grid_holds_what_the_issue_asks_for():
    f = set(FUSED)
    for e in R.FUSED_ENTRIES:
        for W in (128, 256):
            assert {c.H for c in f if c.entry == e and c.W == W} >= set(R.FUSED_H[W])
            assert {c.imgs for c in f if c.entry == e and c.W == W} >= ({1, 5} if e in R.IS_IDX else {1, 3})
            assert any(c.ldo > c.O for c in f if c.entry == e and c.W == W) and any(c.ldo == c.O for c in f if c.entry == e)
            assert {c.O for c in f if c.entry == e} >= ({32, 64} if e in R.IS_CB else {4, 36, 64})
    assert R.FUSED_H[128] == (3, 4, 7, 8, 16, 36) and R.FUSED_H[256] == (3, 4, 7, 8, 16)
    assert R.fused_sizes(R.Fused('f32', 128, 36, 64, 64, 1))[0] // 2 == 9 and R.fused_sizes(R.Fused('f32', 256, 16, 64, 64, 1))[0] == 8
    for W, H in ((128, 128), (256, 256)):
        assert any((c.W, c.H) == (W, H) for c in f if c.entry == 'f32') and any((c.W, c.H) == (W, H) for c in f if c.entry == 'f16mul')
    assert {(c.W, c.imgs) for c in f if c.entry == 'f32' and c.imgs > 7} == {(128, 515), (256, 259)}
    assert {(c.W, c.imgs) for c in f if c.entry == 'f16mul' and c.imgs > 7} == {(128, 771), (256, 771)}
    assert all(c.H == 8 for c in f if c.imgs > 7)
    for c in f:
        if c.entry in R.IS_IDX and c.imgs >= 3:
            lst, d = R.src_list(c), R.distinct(c)
            assert min(lst) < 0 and max(lst) >= d and len(set(R.image_map(c))) < len(lst) and len(lst) == c.imgs
        if c.imgs > 7:                                     # the two images of any workgroup differ
            cap = R.CAP['f16' if c.entry in R.IS_F16MUL else 'f32', c.W]
            m = R.image_map(c)
            assert c.imgs == cap + 3 and cap % 7 and (c.entry in R.IS_IDX or all(m[i] != m[i + cap] for i in range(3)))
    assert any(c.entry in R.IS_IDX and c.imgs > 7 for c in f)
    s = STEMS
    patch = [c for c in s if R.form_of(c) in ('stem.patch7', 'stem.patch3')]
    for form in ('stem.patch7', 'stem.patch3'):
        p = [c for c in patch if R.form_of(c) == form]
        assert {c.O for c in p} >= {8, 10, 33, 64} and any(c.ldc > c.O for c in p) and any(c.H != c.W for c in p)
        assert any(c.pad == 0 for c in p)
        assert any(R.conv_out(c.H, c.KH, c.stride, c.pad) % 8 and R.conv_out(c.W, c.KW, c.stride, c.pad) % 16 for c in p)
        assert any(c.imgs * -(-R.conv_out(c.H, c.KH, c.stride, c.pad) // 8) * -(-R.conv_out(c.W, c.KW, c.stride, c.pad) // 16) > R.STEM_CAP
                   for c in p)
    gen = [c for c in s if R.form_of(c) == 'stem.generic']
    assert {c.O for c in gen if c.Cin == 3 and (c.KH, c.KW, c.stride, c.pad) == (7, 7, 2, 3)} >= {65, 96}
    assert {c.Cin for c in gen} >= {1, 3, 4} and any(c.KH != c.KW for c in gen) and any(c.KW == 8 for c in gen)
    assert any(c.stride == 3 and c.pad == 0 for c in gen)
    M = {c.imgs * R.conv_out(c.H, c.KH, c.stride, c.pad) * R.conv_out(c.W, c.KW, c.stride, c.pad) for c in gen}
    assert M >= {126, 128, 129, 257}
    p = POOLS
    assert {c.C for c in p} >= {1, 6, 8, 64} and any(c.Hi == 1 for c in p) and any(c.Hi % 2 and c.Wi % 2 and c.Hi != c.Wi for c in p)
    assert any(c.ldi > c.C for c in p) and any(c.ldo > c.C for c in p)
    for am in (0, 1):
        q = [c for c in p if c.argmax == am]
        assert {c.off for c in q} >= {'in', 'out', 'scale', 'shift'} | ({'amax'} if am else set())
        assert any(c.C % 4 and not c.ldi % 4 and not c.ldo % 4 for c in q) and any(not c.C % 4 and c.ldi % 4 and not c.ldo % 4 for c in q)
        assert any(not c.C % 4 and not c.ldi % 4 and c.ldo % 4 for c in q)
        for form, cap, per in (('scalar', R.POOL_CAP, 1), ('vec4', R.POOL4_CAP, 4)):
            big = [c for c in q if R.form_of(c).startswith('maxpool.' + form) and c.imgs * 2 * c.C // per > cap * 256]
            assert big and all((c.Hi, c.Wi) == (2, 3) and c.imgs * 2 * c.C // per <= cap * 256 + 16 for c in big)
    a = AVGS
    for e in ('f32', 'idx', 'h16'):
        assert {(c.C, c.S2) for c in a if c.entry == e} >= {(C, S) for C in (1, 63, 64, 65, 130) for S in (1, 3, 4, 5, 49, 1024)}
        assert all(c.ldi > c.C for c in a if c.entry == e)
    assert {c.S2 for c in a if c.entry == 'h16_cb'} >= {1, 3, 4, 5, 49, 1024} and any(c.extra for c in a if c.entry == 'h16_cb')
    for c in a:
        if c.entry == 'idx':
            lst = R.avg_dst(c)
            assert min(lst) < 0 and max(lst) >= c.imgs + c.extra and sorted(lst) != lst
            ok = [v for v in lst if 0 <= v < c.imgs + c.extra]
            assert len(set(ok)) == len(ok)
    assert {c.C for c in U8S} >= {1, 3, 4} and {c.norm for c in U8S} == {0, 1}
    assert any(c.imgs * c.C * c.H * c.W // 4 > R.U8_CAP * 256 for c in U8S)
    assert R.G >= R.G_FLOOR and R.G == max(R.G_FLOOR, 4 * max(R.TORCH_FP32_RATIO, R.CHAIN_FP32_RATIO))


# ------------------------------------------------------------------------------------------------------------ dispatch mirror
def test_every_form_is_reached_by_an_accepted_case():
    got = {R.form_of(c) for c in R.GRID}
    assert got == set(R.FORMS), (set(R.FORMS) - got, got - set(R.FORMS))
    assert len(R.FORMS) == 3 + 14 + 8 + 4 + 4 + 1


def test_every_refusing_condition_is_produced_alone():
    seen = set()
    for e, lst in R.REFUSALS.items():
        entry, a = R.call_of(R.REFUSAL_BASE[e])
        assert R.form_of_call(entry, a) in R.FORMS
        for over, want in lst:
            assert want in R.REFUSED and R.form_of_call(entry, dict(a, **over)) == want, (e, over, want)
            assert len(over) == 1 or set(over) in ({'O', 'ldo'}, {'rows_total', 'imgs'}, {'C', 'norm'}, {'H', 'W'}), over
            seen.add((e, want))
        assert R.form_of_call(entry, dict(a, imgs=0)) == R.EMPTY
    assert {e for e, w in seen if w == 'unsupported'} >= set(R.FUSED_ENTRIES) | {'u8_to_f32'}
    # the contract hole this grid closes: a channel-blocked buffer with fewer rows than the pooled map has
    for e in R.IS_CB:
        entry, a = R.call_of(R.REFUSAL_BASE[e])
        rows = a['imgs'] * 2 * 32
        assert R.form_of_call(entry, dict(a, rows_total=rows)) in R.FORMS and R.form_of_call(entry, dict(a, rows_total=rows - 1)) == 'bad_arg'


# ------------------------------------------------------------------------------------------------------------ mirror vs library
BASE = 1 << 20                                             # a 16-byte boundary: the queries look at a pointer's low bits only


def ask(entry, a):
    """((code, workgroups) of the library's query for the call, (code, workgroups) of the mirror); pointers go in as bare
    integers, `a`'s offsets from BASE.  None for an entry without a query."""
    import ctypes
    from gridnext_amd import _lib as L
    q = R.query_call(entry, a, {k: None if a.get(k) is None else BASE + a[k] for k in R.POINTERS})
    if q is None:
        return None
    wg = ctypes.c_int(-7)
    code = L.query(q[0], *q[1], ctypes.addressof(wg))
    assert L.query(q[0], *q[1], None) == code, 'NULL workgroups'
    want = R.query_answer(entry, a)
    return (code, wg.value), (L.CONSTANTS[want[0]], want[1])


def test_queries_answer_as_the_mirror_over_the_grid():
    """gnx_conv_stem_form, gnx_conv_stem_pool_form, gnx_conv_stem_pool_f16mul_form and gnx_bnrelu_maxpool_form (they touch no
    device) on every case of GRID: the code and the workgroups the mirror derives from CAP, STEM_CAP, POOL_CAP and POOL4_CAP; every
    code of the four queries is reached, and the batches above a cap are held to it."""
    from gridnext_amd import _lib as L
    caps = {'GNX_STEM_PATCH7': R.STEM_CAP, 'GNX_STEM_PATCH3': R.STEM_CAP, 'GNX_SP_64': R.CAP['f32', 128], 'GNX_SP_128': R.CAP['f32', 256],
            'GNX_SP16_64': R.CAP['f16', 128], 'GNX_SP16_128': R.CAP['f16', 256], 'GNX_MP_SCALAR': R.POOL_CAP, 'GNX_MP_VEC4': R.POOL4_CAP}
    reached, capped = set(), set()
    for c in R.GRID:
        entry, a = R.call_of(c)
        r = ask(entry, a)
        assert (r is None) == isinstance(c, (R.Avg, R.U8)), c
        if r is not None:
            got, want = r
            assert got == want, (c, got, want)
            code = R.query_answer(entry, a)[0]
            assert code in R.QUERY_CODES and 0 < got[1] <= caps.get(code, got[1]), (c, got)
            reached.add(code)
            if got[1] == caps.get(code):
                capped.add(code)
    assert reached == set(R.QUERY_CODES) and capped == set(caps)            # (the generic stem's grid has no cap)
    for prefix, n in (('GNX_STEM_', 3), ('GNX_SP_', 2), ('GNX_SP16_', 2), ('GNX_MP_', 2)):
        assert sorted(L.CONSTANTS[k] for k in L.CONSTANTS if k.startswith(prefix)) == list(range(n)), prefix
        assert {k for k in L.CONSTANTS if k.startswith(prefix)} == {k for k in R.QUERY_CODES if k.startswith(prefix)}


@pytest.mark.parametrize('e', list(R.REFUSALS), ids=str)
def test_queries_refuse_as_the_mirror(e):
    """Each refusing condition of the launchers broken alone, imgs == 0, then the accepted call: the query's answer is the mirror's,
    and it is the call's own code except for the one condition an entry point checks before its launcher sees the call."""
    from gridnext_amd import _lib as L
    entry, a = R.call_of(R.REFUSAL_BASE[e])
    for over, want in R.REFUSALS[e] + [({'imgs': 0}, R.EMPTY), ({}, None)]:
        b = dict(a, **over)
        r = ask(entry, b)
        if r is None:
            assert entry.startswith('avgpool.') or entry == 'u8_to_f32'
            continue
        got, mirror = r
        assert got == mirror, (over, got, mirror)
        own = any(k in ('idx', 'amax') and v is None for k, v in over.items())         # a NULL list / index: the entry point's check
        if want in R.REFUSED and not own:
            assert got == (L.CONSTANTS[R.ERROR_CODE[want]], 0), (over, got)
        elif want == R.EMPTY:
            assert got == (0, 0), (over, got)
        else:
            assert got[0] >= 0 and got[1] > 0, (over, got)


# ------------------------------------------------------------------------------------------------------------ references vs torch
@pytest.mark.parametrize('c', PER_REF, ids=R.ids)
def test_fused_reference_against_torch(c):
    """conv, act and the pool of both kinds against torch's float64 F.conv2d / F.max_pool2d; the index against torch's wherever the
    maximum is unique, and on kind 1 EVERYWHERE: torch's float64 pool agrees with the first-maximum rule, ties included."""
    ho, wo, hp, wp = R.fused_sizes(c)
    for kind in ('int', 'mag'):
        r, ref = R.fused_inputs(c, kind), R.fused_reference(c, kind)
        x, w = R.fused_operands(c, kind)
        pre = F.conv2d(x, w, stride=2, padding=3)
        assert pre.shape == ref.pre.shape == (R.distinct(c), c.O, ho, wo)
        assert bool(((pre - ref.pre).abs() <= 2.0 ** -40 * ref.T).all())
        a = F.relu(pre * r.scale.double().view(1, -1, 1, 1) + r.shift.double().view(1, -1, 1, 1))
        val, ind = F.max_pool2d(a, 3, 2, 1, return_indices=True)
        assert val.shape[2:] == (hp, wp) and ref.val.shape == (R.distinct(c), hp, wp, c.O)
        win = (ind // wo - (2 * torch.arange(hp).view(1, 1, hp, 1) - 1)) * 3 + (ind % wo - (2 * torch.arange(wp).view(1, 1, 1, wp) - 1))
        win = win.permute(0, 2, 3, 1)
        if kind == 'int':
            assert float(pre.abs().max()) <= (128 if c.entry not in R.IS_U8 else 294)
            assert torch.equal(pre, ref.pre) and torch.equal(val.permute(0, 2, 3, 1), ref.val)
            assert torch.equal(ref.val.float().double(), ref.val) and torch.equal(ref.val.half().double(), ref.val)
            assert torch.equal(win, ref.idx)
        else:
            assert bool(((val.permute(0, 2, 3, 1) - ref.val).abs() <= ref.tol * 2.0 ** -10).all())
            assert not R.idx_flagged(win, ref.idx, ref.comparable)
            assert R.excluded(ref.comparable) <= R.MAX_EXCLUDED, R.excluded(ref.comparable)
            if c.entry not in R.IS_U8:
                assert R.detectable(ref.tol), float(ref.tol.max())
        assert int(ref.idx.min()) >= 0 and int(ref.idx.max()) <= 8


@pytest.mark.parametrize('c', [c for c in FLOAT_GEO if c.O == 64 and R.distinct(c) >= 3], ids=R.ids)
def test_integer_inputs_make_every_conv_position_a_recorded_winner(c):
    """Kind 1, O == 64, three images or more: every position of the conv0 map is the recorded maximum of some window of some
    channel, and 2 to 10 % of the windows hold an exact tie - no tap or position can be wrong unseen."""
    ho, wo, _, _ = R.fused_sizes(c)
    ref = R.fused_reference(c, 'int')
    assert bool(R.winners(ref.idx, ho, wo).all())
    ties = 1.0 - R.maxpool(R.act(ref.pre, R.fused_inputs(c, 'int').scale.double(), R.fused_inputs(c, 'int').shift.double()),
                           torch.zeros_like(ref.pre)).comparable.double().mean().item()
    assert 0.02 <= ties <= 0.25, ties


@pytest.mark.parametrize('c', STEM_GEO, ids=R.ids)
def test_stem_reference_against_torch(c):
    for kind in ('int', 'mag'):
        r, ref = R.stem_inputs(c, kind), R.stem_reference(c, kind)
        pre = F.conv2d(r.x.double(), r.w.double(), stride=c.stride, padding=c.pad)
        assert bool(((R.as_rows(pre) - ref.val).abs() <= 2.0 ** -40 * R.as_rows(ref.T)).all())
        if kind == 'int':
            assert torch.equal(R.as_rows(pre), ref.val) and torch.equal(ref.val.float().double(), ref.val)
        else:
            assert R.detectable(ref.tol)


@pytest.mark.parametrize('c', list({(c.C, c.Hi, c.Wi): c for c in POOLS}.values()), ids=R.ids)
def test_pool_reference_against_torch(c):
    ho, wo = R.pooled(c.Hi), R.pooled(c.Wi)
    for kind in ('int', 'mag'):
        r, ref = R.pool_inputs(c, kind), R.pool_reference(c, kind)
        a = F.relu(r.x.double() * r.scale.double().view(1, -1, 1, 1) + r.shift.double().view(1, -1, 1, 1))
        val, ind = F.max_pool2d(a, 3, 2, 1, return_indices=True)
        win = (ind // c.Wi - (2 * torch.arange(ho).view(1, 1, ho, 1) - 1)) * 3 + (ind % c.Wi - (2 * torch.arange(wo).view(1, 1, 1, wo) - 1))
        assert torch.equal(val.permute(0, 2, 3, 1), ref.val)
        if kind == 'int':
            assert torch.equal(win.permute(0, 2, 3, 1), ref.idx) and torch.equal(ref.val.float().double(), ref.val)
        else:
            assert not R.idx_flagged(win.permute(0, 2, 3, 1), ref.idx, ref.comparable)
            assert R.excluded(ref.comparable) <= R.MAX_EXCLUDED and R.detectable(ref.tol)


@pytest.mark.parametrize('c', AVGS, ids=R.ids)
def test_avgpool_reference_against_torch(c):
    for kind in ('int', 'mag'):
        r, ref = R.avg_inputs(c, kind), R.avg_reference(c, kind)
        want = F.relu(r.x.double() * r.scale.double() + r.shift.double()).view(c.imgs, c.S2, c.C).mean(1)
        assert bool(((want - ref.val).abs() <= 2.0 ** -45 * (1 + ref.val)).all()) and R.detectable(ref.tol)
        if c.entry in ('h16', 'h16_cb'):
            assert torch.equal(r.x.half().float(), r.x)


def test_to_tensor_is_torch_in_float32():
    g = torch.Generator().manual_seed(1)
    x8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).expand(2, 3, 16, 16).contiguous()
    assert torch.equal(R.to_tensor(x8, 0), x8.float() / 255.0)
    mean, std = torch.tensor(R.MEAN).view(1, 3, 1, 1), torch.tensor(R.STD).view(1, 3, 1, 1)
    assert torch.equal(R.to_tensor(x8, 1), ((x8.float() / 255.0) - mean) / std) and R.to_tensor(x8, 1).dtype == torch.float32
    nv = R.norm_vector()
    assert torch.equal(nv[:3], torch.tensor(R.MEAN)) and torch.equal(nv[6:], 1.0 / torch.tensor(R.STD)) and nv.dtype == torch.float32
    h = R.half_round(R.signed(g, 0.5, 1.5, 1000).double())
    assert torch.equal(h.half().double(), h)


# ------------------------------------------------------------------------------------------------------------ layouts
def test_layout_helpers_round_trip():
    g = torch.Generator().manual_seed(2)
    rows = torch.rand(12, 64, generator=g)
    buf = R.to_ld(rows, 72, 4)
    assert torch.equal(R.from_ld(buf, 64, 4), rows) and bool(torch.isnan(buf[:, :4]).all()) and bool(torch.isnan(buf[:, 68:]).all())
    for total in (12, 17):
        cb = R.to_cb(rows, total)
        assert cb.numel() == 2 * total * 32 and torch.equal(R.from_cb(cb, 12, 64, total), rows)
        assert int(torch.isnan(cb).sum()) == 2 * (total - 12) * 32
        assert cb[1 * total * 32 + 5 * 32 + 7] == rows[5, 39]
    assert torch.equal(R.as_rows(R.as_map(rows, 2, 2, 3)), rows) and R.as_map(rows, 2, 2, 3).shape == (2, 64, 2, 3)
    x = torch.rand(5, 3, generator=g)
    assert torch.equal(R.gather(x, [-4, 0, 4, 5, 99, 2, 2]), x[[0, 0, 4, 4, 4, 2, 2]])
    s = R.scatter(x, [3, -1, 0, 6, 5], 6)
    assert torch.equal(s[[3, 0, 5]], x[[0, 2, 4]]) and bool(torch.isnan(s[[1, 2, 4]]).all())
    assert torch.equal(R.half_round(torch.tensor([1.0 + 2.0 ** -12])), torch.tensor([1.0]))


# ------------------------------------------------------------------------------------------------------------ G
def _ratios(x, w, stride, pad):
    ref = R.conv(x.double(), w.double(), stride, pad)
    T = R.conv(x.double().abs(), w.double().abs(), stride, pad)
    n = torch.get_num_threads()
    torch.set_num_threads(1)                               # torch's blocking of the sum follows the thread count: measure it on one
    try:
        rt = R.ratio(F.conv2d(x, w, stride=stride, padding=pad), ref, T)
    finally:
        torch.set_num_threads(n)
    return rt, R.ratio(R.conv(x, w, stride, pad), ref, T)


def _measure():
    for c in FLOAT_GEO:
        r = R.fused_inputs(c, 'mag')
        rt, rc = _ratios(r.x, r.w, 2, 3)
        note('torch', rt, c)
        note('chain', rc, c)
    for c in STEM_GEO:
        r = R.stem_inputs(c, 'mag')
        rt, rc = _ratios(r.x, r.w, c.stride, c.pad)
        note('torch', rt, c)
        note('chain', rc, c)


def test_recorded_ratios_are_what_the_grid_gives(capsys):
    """The two plain fp32 evaluations of every convolution of GRID (kind 2) against float64.  The chain is elementwise IEEE
    arithmetic: its largest ratio is the recorded one to the printed digits, at the recorded case.  torch's CPU convolution
    blocks its sums by its build: it is measured on one thread, printed, and held to G / 4."""
    _measure()
    with capsys.disabled():
        print('\n G = %.3f' % R.G)
        for kind, (ratio, c) in sorted(SEEN.items()):
            print(' largest fp32 %-5s ratio %.4f at %s' % (kind, ratio, R.ids(c)))
    assert abs(SEEN['chain'][0] - R.CHAIN_FP32_RATIO) <= 5e-4, SEEN['chain']
    assert R.ids(SEEN['chain'][1]) == R.CHAIN_FP32_AT
    assert SEEN['torch'][0] <= R.G / 4 + 5e-4, SEEN['torch']
    assert R.G == pytest.approx(17.456) and R.G >= 4 * SEEN['chain'][0]


# ------------------------------------------------------------------------------------------------------------ mutants
def _got(c, kind, **wrong):
    return R.fused_eval(c, kind, **wrong)


MUT_F32 = R.Fused('f32', 128, 8, 64, 64, 3)
MUT_U8 = R.Fused('u8', 128, 8, 64, 64, 3)
MUT_F16 = R.Fused('f16mul', 128, 8, 64, 64, 3)
MUT_CB = R.Fused('cb', 128, 8, 64, 72, 3)
MUT_ARG = R.Fused('argmax', 128, 8, 64, 64, 3)


@pytest.mark.parametrize('name, c, wrong', [
    ('window one row off', MUT_F32, dict(dy=1)), ('window one row off, fp16', MUT_F16, dict(dy=-1)),
    ('window one column off', MUT_F32, dict(dx=1)), ('window one column off, u8', MUT_U8, dict(dx=-1)),
    ('carry not reset at an image boundary', MUT_F32, dict(carry=True)),
    ('carry not reset at an image boundary, fp16', MUT_F16, dict(carry=True)),
    ('edge pixel instead of zero padding', MUT_F32, dict(edge=True)),
    ('uint8 padding with pixel 0 after Normalize', MUT_U8, dict(padval=-torch.tensor(R.MEAN) / torch.tensor(R.STD))),
    ('the 22nd (c, ky) group counted twice', MUT_F16, dict(twice=(2, 6)))], ids=lambda v: v if isinstance(v, str) else '')
def test_comparator_flags_wrong_values(name, c, wrong):
    assert any(c[:4] == k[:4] and c.imgs == k.imgs for k in FUSED)                   # a case the kernel tests run
    kinds = ('mag',) if 'padval' in wrong else ('int', 'mag')                # (kind 1 of uint8 runs without Normalize)
    for kind in kinds:
        ref = R.fused_reference(c, kind)
        got = _got(c, kind, **wrong)
        assert not R.flagged(ref.val, ref.val, ref.tol)
        if kind == 'int':
            assert not torch.equal(got.val, ref.val), name
        else:
            assert R.flagged(got.val.float(), ref.val, ref.tol), name


def test_comparator_flags_wrong_indices_and_layouts():
    ref = R.fused_reference(MUT_ARG, 'int')
    got = _got(MUT_ARG, 'int', ge=True)
    assert torch.equal(got.val, ref.val) and R.idx_flagged(got.idx, ref.idx) and not R.idx_flagged(ref.idx, ref.idx)
    ref2 = R.fused_reference(MUT_ARG, 'mag')                 # kind 2 cannot see >= (its ties are excluded) but sees a window shift
    assert not R.idx_flagged(_got(MUT_ARG, 'mag', ge=True).idx, ref2.idx, ref2.comparable)
    assert R.idx_flagged(_got(MUT_ARG, 'mag', dx=1).idx, ref2.idx, ref2.comparable)
    # stand-alone max pool
    p = next(c for c in POOLS if c.argmax and c.C == 8 and c.Hi == 5)
    r, pr = R.pool_inputs(p, 'int'), R.pool_reference(p, 'int')
    wrong = R.maxpool(R.act(r.x.double(), r.scale.double(), r.shift.double()), ge=True)
    assert R.idx_flagged(wrong.idx.permute(0, 2, 3, 1), pr.idx)
    # block 1 of the channel-blocked layout at rows * 32 instead of rows_total * 32: seen where rows_total > rows
    rows = R.fused_reference(MUT_CB, 'mag').val.reshape(-1, 64)
    M, total = rows.shape[0], R.rows_total(MUT_CB)
    assert total > M
    good, bad = R.to_cb(rows, total), R.to_cb(rows, total, block=M * 32)
    tol = R.fused_reference(MUT_CB, 'mag').tol.reshape(-1, 64)
    assert not R.flagged(R.from_cb(good, M, 64, total), rows, tol) and R.flagged(R.from_cb(bad, M, 64, total), rows, tol)
    assert torch.equal(R.to_cb(rows, M), R.to_cb(rows, M, block=M * 32))          # ... and only there
