"""GPU: the masked cross-entropy with options (GF.masked_cross_entropy_opt -> gnx_masked_ce_opt_fwd / _bwd) at its kernel edges
and over nn.CrossEntropyLoss's scalar-valued options, against the float64 restatement tests/ce_ref.py (proved on the CPU by
test_ce_ref_host.py).

Tolerance: measured per case, never fixed.  On the same fp32 inputs torch's own fp32 CPU cross_entropy (the generic loop's chain)
has an error against ce_ref, for the loss and for max |dz|; the HIP error must be <= 4 x that (another summation order, another
expf: a few ulp each), with a floor of one fp32 ulp at the reference's magnitude for the cases where torch happens to be exact.
Both errors are printed per case (run with -s).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _case(M=513, C=8, base=1, w='rand', e=0.1, ign=-100, red='mean', accum=1, wide=False, dloss=1.0):
    return dict(M=M, C=C, base=base, w=w, e=e, ign=ign, red=red, accum=accum, wide=wide, dloss=dloss)


def _cases():
    out = [_case()]
    out += [_case(M=M) for M in (1, 255, 256, 257, 4992)]                    # the block boundary; 1, 2, 3 (base case) and 20 partials
    out += [_case(C=C) for C in (1, 2, 65)]
    out += [_case(base=0), _case(wide=True)]
    out += [_case(w=w) for w in (None, 'zero')]
    out += [_case(e=e) for e in (0.0, 1.0)]
    out += [_case(ign=3), _case(red='sum'), _case(accum=3)]
    out += [_case(M=257, C=65, w='zero', e=1.0, ign=3, red='sum', accum=3, dloss=0.37),      # crossed
            _case(M=4992, C=2, base=0, w=None, e=0.1, red='sum'),
            _case(M=255, C=8, base=0, w='zero', e=0.0, ign=3, accum=3, wide=True),
            _case(M=1, C=1, w='rand', e=0.1),
            _case(M=256, C=65, w=None, e=0.0, red='sum', dloss=2.5),
            _case(M=4992, C=8, w='rand', e=1.0, ign=3, accum=3)]
    return out


CASES = _cases()


def _id(c):
    return "M%d-C%d-b%d-w%s-e%g-i%d-%s-a%d%s%s" % (c['M'], c['C'], c['base'], c['w'], c['e'], c['ign'], c['red'], c['accum'],
                                                    '-wide' if c['wide'] else '', '-dl%g' % c['dloss'] if c['dloss'] != 1 else '')


def _inputs(c):
    z, lab = R.case(c['M'], c['C'], c['base'], seed=3, ignore_index=c['ign'])
    if c['M'] == 1:
        lab[0] = c['base'] + c['C'] - 1                                      # (one row: a selected one)
    return z, lab, R.weights(c['w'], c['C'], seed=3)


def _hip(z, lab, w, c, **over):
    """(loss, stats, preds, dz) on the device, copied back.  wide: the rows are a column window of a wider buffer (ld > C)."""
    o = dict(c, **over)
    C = z.shape[1]
    if o['wide']:
        buf = torch.randn(z.shape[0], C + 5, device=DEV)
        buf[:, 2:2 + C] = z.to(DEV)
        leaf = buf.requires_grad_(True)
        rows = leaf[:, 2:2 + C]
    else:
        leaf = rows = z.to(DEV).requires_grad_(True)
    from gridnext_amd import functional as GF
    loss, stats, preds = GF.masked_cross_entropy_opt(rows, lab.to(DEV), o['accum'], o['base'], None if w is None else w.to(DEV),
                                                     o['e'], o['ign'], o['red'])
    (loss * o['dloss']).backward()
    torch.cuda.synchronize()
    g = leaf.grad.cpu()
    if o['wide']:
        assert (g[:, :2] == 0).all() and (g[:, 2 + C:] == 0).all()
        g = g[:, 2:2 + C].contiguous()
    return loss.detach().cpu(), stats.cpu(), preds.cpu(), g


def _torch_fp32(z, lab, w, c):
    """The generic loop's chain in fp32 on the CPU: the measure of what fp32 costs on these inputs."""
    zt = z.clone().requires_grad_(True)
    keep = lab >= c['base']
    loss = F.cross_entropy(zt[keep], lab[keep] - c['base'], weight=w, ignore_index=c['ign'], reduction=c['red'],
                           label_smoothing=c['e']) / c['accum']
    (loss * c['dloss']).backward()
    return loss.detach(), zt.grad


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_opt_family_against_float64(c, capsys):
    z, lab, w = _inputs(c)
    ref = R.masked_ce(z, lab, c['base'], w, c['e'], c['ign'], c['red'], c['accum'], c['dloss'])
    assert math.isfinite(ref.loss.item())
    t_loss, t_dz = _torch_fp32(z, lab, w, c)
    loss, stats, preds, dz = _hip(z, lab, w, c)
    loss2, stats2, preds2, dz2 = _hip(z, lab, w, c)
    e_t = (abs(t_loss.double().item() - ref.loss.item()), (t_dz.double() - ref.dz).abs().max().item())
    e_h = (abs(loss.double().item() - ref.loss.item()), (dz.double() - ref.dz).abs().max().item())
    tol = (max(4 * e_t[0], R.ulp32(ref.loss)), max(4 * e_t[1], R.ulp32(ref.dz.abs().max())))
    with capsys.disabled():
        print("\n[masked CE opt %s] loss %.9g: err hip %.3e torch fp32 %.3e (tol %.3e); max|dz| %.3e: err hip %.3e torch fp32 %.3e "
              "(tol %.3e)" % (_id(c), ref.loss.item(), e_h[0], e_t[0], tol[0], ref.dz.abs().max().item(), e_h[1], e_t[1], tol[1]))
    # exact
    assert torch.equal(preds, ref.preds)
    assert tuple(stats.tolist()) == ref.stats
    assert (dz[~ref.live] == 0).all()
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2) and torch.equal(stats, stats2) and torch.equal(preds, preds2)
    # measured
    assert e_h[0] <= tol[0], "loss: hip error %.3e > %.3e (torch fp32: %.3e)" % (e_h[0], tol[0], e_t[0])
    assert e_h[1] <= tol[1], "dz: hip error %.3e > %.3e (torch fp32: %.3e)" % (e_h[1], tol[1], e_t[1])


def test_first_maximal_index_on_ties():
    z = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]])
    lab = torch.tensor([2, 1, 4])
    c = _case(M=3, C=4, w=None, e=0.0)
    _, stats, preds, _ = _hip(z, lab, None, c)
    assert preds.tolist() == [1, 0, 2] and stats.tolist() == [3, 2]


@pytest.mark.parametrize("red", R.REDUCTIONS)
def test_empty_reductions(red):
    """All rows ignored, nothing selected, only zero-weight classes: NaN under 'mean' (0 / 0, as torch), exactly 0 under 'sum';
    dz exactly 0 where nothing is live."""
    c = _case(M=300, C=5, w='zero', red=red)
    z, lab, w = _inputs(c)
    runs = {'ignored': (torch.full_like(lab, 4), 3, 0.1), 'none': (torch.zeros_like(lab), -100, 0.1),
            'zero_w': (torch.full_like(lab, 5 // 2 + 1), -100, 0.0)}
    for name, (labels, ign, e) in runs.items():
        loss, stats, _, dz = _hip(z, labels, w, c, ign=ign, e=e)
        ref = R.masked_ce(z, labels, 1, w, e, ign, red)
        assert tuple(stats.tolist()) == ref.stats, name
        if red == 'mean':
            assert math.isnan(loss.item()), name
        else:
            assert loss.item() == 0.0, name
        if name != 'zero_w':
            assert (dz == 0).all(), name


@pytest.mark.parametrize("red", R.REDUCTIONS)
def test_class_index_past_c_is_nan_and_reads_nothing(red):
    c = _case(M=300, C=5, red=red)
    z, lab, w = _inputs(c)
    lab[7] = 5 + 1 + 2 ** 40                                                 # (far outside any buffer)
    lab[299] = 5 + 1
    loss, stats, preds, dz = _hip(z, lab, w, c)
    ref = R.masked_ce(z, lab, 1, w, c['e'], c['ign'], red)
    assert math.isnan(loss.item()) and torch.isnan(dz[7]).all() and torch.isnan(dz[299]).all()
    assert (dz[~ref.live] == 0).all() and torch.equal(preds, ref.preds) and tuple(stats.tolist()) == ref.stats


@pytest.mark.parametrize("M,C,base", [(513, 8, 1), (257, 5, 0), (4992, 20, 1), (1, 3, 1)])
def test_default_options_equal_the_plain_family(M, C, base):
    """weight None, e 0, ignore_index -100, 'mean': the plain family's loss within 1 fp32 ulp (bit-equality is not promised: the
    two kernels may round the per-row term differently), the same stats and preds."""
    from gridnext_amd import functional as GF
    z, lab = R.case(M, C, base, seed=11)
    if M == 1:
        lab[0] = base
    for accum in R.ACCUMS:
        zp = z.to(DEV).requires_grad_(True)
        lp, sp, pp = GF.masked_cross_entropy(zp, lab.to(DEV), accum, label_base=base)
        lp.backward()
        lo, so, po, dzo = _hip(z, lab, None, _case(M=M, C=C, base=base, w=None, e=0.0, accum=accum))
        assert abs(lo.item() - lp.item()) <= R.ulp32(lp.item())
        assert torch.equal(so, sp.cpu()) and torch.equal(po, pp.cpu())
        np.testing.assert_allclose(dzo.numpy(), zp.grad.cpu().numpy(), rtol=0, atol=4 * R.ulp32(zp.grad.abs().max().item()))


def test_bad_arguments_are_refused():
    from gridnext_amd import _lib as L
    from gridnext_amd import functional as GF
    z, lab = R.case(10, 4, 1)
    zd, ld = z.to(DEV), lab.to(DEV)
    for e in (-0.1, 1.5, float('nan')):
        with pytest.raises(RuntimeError, match="gnx_masked_ce_opt_fwd failed: bad argument"):
            GF.masked_cross_entropy_opt(zd, ld, label_smoothing=e)
    with pytest.raises(ValueError, match="reduction"):
        GF.masked_cross_entropy_opt(zd, ld, reduction='none')
    with pytest.raises(ValueError, match="class weights"):
        GF.masked_cross_entropy_opt(zd, ld, weight=torch.ones(5, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        GF.masked_cross_entropy_opt(zd, ld, weight=torch.ones(4))
    with pytest.raises(TypeError, match="float32"):
        GF.masked_cross_entropy_opt(zd, ld, weight=torch.ones(4, device=DEV, dtype=torch.float64))
    # the C ABI itself: an unknown reduction, ld < C
    loss, den = torch.empty((), device=DEV), torch.empty(1, device=DEV, dtype=torch.float64)
    stats, ws = torch.empty(2, device=DEV, dtype=torch.int64), torch.empty(4, device=DEV, dtype=torch.float64)
    args = lambda ldz, red: (zd.data_ptr(), ldz, ld.data_ptr(), 10, 4, 1, None, 0.0, -100, red, 1.0, loss.data_ptr(),
                             stats.data_ptr(), den.data_ptr(), None, ws.data_ptr(), L.stream())
    assert L.lib().gnx_masked_ce_opt_fwd(*args(4, 2)) == -1
    assert L.lib().gnx_masked_ce_opt_fwd(*args(3, 0)) == -1
    assert L.lib().gnx_masked_ce_opt_fwd(*args(4, 1)) == 0
    torch.cuda.synchronize()
    assert L.query('gnx_masked_ce_opt_workspace', 257) == 8
