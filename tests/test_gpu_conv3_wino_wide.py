"""The 8-wave form of the Winograd conv2 (conv3x3_wino_kernel<S, 8>: 512-pixel tiles, S = 16 and 32), the halo-free staging of
both forms where a tile holds whole images, and the single raw-strip buffer (csrc/conv3x3.hip).

gnx_conv3x3_winograd runs the wide form from 262144 rows on; gnx_conv3x3_winograd_wide runs it at any M, which is how the cases
below reach it at a size a test can afford.  An output element's sum order does not depend on the tile it falls in (chunks in
order, the k parity over two accumulators, then the output transform), so the wide form must give the 256-pixel form's BITS:
every case holds gnx_conv3x3_winograd_wide against the float64 reference with conv3_ref's per-element gate G_WINO 2^-24 T (measured
on references alone; the algebra is the same) and against gnx_conv3x3_winograd of the same operands with torch.equal.

  S   images  K        tiles of 512 pixels
  16  1       32       half a tile
  16  2       32       one full tile, both array ends in it
  16  3, 17   32       a ragged last tile (half a tile)
  16  514     32       257 tiles: a second round, the XCD-permuted and the plain order meet
  32  1       32, 96   two tiles, image top and bottom; K = 96: an odd number of chunk pairs
  32  129     32       258 tiles
  32  5       128      ten tiles, the headline's K

Operands and outputs lie as test_gpu_conv3_forms.py lays them (sentinel rows above and below, an odd leading dimension for the
output at a column offset); each case also writes a padded output with ldc = 36 at a two-column offset and holds the guard columns.
"""
import pytest
import torch

import conv3_ref as R
from gridnext_amd import _lib as L
from test_gpu_conv3_forms import UNSUPPORTED, WinoOps, query, ratio_of

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WINO, WINO8 = R.CODES['wino'], R.CODES['wino8']
WIDE_CASES = [R.wino(1, 16, 32), R.wino(2, 16, 32), R.wino(3, 16, 32), R.wino(17, 16, 32), R.wino(514, 16, 32),
              R.wino(1, 32, 32), R.wino(1, 32, 96), R.wino(129, 32, 32), R.wino(5, 32, 128)]


def ids(c):
    return '%dx%d-K%d' % (c.n, c.S, c.K)


def run(name, o, out):
    L.call(name, *o.args(out), L.stream())
    torch.cuda.synchronize()
    assert o.A.unchanged() and o.Wu.unchanged(), name + ': an input was written'
    assert out.outside_unchanged(), name + ': wrote outside the window'
    return out


def gate(c, what, got):
    ref = R.reference(c)
    t = R.tol(ref.T, R.G_WINO)
    assert R.detectable(ref.term, t), what + ': the smallest non-zero term is below 4 tolerances'
    worst = ratio_of(what, got, ref.ref, t)
    print('%s: worst |err| / tolerance %.3f' % (what, worst))


@pytest.mark.parametrize("c", WIDE_CASES, ids=ids)
def test_wide_form_against_float64_and_the_256_pixel_form(c):
    M = R.rows(c)
    assert M < R.WIDE_ROWS
    o = WinoOps(c)
    what = 'wide, %d maps of %d x %d, K %d (%d tiles of 512, %d rows in the last)' % (c.n, c.S, c.S, c.K, -(-M // 512),
                                                                                    M % 512 or 512)
    narrow = o.out()
    assert query('gnx_conv3x3_winograd_form', *o.args(narrow)) == (WINO, min(-(-M // 256), 256)), what
    run('gnx_conv3x3_winograd', o, narrow)
    wide = run('gnx_conv3x3_winograd_wide', o, o.out())
    gate(c, what, wide.get())
    assert torch.equal(wide.flat, narrow.flat), what + ': not the bits of the 256-pixel form'
    again = run('gnx_conv3x3_winograd_wide', o, o.out())
    assert torch.equal(again.flat, wide.flat), what + ': a second call gives other bits'
    # a padded output: ldc = 36, two guard columns on either side
    pad = torch.full((M, 36), 7.0, device=DEV)
    L.call('gnx_conv3x3_winograd_wide', o.A.ptr, o.lo.lda, o.Wu.ptr, pad.data_ptr() + 4 * 2, 36, M, c.N, c.K, c.S, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(pad[:, 2:34], wide.win), what + ': other bits with ldc = 36'
    assert float(pad[:, :2].min()) == 7.0 == float(pad[:, :2].max()) and float(pad[:, 34:].min()) == 7.0 == float(pad[:, 34:].max())


@pytest.mark.parametrize("c", [R.wino(1, 16, 32), R.wino(5, 8, 32)], ids=ids)
def test_halo_free_staging_of_the_256_pixel_form(c):
    """S = 8 and 16: a 256-pixel tile holds whole images and stages no halo; one image of 16 x 16 is exactly one tile, five of
    8 x 8 leave a ragged second one."""
    o = WinoOps(c)
    out = run('gnx_conv3x3_winograd', o, o.out())
    gate(c, '256-pixel form, %d maps of %d x %d' % (c.n, c.S, c.S), out.get())


def test_dispatch_goes_wide_from_262144_rows_at_16_and_32():
    c = R.wino(R.WIDE_ROWS // 256, 16, 32)
    M = R.rows(c)
    o = WinoOps(c)
    out = o.out()
    assert query('gnx_conv3x3_winograd_form', *o.args(out)) == (WINO8, 256)
    assert query('gnx_conv3x3_winograd_form', *o.args(out, M=M - 256)) == (WINO, 256)
    assert query('gnx_conv3x3_winograd_form', *o.args(out, M=M, S=8)) == (WINO, 256)          # 4096 maps of 8 x 8
    assert query('gnx_conv3x3_winograd_form', *o.args(out, M=M, S=32)) == (WINO8, 256)
    assert query('gnx_conv3x3_winograd_form', *o.args(out, M=M, S=64)) == (WINO, 256)
    assert query('gnx_conv3x3_winograd_form', *o.args(out, M=M + 256)) == (WINO8, 256)        # 512 does not divide M
    run('gnx_conv3x3_winograd', o, out)
    wide = run('gnx_conv3x3_winograd_wide', o, o.out())
    assert torch.equal(out.flat, wide.flat)
    assert bool((out.win.abs() < 1.0e6).all()), 'a NaN, an infinity or an unwritten element in the window'


def test_wide_refusals_write_nothing():
    c = R.wino(16, 16, 32)                                    # 4096 rows: whole maps of 8 x 8 and of 64 x 64 as well
    o = WinoOps(c)
    for kw in (dict(N=16), dict(S=8), dict(S=64), dict(S=4), dict(A=o.A.ptr + 4), dict(Wu=o.Wu.ptr + 4), dict(K=16),
               dict(lda=o.lo.lda + 1)):
        out = o.out()
        assert L.query('gnx_conv3x3_winograd_wide', *o.args(out, **kw), L.stream()) == UNSUPPORTED, kw
        torch.cuda.synchronize()
        assert out.unchanged() and o.A.unchanged() and o.Wu.unchanged(), kw
    out = o.out()
    assert L.query('gnx_conv3x3_winograd_wide', *o.args(out, M=R.rows(c) + 1), L.stream()) == -1
    assert L.query('gnx_conv3x3_winograd_wide', *o.args(out, M=0), L.stream()) == 0
    torch.cuda.synchronize()
    assert out.unchanged()


def test_densenet121_chunks_across_the_wide_threshold_give_the_same_bits():
    """300 spots of 128 px: block 1 runs conv2 at 307200 rows (wide), block 2 at 76800 (256-pixel form); with atonce = 100 block 1
    has 102400 rows a chunk (256-pixel form).  The logits must not know."""
    import gridnext_amd as ga
    from oracle import densenet as odn
    torch.manual_seed(5)
    m = ga.DenseNet(num_classes=8, **odn.DENSENET121).to(DEV).eval()
    assert m.winograd
    x = torch.rand(300, 3, 128, 128, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        m.atonce = None
        full = m(x)
        m.atonce = 100
        chunked = m(x)
    assert bool(torch.isfinite(full).all())
    assert torch.equal(full, chunked)
