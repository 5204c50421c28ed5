"""Saturation and hue jitter on the host: the numpy restatement of Pillow's arithmetic (`transforms.rgb_to_hsv_u8`,
`hsv_to_rgb_u8`, `saturate_u8`, `shift_hue_u8`) against the installed Pillow on ALL 2^24 colours, `hue_shifts`, the draw
protocol, the PIL step, `Augment`'s rules, the CPU form of `augment_patches(sat=, hue=)`, the refusals, the C ABI's two names
and the slide datasets on the host.  Every image comparison is np.array_equal / torch.equal; a Pillow whose arithmetic differs
from the restatement fails here, not on the GPU."""
import numpy as np
import pytest
import torch
from PIL import Image

import augment_hs_ref as H
import augment_ref as R
from gridnext_amd import transforms as T


# ---------------------------------------------------------------------------------------------- all 2^24 colours
def test_rgb_to_hsv_is_pillows_on_every_colour():
    got = H.hsv_table()
    want = H.pil_rgb_to_hsv(H.all_colours_hwc()).reshape(-1, 3)
    bad = int((got != want).any(1).sum())
    print("rgb -> hsv: %d of 2^24 colours differ from Pillow" % bad)
    assert got.dtype == np.uint8 and got.shape == (1 << 24, 3) and bad == 0


def test_hsv_to_rgb_is_pillows_on_every_triple():
    got = H.rgb_table()
    want = H.pil_hsv_to_rgb(H.all_colours_hwc()).reshape(-1, 3)
    bad = int((got != want).any(1).sum())
    print("hsv -> rgb: %d of 2^24 triples differ from Pillow" % bad)
    assert got.dtype == np.uint8 and got.shape == (1 << 24, 3) and bad == 0


@pytest.mark.parametrize("f", H.SAT_FACTORS)
def test_saturate_is_imageenhance_color_on_every_colour(f):
    a = H.all_colours_hwc()
    got = H.saturate(a, f)
    bad = int((got != H.pil_saturate(a, f)).any(-1).sum())
    print("saturation %r: %d of 2^24 colours differ from Pillow" % (f, bad))
    assert got.dtype == np.uint8 and bad == 0
    if f == 1.0:
        assert np.array_equal(got, a)
    if f == 0.0:
        assert np.array_equal(got[..., 0], np.array(Image.fromarray(a).convert('L')))


@pytest.mark.parametrize("shift", H.SHIFTS)
def test_hue_shift_is_the_literal_pillow_calls_on_every_colour(shift):
    a = H.all_colours_hwc()
    got = H.table_hue(a, shift)
    bad = int((got != H.pil_hue(a, shift)).any(-1).sum())
    print("hue shift %d: %d of 2^24 colours differ from Pillow" % (shift, bad))
    assert bad == 0
    sample = a[1000:1003]
    assert np.array_equal(T.shift_hue_u8(sample, shift), got[1000:1003])     # the tables are the function
    if shift == 0:
        assert not np.array_equal(got, a)                                    # the round trip alone is lossy


def test_the_kernels_pixel_arithmetic_compiled_for_the_host_equals_the_restatement_on_every_input(tmp_path):
    """csrc/hs_pixel.h is what csrc/augment.hip evaluates per pixel: Pillow's expressions, with fmod(x, 1.0) written as
    x - floor(x) and the per-H / per-S values of HSV -> RGB taken from 256-entry tables.  It is plain C++, so the host compiler
    builds it (tests/hs_pixel_host.cpp) and its bytes are compared with the restatement on all 2^24 colours / triples."""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), 'gridnext_amd', 'csrc')
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    cmd = [cxx] if cxx else [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++']
    exe = str(tmp_path / 'hs_pixel_host')
    # -Wno-unknown-pragmas: a compiler that does not know `#pragma clang fp` takes -ffp-contract=off instead
    subprocess.run(cmd + ['-O2', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas', '-I', csrc,
                          os.path.join(here, 'hs_pixel_host.cpp'), '-o', exe], check=True)
    subprocess.run([exe, str(tmp_path)] + [repr(f) for f in H.SAT_FACTORS], check=True)

    def load(name, shape):
        return np.fromfile(str(tmp_path / name), dtype=np.uint8).reshape(shape)

    bad = [int((load('hsv.bin', (-1, 3)) != H.hsv_table()).any(1).sum()),
           int((load('rgb.bin', (-1, 3)) != H.rgb_table()).any(1).sum())]
    # saturation = the blend of a pixel's grey value with each channel: the grey value on every colour, the blend on every
    # (grey value, channel byte) pair and factor
    a = H.all_colours_hwc().reshape(-1, 3).astype(np.int64)
    bad.append(int((load('grey.bin', -1) != (19595 * a[:, 0] + 38470 * a[:, 1] + 7471 * a[:, 2] + 0x8000) >> 16).sum()))
    L, c = np.arange(256, dtype=np.int64)[:, None], np.arange(256, dtype=np.int64)[None, :]
    for j, f in enumerate(H.SAT_FACTORS):
        bad.append(int((load('sat%d.bin' % j, (256, 256)) != T._blend_u8(L, np.float32(f), c)).sum()))
    print("hs_pixel.h against the restatement, inputs that differ: rgb->hsv %d, hsv->rgb %d, grey %d, blend %r" %
          (bad[0], bad[1], bad[2], bad[3:]))
    assert bad == [0] * (3 + len(H.SAT_FACTORS))


def test_hue_on_random_patches_at_factors_of_both_signs():
    rng = np.random.default_rng(5)
    factors = list(rng.uniform(-0.5, 0.5, 30)) + [-0.5, 0.5, 0.0, -0.1, 0.1, -1e-3, 1e-3]
    assert min(factors) < 0 < max(factors)
    for j, fh in enumerate(factors):
        a = R.hwc(R.patches(1, 1 + j % 9, seed=j)[0])
        shift = T.hue_shifts(fh)
        assert shift.dtype == np.uint8 and int(shift) == H.pil_shift(fh)
        assert np.array_equal(T.shift_hue_u8(a, shift), H.pil_hue(a, H.pil_shift(fh))), fh
    # a shift per patch broadcasts
    x = H.to_hwc(R.patches(4, 3, seed=1))
    shifts = np.array([0, 200, 17, 255], dtype=np.uint8)
    got = T.shift_hue_u8(x, shifts.reshape(-1, 1, 1))
    for k in range(4):
        assert np.array_equal(got[k], H.pil_hue(x[k], int(shifts[k])))


def test_hue_shifts():
    fh = np.array([-0.1, 0.1, -0.5, 0.5, 0.0, -0.0, 0.004, -0.004, -0.003, 0.25, -0.25])
    want = [231, 25, 129, 127, 0, 0, 1, 255, 0, 63, 193]                     # int() truncates toward zero, then & 255
    assert want == [int(f * 255) & 255 for f in fh.tolist()]
    got = T.hue_shifts(fh)
    assert got.dtype == np.uint8 and got.tolist() == want
    assert T.hue_shifts(torch.from_numpy(fh)).tolist() == want and int(T.hue_shifts(-0.1)) == 231


def test_restatement_refuses_what_is_not_rgb_bytes():
    for fn in (T.rgb_to_hsv_u8, T.hsv_to_rgb_u8, lambda a: T.saturate_u8(a, 0.5)):
        with pytest.raises(ValueError, match="uint8"):
            fn(np.zeros((2, 3), dtype=np.float32))
        with pytest.raises(ValueError, match="uint8"):
            fn(np.zeros((3, 2), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------- the step
def test_ranges():
    s = T.SaturationHueJitter(saturation=0.4, hue=0.1)
    assert s.saturation == (0.6, 1.4) and s.hue == (-0.1, 0.1) and s.has_saturation() and s.has_hue()
    assert T.SaturationHueJitter(saturation=2).saturation == (0.0, 3.0)
    assert T.SaturationHueJitter(saturation=(0.5, 0.5), hue=(-0.5, 0.25)).hue == (-0.5, 0.25)
    assert T.SaturationHueJitter(hue=0.5).hue == (-0.5, 0.5)
    neutral = T.SaturationHueJitter()
    assert neutral.is_identity() and not neutral.has_saturation() and not neutral.has_hue()
    assert T.SaturationHueJitter(saturation=(1, 1), hue=(0, 0)).is_identity()
    assert not T.SaturationHueJitter(hue=(0.1, 0.1)).is_identity()
    assert repr(s) == "SaturationHueJitter(saturation=(0.6, 1.4), hue=(-0.1, 0.1))"
    for bad in (dict(hue=0.6), dict(hue=-0.1), dict(hue=(-0.6, 0.1)), dict(hue=(0.2, 0.1)), dict(hue=(0.1, 0.6)),
                dict(hue=(0.1,)), dict(saturation=-0.1), dict(saturation=(1.5, 0.5)), dict(saturation=(-0.1, 1.0)),
                dict(saturation=(1.0, 1.1, 1.2))):
        with pytest.raises(ValueError, match="SaturationHueJitter: .*%s" % list(bad)[0]):
            T.SaturationHueJitter(**bad)


def test_draw_protocol():
    s = T.SaturationHueJitter(saturation=(0.5, 1.5), hue=0.2)
    g = torch.Generator().manual_seed(3)
    f = s.draw(8, g)
    assert f.dtype == torch.float64 and tuple(f.shape) == (8, 2)
    g = torch.Generator().manual_seed(3)                                     # saturation is drawn first, then hue
    fs = 0.5 + 1.0 * torch.rand(8, dtype=torch.float64, generator=g)
    fh = -0.2 + (0.2 - -0.2) * torch.rand(8, dtype=torch.float64, generator=g)
    assert torch.equal(f, torch.stack([fs, fh], 1))
    # nothing is drawn for a constant range
    for step, col, const in ((T.SaturationHueJitter(saturation=(1.3, 1.3), hue=0.2), 0, 1.3),
                             (T.SaturationHueJitter(saturation=0.5, hue=(0.1, 0.1)), 1, 0.1)):
        g = torch.Generator().manual_seed(4)
        f = step.draw(5, g)
        g = torch.Generator().manual_seed(4)
        lo, hi = (step.hue, step.saturation)[col]
        assert torch.equal(f[:, 1 - col], lo + (hi - lo) * torch.rand(5, dtype=torch.float64, generator=g))
        assert torch.equal(f[:, col], torch.full((5,), const, dtype=torch.float64))
    g = torch.Generator().manual_seed(4)
    state = g.get_state()
    T.SaturationHueJitter(saturation=(0.7, 0.7), hue=(0.2, 0.2)).draw(5, g)
    assert torch.equal(g.get_state(), state)
    # n single draws are one draw of n when it is the only drawing step
    single = T.Augment([T.SaturationHueJitter(hue=0.3)], seed=9)
    batch = single.draw_all(40)[2]
    single.manual_seed(9)
    assert torch.equal(torch.cat([single.draw_all(1)[2] for _ in range(40)]), batch)
    two = T.Augment([T.SaturationHueJitter(0.3, 0.3)], seed=9)                # two ranges: step-major against patch-major
    batch = two.draw_all(40)[2]
    two.manual_seed(9)
    assert not torch.equal(torch.cat([two.draw_all(1)[2] for _ in range(40)]), batch)


def test_pil_step_is_the_literal_calls_under_the_global_generator():
    a = R.hwc(R.patches(1, 9, seed=2)[0])
    im = Image.fromarray(a)
    step = T.SaturationHueJitter(saturation=0.6, hue=(-0.5, 0.5))
    seen = set()
    for seed in range(8):
        torch.manual_seed(seed)
        fs = 0.4 + (1.6 - 0.4) * float(torch.rand(1, dtype=torch.float64))
        fh = -0.5 + 1.0 * float(torch.rand(1, dtype=torch.float64))
        torch.manual_seed(seed)
        got = step(im)
        assert got.mode == 'RGB' and np.array_equal(np.array(got), H.pil_sat_hue(a, fs, fh)), seed
        seen.add(fh < 0)
    assert seen == {False, True}
    # an absent stage does no work: no HSV round trip without a hue range, no blend without a saturation range
    torch.manual_seed(1)
    fs = 0.4 + (1.6 - 0.4) * float(torch.rand(1, dtype=torch.float64))
    torch.manual_seed(1)
    assert np.array_equal(np.array(T.SaturationHueJitter(saturation=0.6)(im)), H.pil_saturate(a, fs))
    assert T.SaturationHueJitter()(im) is im
    assert np.array_equal(np.array(T.SaturationHueJitter(hue=(0.1, 0.1))(im)), H.pil_hue(a, 25))
    # a present hue stage makes the round trip at shift 0 too
    zero = np.array(T.SaturationHueJitter(hue=(0.001, 0.001))(im))
    assert np.array_equal(zero, H.pil_hue(a, 0)) and not np.array_equal(zero, a)
    # inside a host Compose, after a ColorJitter and in front of ToTensor
    torch.manual_seed(3)
    t = T.Compose([T.RandomQuarterTurn(), T.ColorJitter(0.2), step, T.ToTensor()])(im)
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 9, 9)
    with pytest.raises(TypeError, match="PIL image"):
        step(torch.zeros(3, 5, 5))
    with pytest.raises(ValueError, match="RGB"):
        step(im.convert('L'))
    c = T.Compose([step, T.ToTensor()])
    assert c.device_plan() is None and 'SaturationHueJitter' in c.device_plan_refusal()


# ---------------------------------------------------------------------------------------------- Augment
def test_augment_acceptance_rules():
    hs, cj = T.SaturationHueJitter(0.2, 0.1), T.ColorJitter(0.1, 0.1)
    for steps in ([hs], [cj, hs], [T.RandomQuarterTurn(), cj, T.RandomHorizontalFlip(), hs, T.RandomVerticalFlip()],
                  [hs, T.RandomQuarterTurn()], [cj, T.RandomQuarterTurn(), hs]):
        aug = T.Augment(steps, seed=0)
        assert aug.hs is hs and repr(hs) in repr(aug)
    assert T.Augment([cj], seed=0).hs is None
    with pytest.raises(ValueError, match="step 2.*second SaturationHueJitter"):
        T.Augment([hs, T.RandomQuarterTurn(), T.SaturationHueJitter(hue=0.1)])
    with pytest.raises(ValueError, match="step 2: ColorJitter.*follows SaturationHueJitter.*colour order is fixed"):
        T.Augment([T.RandomQuarterTurn(), hs, cj])
    with pytest.raises(ValueError, match="second ColorJitter"):
        T.Augment([cj, hs, T.ColorJitter(0.2)])
    with pytest.raises(ValueError, match="step 1.*SaturationHueJitter"):
        T.Augment([hs, T.ToTensor()])
    for kw in (dict(saturation=0.1), dict(hue=0.05)):                        # ColorJitter itself still refuses them
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            T.ColorJitter(**kw)


def test_draw_is_unchanged_without_the_step_and_draw_all_adds_the_third_value():
    old = [T.RandomHorizontalFlip(), T.RandomVerticalFlip(0.3), T.RandomQuarterTurn(), T.ColorJitter(0.4, (0.5, 1.5))]
    aug = T.Augment(old, seed=5)
    codes, factors = aug.draw(8)
    assert codes.tolist() == [1, 6, 6, 5, 5, 4, 7, 1]                       # the protocol tests/test_augment_ref_host.py pins
    again = aug.manual_seed(5).draw_all(8)
    assert len(again) == 3 and torch.equal(again[0], codes) and torch.equal(again[1], factors) and again[2] is None
    # with the step: drawn in list order, between the others
    hs = T.SaturationHueJitter(saturation=(0.5, 1.5), hue=0.25)
    steps = [T.RandomHorizontalFlip(), T.ColorJitter(0.4), hs, T.RandomQuarterTurn()]
    aug = T.Augment(steps, seed=7)
    codes, factors, f = aug.draw_all(6)
    g = torch.Generator().manual_seed(7)
    h = (torch.rand(6, dtype=torch.float64, generator=g) < 0.5).long() * 4
    fb = 0.6 + (1.4 - 0.6) * torch.rand(6, dtype=torch.float64, generator=g)
    fs = 0.5 + 1.0 * torch.rand(6, dtype=torch.float64, generator=g)
    fh = -0.25 + 0.5 * torch.rand(6, dtype=torch.float64, generator=g)
    r = torch.randint(0, 4, (6,), generator=g)
    assert torch.equal(codes, torch.from_numpy(T.D4)[h, r])
    assert torch.equal(factors, torch.stack([torch.ones(6, dtype=torch.float64), fb], 1))
    assert f.dtype == torch.float64 and torch.equal(f, torch.stack([fs, fh], 1))
    state = aug.generator.get_state()
    two = aug.manual_seed(7).draw(6)                                         # draw: the first two, the generator consumed alike
    assert len(two) == 2 and torch.equal(two[0], codes) and torch.equal(two[1], factors)
    assert torch.equal(aug.generator.get_state(), state)
    # an identity step gives None, and draws nothing
    aug = T.Augment([T.SaturationHueJitter(), T.RandomQuarterTurn()], seed=2)
    g = torch.Generator().manual_seed(2)
    codes, factors, f = aug.draw_all(5)
    assert f is None and factors is None and torch.equal(codes, torch.randint(0, 4, (5,), generator=g).to(torch.uint8))


def test_augment_patches_on_cpu_tensors_is_pillow():
    n, P = 11, 7
    x = R.patches(n, P, seed=4)
    keep = x.clone()
    codes = R.scrambled_codes(n, seed=5)
    rng = np.random.default_rng(6)
    factors = rng.uniform(0.3, 1.8, (n, 2))
    fs, fh = rng.uniform(0.0, 2.5, n), rng.uniform(-0.5, 0.5, n)
    fs[:3] = (0.0, 1.0, 1.0 - 1e-7)
    tables = T.color_tables(factors, T.contrast_means(T.grey_sums(x), P))
    hue = T.hue_shifts(fh)
    for use_sat, use_hue, use_tab in ((1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0), (0, 0, 1)):
        got = T.augment_patches(x, codes, tables if use_tab else None, sat=fs if use_sat else None, hue=hue if use_hue else None)
        for k in range(n):
            a = R.hwc(x[k])                                                 # turn -> table -> Pillow
            a = R.pil_jitter(a, factors[k, 0], factors[k, 1]) if use_tab else a
            a = H.pil_sat_hue(a, float(np.float32(fs[k])) if use_sat else None, fh[k] if use_hue else None)
            assert np.array_equal(R.hwc(got[k]), R.pil_code(a, int(codes[k]))), (use_sat, use_hue, use_tab, k)
    assert torch.equal(T.augment_patches(x, codes, tables, sat=None, hue=None), T.augment_patches(x, codes, tables))
    # float32 and float64 factors, tensors and arrays: one result
    want = T.augment_patches(x, codes, tables, sat=fs, hue=hue)
    for s in (fs.astype(np.float32), torch.from_numpy(fs), torch.from_numpy(fs).float()):
        assert torch.equal(T.augment_patches(x, codes, tables, sat=s, hue=torch.from_numpy(hue)), want)
    # the float form and a scatter
    rows = np.array([3, 0, -1, 12, 7, 13, 1, 5, 2, 9, 4], dtype=np.int32)
    out = torch.full((13, 3, P, P), 7.0)
    assert T.augment_patches(x, codes, tables, out=out, out_rows=rows, out_float=True, norm=R.NORM, sat=fs, hue=hue) is out
    mean, std = (torch.tensor(v).reshape(3, 1, 1) for v in R.NORM)
    for k in range(n):
        if 0 <= rows[k] < 13:
            assert torch.equal(out[rows[k]], (want[k].float().div(255) - mean) / std), k
    for row in set(range(13)) - set(rows.tolist()):
        assert bool((out[row] == 7.0).all())
    assert torch.equal(x, keep)
    assert tuple(T.augment_patches(x[:0], sat=np.zeros(0), hue=np.zeros(0, dtype=np.uint8)).shape) == (0, 3, P, P)


def test_augment_apply_on_the_host_is_the_pil_steps():
    x = R.patches(9, 6, seed=8)
    hs = T.SaturationHueJitter(0.5, 0.3)
    aug = T.Augment([T.RandomVerticalFlip(), T.ColorJitter(0.3, 0.6), T.RandomQuarterTurn(), hs], seed=11)
    got = aug.apply(x)
    codes, factors, f = aug.manual_seed(11).draw_all(9)
    for k in range(9):
        a = R.pil_jitter(R.hwc(x[k]), float(factors[k, 0]), float(factors[k, 1]))
        a = H.pil_sat_hue(a, float(np.float32(float(f[k, 0]))), float(f[k, 1]))
        assert np.array_equal(R.hwc(got[k]), R.pil_code(a, int(codes[k]))), k
    assert not torch.equal(aug.apply(x), got) and torch.equal(aug.manual_seed(11).apply(x), got)
    # an absent stage is not passed on: a saturation-only step equals the blend alone
    only = T.Augment([T.SaturationHueJitter(saturation=0.5)], seed=3)
    f = only.draw_all(9)[2]
    assert torch.equal(only.manual_seed(3).apply(x), T.augment_patches(x, sat=f[:, 0].contiguous()))
    assert torch.equal(T.Augment([T.SaturationHueJitter()], seed=3).apply(x), x)


def test_refusals():
    x = R.patches(2, 4, seed=0)
    ok_s, ok_h = np.ones(2, dtype=np.float32), np.zeros(2, dtype=np.uint8)
    for bad in (np.ones(3, dtype=np.float32), np.ones((2, 1), dtype=np.float32), np.ones(2, dtype=np.int32),
                torch.ones(2, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="sat"):
            T.augment_patches(x, sat=bad, hue=ok_h)
    for bad in (np.zeros(3, dtype=np.uint8), np.zeros((1, 2), dtype=np.uint8), np.zeros(2, dtype=np.int64),
                np.zeros(2, dtype=np.float32), torch.zeros(2, dtype=torch.int8)):
        with pytest.raises(ValueError, match="hue"):
            T.augment_patches(x, sat=ok_s, hue=bad)
    with pytest.raises(ValueError, match="uint8"):
        T.augment_patches(x.float(), sat=ok_s)
    with pytest.raises(ValueError, match="square"):
        T.augment_patches(torch.zeros((2, 3, 4, 5), dtype=torch.uint8), hue=ok_h)
    with pytest.raises(ValueError, match="out"):
        T.augment_patches(x, out=torch.zeros((2, 3, 4, 4)), sat=ok_s)
    with pytest.raises(ValueError, match="uint8"):
        T.Augment([T.SaturationHueJitter(0.1)]).apply(x.float())


def test_header_signatures_and_library_agree_on_the_two_names():
    import ctypes
    from gridnext_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (('gnx_patch_augment_hs_u8', 11), ('gnx_patch_augment_hs_u8_f32', 12)):
        assert name in _lib.PARAMS, "%s is not declared in the header" % name
        params = _lib.PARAMS[name]
        assert len(params) == nargs == len(_lib.SIGNATURES[name][1]) and params[-1] == 'stream'
        assert params[:10] == ['src', 'dst', 'n', 'P', 'dst_n', 'codes', 'luts', 'sat', 'hue', 'dst_rows']
        assert hasattr(handle, name)
    old = _lib.PARAMS['gnx_patch_augment_u8']
    assert [p for p in _lib.PARAMS['gnx_patch_augment_hs_u8'] if p not in ('sat', 'hue')] == old
    assert _lib.PARAMS['gnx_patch_augment_hs_u8_f32'][10] == 'norm'
    assert text.count('image_datasets.py:102-105') >= 2 and text.count(':184-187') >= 2


def test_slide_datasets_on_the_host_with_the_step(tmp_path):
    """device=None: the datasets route through `Augment.apply`, so they get the step with no change of their own; an epoch
    differs from the next, and re-seeding reproduces it."""
    import gridnext_amd as ga
    from slide_fixture import SLIDE, SR1, SR2, write_annots
    annots = write_annots(tmp_path)
    steps = [T.RandomHorizontalFlip(), T.ColorJitter(0.3, 0.5), T.RandomQuarterTurn(), T.SaturationHueJitter(0.4, 0.2)]
    args = ([SLIDE, SLIDE], [SR1, SR2], annots)
    aug = T.Augment(steps, seed=3)
    grid = ga.SlideGridDataset(*args, patch_size=8, window_size=12, augment=aug)
    pats = ga.SlidePatchDataset(*args, patch_size=8, window_size=12, augment=aug)
    idx = [17, 2, 9, 2, 0, 18]

    def epoch():
        return [grid[i][0].clone() for i in range(2)] + [b[0].clone() for b in pats.__getitems__(idx)]

    first, second = epoch(), epoch()
    assert all(not torch.equal(a, b) for a, b in zip(first, second))
    aug.manual_seed(3)
    assert all(torch.equal(a, b) for a, b in zip(first, epoch()))
    # against the same list without the step: the step changes the bytes, the geometry and the labels stay
    plain = ga.SlideGridDataset(*args, patch_size=8, window_size=12, augment=T.Augment(steps[:3], seed=3))
    assert not torch.equal(plain[0][0], first[0]) and torch.equal(plain[0][1], grid[0][1])
    assert torch.equal(plain[0][0].flatten(2).any(2), first[0].flatten(2).any(2))
