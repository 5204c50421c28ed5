"""Train-time augmentation on the host: the codes, the composition table, the colour tables, the grey sums, the draw protocol,
the PIL steps and the CPU form of `augment_patches` against Pillow itself (tests/augment_ref.py); the refusals; the C ABI's
three names.  Every image comparison is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch
from PIL import Image

import augment_ref as R
from gridnext_amd import transforms as T


def _asym():
    """An asymmetric 5 x 5 RGB patch: every pixel and channel its own value."""
    return np.arange(75, dtype=np.uint8).reshape(5, 5, 3) * 3 + 1


def test_the_eight_codes_are_pillows_transposes():
    a = _asym()
    x = R.chw(a)[None]
    seen = set()
    for code in range(8):
        want = R.pil_code(a, code)
        seen.add(want.tobytes())
        assert np.array_equal(R.hwc(R.torch_code(x, code)[0]), want), code
        assert np.array_equal(R.hwc(T.augment_patches(x, np.array([code], dtype=np.uint8))[0]), want), code
        assert np.array_equal(R.hwc(T.augment_patches(x, np.array([code + 8 * 13], dtype=np.uint8))[0]), want), code
        assert T.PIL_TRANSPOSE[code] == R.PIL_OPS[code]
    assert len(seen) == 8
    assert torch.equal(T.augment_patches(x), x)


def test_composition_table_against_the_sequential_ops():
    x = R.chw(_asym())[None]
    assert T.D4.shape == (8, 8) and T.D4.dtype == np.uint8
    for c1 in range(8):
        assert sorted(T.D4[c1].tolist()) == list(range(8)) and T.D4[0, c1] == c1 == T.D4[c1, 0]
        for c2 in range(8):
            assert torch.equal(R.torch_code(R.torch_code(x, c1), c2), R.torch_code(x, int(T.D4[c1, c2]))), (c1, c2)


def test_grey_sums_are_pillows_convert_l():
    for P in (1, 3, 17, 32):
        x = R.patches(5, P, seed=P)
        x[1] = 255
        x[2] = 0
        sums = T.grey_sums(x)
        assert sums.dtype == np.int64 and sums[1] == 255 * P * P and sums[2] == 0
        for k in range(5):
            assert int(sums[k]) == R.pil_grey_sum(R.hwc(x[k])), (P, k)


@pytest.mark.parametrize("P", [1, 3, 17, 32])
def test_color_tables_are_imageenhance(P):
    rng = np.random.default_rng(100 + P)
    factors = list(rng.uniform(0.0, 2.0, 40)) + list(R.FIXED_FACTORS)
    bad = cases = 0
    for j, f in enumerate(factors):
        for constant in (False, True):
            x = R.patches(1, P, seed=1000 * P + j)
            if constant:
                x[:] = x[:, :, :1, :1]
            a = R.hwc(x[0])
            other = factors[(j * 7 + 3) % len(factors)]
            means = T.contrast_means(T.grey_sums(x), P)
            for fc, fb in ((f, 1.0), (1.0, f), (f, other)):
                table = T.color_tables(np.array([[fc, fb]]), means)
                assert table.shape == (1, 3, 256) and table.dtype == np.uint8
                got = R.hwc(T.augment_patches(x, None, table)[0])
                cases += 1
                bad += not np.array_equal(got, R.pil_jitter(a, fc, fb))
    print("P = %d: %d of %d cases differ from ImageEnhance" % (P, bad, cases))
    assert bad == 0


def test_color_tables_without_contrast_need_no_means():
    t = T.color_tables(np.array([[1.0, 1.0], [1.0, 0.5]]))
    assert np.array_equal(t[0, 1], np.arange(256)) and np.array_equal(t[1, 2], np.arange(256) // 2)
    with pytest.raises(ValueError, match="grey means"):
        T.color_tables(np.array([[0.9, 1.0]]))


def test_draw_protocol():
    steps = [T.RandomHorizontalFlip(), T.RandomVerticalFlip(0.3), T.RandomQuarterTurn(), T.ColorJitter(0.4, (0.5, 1.5))]
    aug = T.Augment(steps, seed=5)
    codes, factors = aug.draw(8)
    assert codes.dtype == torch.uint8 and factors.dtype == torch.float64 and tuple(factors.shape) == (8, 2)
    assert codes.tolist() == [1, 6, 6, 5, 5, 4, 7, 1]                       # the fixed protocol under seed 5
    # restated: one call per step for the whole batch, in the order listed; contrast before brightness
    g = torch.Generator().manual_seed(5)
    h = (torch.rand(8, dtype=torch.float64, generator=g) < 0.5).long() * 4
    v = (torch.rand(8, dtype=torch.float64, generator=g) < 0.3).long() * 6
    r = torch.randint(0, 4, (8,), generator=g)
    d4 = torch.from_numpy(T.D4)
    assert torch.equal(codes, d4[d4[h, v].long(), r])
    fc = 0.5 + 1.0 * torch.rand(8, dtype=torch.float64, generator=g)
    fb = 0.6 + (1.4 - 0.6) * torch.rand(8, dtype=torch.float64, generator=g)
    assert torch.equal(factors, torch.stack([fc, fb], 1))
    assert torch.equal(aug.manual_seed(5).draw(8)[0], codes) and not torch.equal(aug.draw(8)[0], codes)
    # a degenerate range draws nothing; an identity jitter gives no factors
    one = T.Augment([T.ColorJitter(brightness=(1.2, 1.2), contrast=0.5)], seed=2)
    g = torch.Generator().manual_seed(2)
    assert torch.equal(one.draw(4)[1], torch.stack([0.5 + 1.0 * torch.rand(4, dtype=torch.float64, generator=g),
                                                    torch.full((4,), 1.2, dtype=torch.float64)], 1))
    assert T.Augment([T.RandomQuarterTurn(), T.ColorJitter()], seed=0).draw(3)[1] is None
    assert T.Augment([T.RandomQuarterTurn()], seed=0).draw(3)[1] is None
    # n = 1 repeated against one batch: equal with ONE drawing step, step-major against patch-major with several
    single = T.Augment([T.RandomQuarterTurn()], seed=9)
    batch = single.draw(40)[0]
    single.manual_seed(9)
    assert torch.equal(torch.cat([single.draw(1)[0] for _ in range(40)]), batch)
    two = T.Augment([T.RandomHorizontalFlip(), T.RandomQuarterTurn()], seed=9)
    batch = two.draw(40)[0]
    two.manual_seed(9)
    assert not torch.equal(torch.cat([two.draw(1)[0] for _ in range(40)]), batch)
    assert tuple(T.Augment([], seed=1).draw(0)[0].shape) == (0,)


def test_pil_steps_draw_from_the_global_generator():
    a = _asym()
    im = Image.fromarray(a)
    for step, op in ((T.RandomHorizontalFlip(0.5), 4), (T.RandomVerticalFlip(0.5), 6)):
        seen = set()
        for seed in range(12):
            torch.manual_seed(seed)
            hit = bool(torch.rand(1, dtype=torch.float64) < 0.5)
            torch.manual_seed(seed)
            got = np.array(step(im))
            assert np.array_equal(got, R.pil_code(a, op if hit else 0)), (step, seed)
            seen.add(hit)
        assert seen == {False, True}
        assert np.array_equal(np.array(type(step)(1.0)(im)), R.pil_code(a, op))
        assert np.array_equal(np.array(type(step)(0.0)(im)), a)
    turns = set()
    for seed in range(12):
        torch.manual_seed(seed)
        r = int(torch.randint(0, 4, (1,)))
        torch.manual_seed(seed)
        assert np.array_equal(np.array(T.RandomQuarterTurn()(im)), R.pil_code(a, r))
        turns.add(r)
    assert turns == {0, 1, 2, 3}
    jitter = T.ColorJitter(brightness=0.4, contrast=(0.5, 1.5))
    assert jitter.brightness == (0.6, 1.4) and jitter.contrast == (0.5, 1.5) and T.ColorJitter(brightness=2).brightness == (0.0, 3.0)
    for seed in range(6):
        torch.manual_seed(seed)
        fc = 0.5 + 1.0 * float(torch.rand(1, dtype=torch.float64))
        fb = 0.6 + (1.4 - 0.6) * float(torch.rand(1, dtype=torch.float64))
        torch.manual_seed(seed)
        assert np.array_equal(np.array(jitter(im)), R.pil_jitter(a, fc, fb)), seed
    # inside a host Compose, in front of ToTensor
    torch.manual_seed(3)
    t = T.Compose([T.RandomQuarterTurn(), T.RandomHorizontalFlip(), jitter, T.ToTensor()])(im)
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 5, 5)
    with pytest.raises(TypeError, match="PIL image"):
        T.RandomQuarterTurn()(torch.zeros(3, 5, 5))


def test_augment_patches_on_cpu_tensors_is_pillow():
    n, P = 11, 7
    x = R.patches(n, P, seed=4)
    keep = x.clone()
    codes = R.scrambled_codes(n, seed=5)
    factors = np.random.default_rng(6).uniform(0.3, 1.8, (n, 2))
    tables = T.color_tables(factors, T.contrast_means(T.grey_sums(x), P))
    got = T.augment_patches(x, codes, tables)
    for k in range(n):
        want = R.pil_code(R.pil_jitter(R.hwc(x[k]), factors[k, 0], factors[k, 1]), int(codes[k]))
        assert np.array_equal(R.hwc(got[k]), want), k
    # the float form, a scatter into a larger sentinel-filled buffer, rows outside it skipped
    rows = np.array([3, 0, -1, 12, 7, 13, 1, 5, 2, 9, 4], dtype=np.int32)
    out = torch.full((13, 3, P, P), 7.0)
    r = T.augment_patches(x, codes, tables, out=out, out_rows=rows, out_float=True, norm=R.NORM)
    assert r is out
    mean, std = (torch.tensor(v).reshape(3, 1, 1) for v in R.NORM)
    for k in range(n):
        if 0 <= rows[k] < 13:
            assert torch.equal(out[rows[k]], (got[k].float().div(255) - mean) / std), k
    for row in set(range(13)) - set(rows.tolist()):
        assert bool((out[row] == 7.0).all())
    assert torch.equal(T.augment_patches(x, codes, None, out_float=True), T.augment_patches(x, codes).float().div(255))
    grid = torch.zeros((3, 5, 3, P, P), dtype=torch.uint8)
    T.augment_patches(x, codes, out=grid, out_rows=np.arange(n, dtype=np.int32) + 2)
    assert torch.equal(grid.view(15, 3, P, P)[2:13], T.augment_patches(x, codes)) and not grid.view(15, 3, P, P)[:2].any()
    assert torch.equal(x, keep)


def test_augment_apply_on_the_host_is_the_pil_steps():
    x = R.patches(9, 6, seed=8)
    aug = T.Augment([T.RandomVerticalFlip(), T.RandomQuarterTurn(), T.ColorJitter(0.3, 0.6)], seed=11)
    got = aug.apply(x)
    codes, factors = aug.manual_seed(11).draw(9)
    for k in range(9):
        want = R.pil_code(R.pil_jitter(R.hwc(x[k]), float(factors[k, 0]), float(factors[k, 1])), int(codes[k]))
        assert np.array_equal(R.hwc(got[k]), want), k
    assert not torch.equal(aug.apply(x), got) and torch.equal(aug.manual_seed(11).apply(x), got)


def test_a_compose_with_a_new_step_has_no_device_plan():
    for step in (T.RandomHorizontalFlip(), T.RandomVerticalFlip(), T.RandomQuarterTurn(), T.ColorJitter(0.1, 0.1)):
        for steps in ([step, T.ToTensor()], [T.Resize(8), step, T.ToTensor()], [T.ToTensor(), step]):
            c = T.Compose(steps)
            assert c.device_plan() is None and type(step).__name__ in c.device_plan_refusal()


def test_refusals():
    x = R.patches(2, 4, seed=0)
    with pytest.raises(ValueError, match="square"):
        T.augment_patches(torch.zeros((2, 3, 4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="square"):
        T.augment_patches(torch.zeros((2, 1, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        T.augment_patches(x.float())
    with pytest.raises(ValueError, match="codes"):
        T.augment_patches(x, np.zeros(3, dtype=np.uint8))
    with pytest.raises(ValueError, match="tables"):
        T.augment_patches(x, None, np.zeros((2, 3, 255), dtype=np.uint8))
    with pytest.raises(ValueError, match="out"):
        T.augment_patches(x, out_rows=np.zeros(2, dtype=np.int32))
    with pytest.raises(ValueError, match="out"):
        T.augment_patches(x, out=torch.zeros((1, 3, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        T.augment_patches(x, out=torch.zeros((2, 3, 4, 4)))
    with pytest.raises(ValueError, match="uint8"):
        T.Augment([T.RandomQuarterTurn()]).apply(x.float())
    with pytest.raises(ValueError, match="second ColorJitter"):
        T.Augment([T.ColorJitter(0.1), T.RandomQuarterTurn(), T.ColorJitter(0.2)])
    for kw in (dict(saturation=0.1), dict(hue=0.05), dict(saturation=(0.5, 1.5)), dict(hue=(-0.1, 0.1))):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            T.ColorJitter(**kw)
    T.ColorJitter(saturation=0, hue=0)
    for foreign in (T.ToTensor(), T.Resize(8), T.Normalize(*R.NORM), (lambda im: im)):
        with pytest.raises(ValueError, match="step 1"):
            T.Augment([T.RandomQuarterTurn(), foreign])
    with pytest.raises(ValueError):
        T.RandomHorizontalFlip(1.5)
    with pytest.raises(ValueError):
        T.ColorJitter(brightness=-0.1)
    import gridnext_amd as ga
    from slide_fixture import SLIDE, SR1
    with pytest.raises(TypeError, match="Augment"):
        ga.SlideGridDataset([SLIDE], [SR1], patch_size=8, augment=T.RandomQuarterTurn())


def test_header_signatures_and_library_agree_on_the_three_names():
    import ctypes
    from gridnext_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (('gnx_patch_augment_u8', 9), ('gnx_patch_augment_u8_f32', 10), ('gnx_patch_grey_sum_u8', 5)):
        assert name in _lib.PARAMS, "%s is not declared in the header" % name
        params = _lib.PARAMS[name]
        assert len(params) == nargs == len(_lib.SIGNATURES[name][1]) and params[-1] == 'stream'
        assert hasattr(handle, name)
    assert _lib.SIGNATURES['gnx_patch_augment_u8_f32'][1][:8] == _lib.SIGNATURES['gnx_patch_augment_u8'][1][:8]
    assert 'image_datasets.py:102-105' in text and ':184-187' in text


def test_slide_datasets_on_the_host_with_an_augment(tmp_path):
    """device=None: the items are `Augment.apply` of the unaugmented items' bytes, drawn once per in-tissue spot in the spot
    table's order (grid) or once per slide of a batch (patches); cells without a spot stay zero; the float form is the dataset's
    transform of the augmented bytes."""
    import gridnext_amd as ga
    from gridnext_amd import imgprocess as IP
    from slide_fixture import SLIDE, SR1, SR2, write_annots
    annots = write_annots(tmp_path)
    steps = [T.RandomHorizontalFlip(), T.RandomQuarterTurn(), T.ColorJitter(0.3, 0.5)]
    args = ([SLIDE, SLIDE], [SR1, SR2], annots)
    norm = T.Compose([T.ToTensor(), T.Normalize(*R.NORM)])
    for kw in (dict(), dict(remove_cast=True), dict(raw_uint8=False, img_transforms=norm)):
        plain = ga.SlideGridDataset(*args, patch_size=8, window_size=12, **{**kw, 'raw_uint8': True, 'img_transforms': None})
        ds = ga.SlideGridDataset(*args, patch_size=8, window_size=12, augment=T.Augment(steps, seed=3), **kw)
        twin = T.Augment(steps, seed=3)
        for i, srd in enumerate((SR1, SR2)):
            (g, l), (g0, l0) = ds[i], plain[i]
            spots = IP._spot_table(srd, 47, 61).astype(np.int64)
            want = torch.zeros((78 * 64, 3, 8, 8), dtype=torch.float32 if 'img_transforms' in kw else torch.uint8)
            twin.apply(g0[spots[:, 2], spots[:, 3]], out=want, out_rows=(spots[:, 2] * 64 + spots[:, 3]).astype(np.int32),
                       out_float='img_transforms' in kw, norm=R.NORM if 'img_transforms' in kw else None)
            assert g.dtype == want.dtype and torch.equal(g, want.view(78, 64, 3, 8, 8)) and torch.equal(l, l0), (kw, i)
            empty = torch.ones((78, 64), dtype=torch.bool)
            empty[spots[:, 2], spots[:, 3]] = False
            assert not g[empty].any() and not torch.equal(g.to(g0.dtype), g0)
    pd = ga.SlidePatchDataset(*args, patch_size=8, window_size=12, augment=T.Augment(steps, seed=4))
    p0 = ga.SlidePatchDataset(*args, patch_size=8, window_size=12)
    idx = [17, 2, 9, 2, 0, 18]
    batch = pd.__getitems__(idx)
    twin = T.Augment(steps, seed=4)
    first = [b for b in range(6) if pd.items[idx[b]][0] == 0]
    second = [b for b in range(6) if pd.items[idx[b]][0] == 1]
    assert first and second
    for group in (first, second):                                           # one draw per slide of the batch, in batch order
        want = twin.apply(torch.stack([p0[idx[b]][0] for b in group]))
        for j, b in enumerate(group):
            assert torch.equal(batch[b][0], want[j]) and int(batch[b][1]) == int(p0[idx[b]][1])
