"""The tutorial transform on the host (no GPU):
 * tests/resize_ref.py - the numpy restatement of Pillow's fixed-point BILINEAR resize that gnx_resize_crop_u8 implements -
   equals Pillow bit for bit over a grid of geometries and byte patterns;
 * gridnext_amd.transforms.axis_tables (the tables the kernel reads) equals the restatement's, window by window;
 * the five transforms compute what torchvision's compute on PIL images; device_plan recognises exactly
   [Resize] [CenterCrop] ToTensor [Normalize];
 * the datasets: raw_uint8 + such a Compose decode only and carry the transform; everything else is unchanged;
 * header, ctypes table and library agree on the new symbols."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as R
from gridnext_amd import transforms as T


# (H0, W0, Hr, Wr)
GEOMETRIES = [
    (260, 260, 256, 256),        # the tutorial: a slight reduction
    (300, 300, 256, 256),
    (64, 64, 128, 128),          # upscaling
    (37, 41, 16, 17),            # H0 != W0, odd sizes
    (129, 257, 64, 127),         # non-square, Resize(64)'s own shape
    (41, 41, 40, 40),            # a one-pixel reduction
    (40, 40, 41, 41),            # a one-pixel enlargement
    (50, 60, 50, 45),            # one unchanged axis (vertical pass skipped)
    (60, 50, 45, 50),            # ... (horizontal pass skipped)
    (127, 255, 16, 32),          # a reduction just below 8x on both axes (7.94, 7.97: ksize 17)
    (120, 90, 31, 23),           # 3.9x
    (33, 20, 70, 25),            # up on one axis, up on the other by a different factor
]


@pytest.mark.parametrize("H0,W0,Hr,Wr", GEOMETRIES)
def test_restatement_equals_pillow_bit_for_bit(H0, W0, Hr, Wr):
    pats = R.patterns((2, 3, H0, W0), seed=H0 * 1000 + W0)
    pats['constant'] = np.full((2, 3, H0, W0), 77, dtype=np.uint8)
    for name, x in pats.items():
        got = R.resize_crop_u8(x, (Hr, Wr), None)
        want = R.pillow_resize_crop(x, (Hr, Wr), None)
        assert got.shape == (2, 3, Hr, Wr)
        assert np.array_equal(got, want), "%s: %d bytes differ" % (name, int((got != want).sum()))
    # flat images stay flat (an all-zero background stays all-zero: skip_empty still finds it after a resize)
    assert not R.resize_crop_u8(pats['zeros'], (Hr, Wr), None).any()
    assert (R.resize_crop_u8(pats['full'], (Hr, Wr), None) == 255).all()
    assert (R.resize_crop_u8(pats['constant'], (Hr, Wr), None) == 77).all()


def test_restatement_with_crop_equals_pillow():
    for (H0, W0), resize, crop in (((260, 260), 256, 224), ((129, 257), 64, 64), ((224, 224), None, 201), ((37, 41), 16, 12)):
        x = R.patterns((2, 3, H0, W0), seed=3)['random']
        assert np.array_equal(R.resize_crop_u8(x, resize, crop), R.pillow_resize_crop(x, resize, crop))


@pytest.mark.parametrize("H0,W0,Hr,Wr", GEOMETRIES)
def test_axis_tables_equal_the_restatement(H0, W0, Hr, Wr):
    for n_in, n_out in ((W0, Wr), (H0, Hr)):
        coef, bnd = T.axis_tables(n_in, n_out)
        assert coef.dtype == np.int32 and bnd.dtype == np.int32 and coef.flags['C_CONTIGUOUS']
        if n_in == n_out:                       # identity: one tap of 2^22 at the index itself (the pass returns its input)
            assert T.axis_ksize(n_in, n_out) == 1 and coef.shape == (n_out, 1) and (coef == 1 << 22).all()
            assert np.array_equal(bnd, np.stack([np.arange(n_out), np.ones(n_out)], 1))
            continue
        kk, bb = R.coeffs(n_in, n_out)
        assert T.axis_ksize(n_in, n_out) == R.ksize(n_in, n_out) == coef.shape[1] <= T.MAX_KSIZE
        assert np.array_equal(coef, kk) and np.array_equal(bnd, bb)
        assert (bnd[:, 0] >= 0).all() and (bnd[:, 0] + bnd[:, 1] <= n_in).all() and (bnd[:, 1] >= 1).all()
        assert (np.diff(bnd[:, 0]) >= 0).all() and (np.diff(bnd[:, 0] + bnd[:, 1]) >= 0).all()    # a tile's rows: first .. last
        # 255 (2^22 + ksize) + 2^21 < 2^31: the accumulator fits 32 bits
        assert 255 * int(coef.astype(np.int64).sum(1).max()) + (1 << 21) < 2 ** 31
        lo, n = n_out // 3, n_out - n_out // 3 - 1              # a window's tables are the rows of the full ones
        cw, bw = T.axis_tables(n_in, n_out, lo, n)
        assert np.array_equal(cw, coef[lo:lo + n]) and np.array_equal(bw, bnd[lo:lo + n])
    with pytest.raises(ValueError):
        T.axis_tables(W0, Wr, 1, Wr)
    assert T.axis_ksize(1000, 125) == 17 and T.axis_ksize(1001, 125) == 19      # 8x is the last ksize the kernel takes


def _pil(H, W, seed=0):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8))


def test_resize_short_edge_rule_and_shapes():
    assert T.resized_shape(129, 257, 64) == (64, 127)          # int(64 * 257 / 129) = int(127.5)
    assert T.resized_shape(257, 129, 64) == (127, 64)
    assert T.resized_shape(100, 100, 64) == (64, 64)
    assert T.resized_shape(64, 100, 64) == (64, 100)           # the short edge already has the size: unchanged
    assert T.resized_shape(129, 257, (30, 40)) == (30, 40)
    assert T.resized_shape(129, 257, None) == (129, 257)
    img = _pil(129, 257)
    out = T.Resize(64)(img)
    assert out.size == (127, 64)
    assert np.array_equal(np.asarray(out), np.asarray(img.resize((127, 64), Image.BILINEAR)))
    assert T.Resize((30, 40))(img).size == (40, 30)
    assert T.Resize(129)(img) is img
    T.Resize(64, interpolation=Image.BILINEAR)
    T.Resize(64, interpolation='bilinear')
    for bad in (Image.NEAREST, Image.BICUBIC, Image.LANCZOS, 'nearest'):
        with pytest.raises(NotImplementedError):
            T.Resize(64, interpolation=bad)
    with pytest.raises(TypeError):
        T.Resize(64)(torch.zeros(3, 8, 8))


def test_center_crop_offsets_round_half_to_even():
    # margin 23 -> 11.5 -> 12; margin 21 -> 10.5 -> 10; margin 1 -> 0.5 -> 0 (Python's round)
    assert T.crop_window(224, 224, 201) == (12, 12, 201, 201)
    assert T.crop_window(222, 223, 201)[:2] == (10, 11)
    assert T.crop_window(9, 9, 8)[:2] == (0, 0)
    assert T.crop_window(50, 60, None) == (0, 0, 50, 60)
    img = _pil(224, 224, 1)
    out = T.CenterCrop(201)(img)
    assert np.array_equal(np.asarray(out), np.asarray(img)[12:213, 12:213])
    out = T.CenterCrop((10, 20))(img)
    assert out.size == (20, 10) and np.array_equal(np.asarray(out), np.asarray(img)[107:117, 102:122])
    with pytest.raises(ValueError, match="larger"):
        T.CenterCrop(225)(img)
    with pytest.raises(ValueError, match="larger"):
        T.transform_geometry(40, 40, 32, 33)
    assert T.transform_geometry(260, 260, 256, 224) == (256, 256, 16, 16, 224, 224)
    assert T.transform_geometry(129, 257, 64, 64) == (64, 127, 0, 32, 64, 64)


def test_to_tensor_normalize_against_torch():
    img = _pil(17, 23, 2)
    t = T.ToTensor()(img)
    want = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255)
    assert t.dtype == torch.float32 and torch.equal(t, want)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    n = T.Normalize(mean, std)(t)
    assert torch.equal(n, (want - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1))
    with pytest.raises(TypeError):
        T.Normalize(mean, std)(img)
    with pytest.raises(ValueError):
        T.Normalize(mean, (1.0, 0.0, 1.0))
    full = T.Compose([T.Resize(16), T.CenterCrop(12), T.ToTensor(), T.Normalize(mean, std)])(img)
    ref = R.pillow_resize_crop(np.asarray(img).transpose(2, 0, 1)[None], 16, 12)[0]
    ref = (torch.from_numpy(ref).float().div(255) - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    assert torch.equal(full, ref)


def test_device_plan_recognition_and_refusals():
    mean, std = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)
    C = T.Compose
    assert C([T.Resize(256), T.CenterCrop(224), T.ToTensor(), T.Normalize(mean, std)]).device_plan() == (256, 224, (mean, std))
    assert C([T.Resize((30, 40)), T.ToTensor()]).device_plan() == ((30, 40), None, None)
    assert C([T.CenterCrop(201), T.ToTensor()]).device_plan() == (None, 201, None)
    assert C([T.CenterCrop((10, 20)), T.ToTensor()]).device_plan() == (None, (10, 20), None)
    assert C([T.ToTensor()]).device_plan() == (None, None, None)
    assert C([T.ToTensor(), T.Normalize(mean, std)]).device_plan() == (None, None, (mean, std))
    assert C([T.ToTensor()]).device_plan_refusal() is None
    refused = {
        'order': C([T.CenterCrop(8), T.Resize(16), T.ToTensor()]),
        'no ToTensor': C([T.Resize(16), T.CenterCrop(8)]),
        'empty': C([]),
        'two resizes': C([T.Resize(16), T.Resize(8), T.ToTensor()]),
        'norm first': C([T.Normalize(mean, std), T.ToTensor()]),
        'after ToTensor': C([T.ToTensor(), T.CenterCrop(8)]),
        'two norms': C([T.ToTensor(), T.Normalize(mean, std), T.Normalize(mean, std)]),
        'foreign step': C([T.Resize(16), (lambda img: img), T.ToTensor()]),
        'one channel': C([T.ToTensor(), T.Normalize((0.5,), (0.5,))]),
    }
    for name, c in refused.items():
        assert c.device_plan() is None, name
        assert re.match(r"step \d+: ", c.device_plan_refusal()), name
    assert 'Resize' in refused['order'].device_plan_refusal()
    assert 'CenterCrop' in refused['after ToTensor'].device_plan_refusal()


def _png_tree(tmp_path, P0=20):
    """One Cartesian array directory of 4 spot images (PNG: lossless)."""
    rng = np.random.default_rng(5)
    imdir = tmp_path / 'arr0'
    imdir.mkdir()
    imgs = {}
    for ax, ay in ((0, 0), (1, 0), (2, 1), (1, 2)):
        a = rng.integers(0, 256, (P0, P0, 3), dtype=np.uint8)
        Image.fromarray(a).save(str(imdir / ('spot_%d_%d.png' % (ax, ay))))
        imgs[(ax, ay)] = a
    return str(imdir), imgs


def test_datasets_decode_only_and_carry_the_transform(tmp_path):
    from gridnext_amd.image_datasets import PatchDataset, PatchGridDataset, to_tensor_u8
    imdir, imgs = _png_tree(tmp_path)
    mean, std = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)
    comp = T.Compose([T.Resize(16), T.CenterCrop(12), T.ToTensor(), T.Normalize(mean, std)])
    kw = dict(annot_files=None, Visium=False, img_ext='png')

    # raw_uint8 + a Compose with a device plan: the stored bytes, and the transform handed on
    ds = PatchDataset([imdir], img_transforms=comp, raw_uint8=True, **kw)
    assert ds.device_transform is comp and len(ds) == 4
    for i in range(4):
        patch, _ = ds[i]
        assert patch.dtype == torch.uint8 and patch.shape == (3, 20, 20)
        assert torch.equal(patch, to_tensor_u8(Image.open(ds.imgpath_mapping[i])))
    gd = PatchGridDataset([imdir], img_transforms=comp, raw_uint8=True, h_st=3, w_st=3, **kw)
    grid, labels = gd[0]
    assert gd.device_transform is comp and grid.dtype == torch.uint8 and grid.shape == (3, 3, 3, 20, 20)
    for (ax, ay), a in imgs.items():
        assert np.array_equal(grid[ay, ax].numpy(), a.transpose(2, 0, 1))
    assert not grid[0, 2].any()

    # ... without a device plan: refused, naming the step
    bad = T.Compose([T.ToTensor(), T.CenterCrop(12)])
    for cls in (PatchDataset, PatchGridDataset):
        with pytest.raises(ValueError, match=r"step 1: CenterCrop"):
            cls([imdir], img_transforms=bad, raw_uint8=True, **kw)

    # every other combination: as before
    host = PatchDataset([imdir], img_transforms=comp, **kw)          # the host path: the Compose runs per image
    assert host.device_transform is None
    patch, _ = host[0]
    assert patch.dtype == torch.float32 and patch.shape == (3, 12, 12)
    assert torch.equal(patch, comp(Image.open(host.imgpath_mapping[0])))
    plain = PatchDataset([imdir], **kw)
    assert plain.device_transform is None and plain[0][0].dtype == torch.float32 and plain[0][0].shape == (3, 20, 20)
    raw = PatchDataset([imdir], raw_uint8=True, **kw)
    assert raw.device_transform is None and raw.preprocess is to_tensor_u8 and raw[0][0].dtype == torch.uint8
    fn = PatchDataset([imdir], img_transforms=to_tensor_u8, raw_uint8=True, **kw)       # any other callable: taken as given
    assert fn.device_transform is None and fn.preprocess is to_tensor_u8
    hg = PatchGridDataset([imdir], img_transforms=comp, h_st=3, w_st=3, **kw)
    assert hg.device_transform is None and hg[0][0].shape == (3, 3, 3, 12, 12) and hg[0][0].dtype == torch.float32


def test_densenet_switches_and_cache_token():
    import gridnext_amd as ga
    from gridnext_amd import fcache
    assert ga.transforms is T
    f = ga.DenseNet(growth_rate=4, block_config=(1, 1), num_init_features=8, bn_size=2, num_classes=3, small_inputs=False)
    assert f.input_resize is None and f.input_crop is None
    assert 'input_resize' in fcache._DENSENET_SWITCHES and 'input_crop' in fcache._DENSENET_SWITCHES
    f.eval()
    t0 = fcache.state_token(f)
    f.set_input_transform(T.Compose([T.Resize(256), T.CenterCrop(224), T.ToTensor(), T.Normalize((.5, .5, .5), (.2, .2, .2))]))
    assert (f.input_resize, f.input_crop, f.input_norm) == (256, 224, ((.5, .5, .5), (.2, .2, .2)))
    t1 = fcache.state_token(f)
    f.input_crop = 200
    t2 = fcache.state_token(f)
    assert len({t0, t1, t2}) == 3                      # a frozen-f cache empties when either switch changes
    with pytest.raises(ValueError, match="step 1"):
        f.set_input_transform(T.Compose([T.CenterCrop(8)]))
    f.set_input_transform(None)
    assert f.input_resize is None and f.input_crop is None and f.input_norm is None and fcache.state_token(f) == t0
    assert f._input_geometry(260, 260) == (260, 260, 0, 0, 260, 260)


def test_header_ctypes_and_library_agree_on_the_resize_symbols():
    from gridnext_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = _lib.lib()
    for name, nargs in (('gnx_resize_crop_u8', 16), ('gnx_resize_crop_u8_f32', 17), ('gnx_resize_ksize', 2)):
        assert name in _lib.PARAMS, "%s is not declared in the header" % name
        assert len(_lib.PARAMS[name]) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(handle, name)
    assert 'image_datasets.py:102-105' in text and ':113-117' in text
    # the host query agrees with the Python formula (no device needed)
    for n_in, n_out in ((260, 256), (64, 128), (1000, 256), (1000, 125), (1001, 125), (50, 50), (127, 16)):
        assert _lib.query('gnx_resize_ksize', n_in, n_out) == T.axis_ksize(n_in, n_out)
