"""gridnext_amd.imgprocess on the host (no GPU): `grid_from_wsi_visium(device=None)` against the reference's recorded output
(tests/golden/wsi_grid.npz, written by tools/gen_golden_wsi.py from the fixture slide and position trees under
tests/golden/files/), its window / rounding / filter rules one by one, the stated refusals, and `save_visium_patches`."""
import io
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import wsi_ref as W
from gridnext_amd import imgprocess as IP
from gridnext_amd import transforms as T

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, 'golden', 'files')
SLIDE = os.path.join(FILES, 'wsi_slide.png')
SR2 = os.path.join(FILES, 'wsi_sr2')          # spaceranger/outs/spatial/tissue_positions.csv (Spaceranger >= 2)
SR1 = os.path.join(FILES, 'wsi_sr1')          # outs/spatial/tissue_positions_list.csv (no header)
HS, WS = 47, 61


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'wsi_grid.npz')))


@pytest.fixture(scope='module')
def slide():
    return np.array(Image.open(SLIDE))


def _pairs(golden):
    return [(int(p), None if w < 0 else (int(w) if float(w).is_integer() else float(w))) for p, w in golden['pairs']]


def test_host_grid_equals_the_reference(golden, slide):
    pairs = _pairs(golden)
    assert pairs == [(8, 8), (8, None), (8, 12), (12, 8), (8, 5), (8, 30), (7, 9), (8, 0.2)]
    for i, (P, w) in enumerate(pairs):
        want = torch.from_numpy(golden['grid_%d' % i]).float()
        got = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w)
        assert got.dtype == torch.float32 and tuple(got.shape) == (78, 64, 3, P, P)
        assert torch.equal(got, want), (P, w)
        assert float(got.max()) > 1.0 and float(got.max()) <= 255.0            # the bytes as 0..255: never divided
        assert torch.equal(IP.grid_from_wsi_visium(slide, SR2, patch_size=P, window_size=w), want)     # a decoded slide
    assert torch.equal(IP.grid_from_wsi_visium(torch.from_numpy(slide), SR2, patch_size=8, window_size=12),
                       torch.from_numpy(golden['grid_2']).float())
    # the headerless layout
    got = IP.grid_from_wsi_visium(SLIDE, SR1, patch_size=8, window_size=12)
    assert torch.equal(got, torch.from_numpy(golden['grid_sr1_8_12']).float())
    # preprocess_xform: xform(to_tensor(patch))
    norm = T.Normalize(tuple(golden['norm_mean']), tuple(golden['norm_std']))
    got = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=4, window_size=6, preprocess_xform=norm)
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(golden['grid_norm_4_6']))


def test_position_files_both_layouts():
    p2, p1 = IP.visium_find_position_file(SR2), IP.visium_find_position_file(SR1)
    assert p2.endswith(os.path.join('spaceranger', 'outs', 'spatial', 'tissue_positions.csv'))
    assert p1.endswith(os.path.join('outs', 'spatial', 'tissue_positions_list.csv'))
    d2, d1 = IP.visium_get_positions(SR2), IP.visium_get_positions(SR1)
    cols = ['in_tissue', 'array_row', 'array_col', 'pxl_row_in_fullres', 'pxl_col_in_fullres']
    assert list(d2.columns) == cols and list(d1.columns) == cols
    assert len(d2) == 16 and len(d1) == 14 and d2.index[0] == d1.index[0] == 'CORNER_TL-1'
    assert list(d1.index) == list(d2.index[:14])
    assert np.array_equal(d1.values.astype(np.float64), d2.values[:14].astype(np.float64))
    assert d2.loc['HALF_EVEN-1', 'pxl_row_in_fullres'] == 20.5
    with pytest.raises(ValueError, match="position file"):
        IP.visium_find_position_file(os.path.join(FILES, 'wsi_sr2', 'spaceranger', 'outs', 'spatial', 'nothing_here'))
    with pytest.raises(NotImplementedError):
        IP.visium_find_position_file(SR2, hd_binning='square_008um')
    with pytest.raises(NotImplementedError):
        IP.visium_get_positions_fromfile('tissue_positions.parquet')


def test_coordinate_helpers():
    assert (IP.VISIUM_H_ST, IP.VISIUM_W_ST) == (78, 64)
    assert IP.pseudo_hex_to_oddr(126, 0) == (63, 0) and IP.pseudo_hex_to_oddr(127, 77) == (63, 77)
    assert IP.pseudo_hex_to_oddr(41.0, 21.0) == (20, 21)                 # floats, as a DataFrame row hands them over
    for col in range(5):
        for row in range(5):
            assert IP.pseudo_hex_to_oddr(*IP.oddr_to_pseudo_hex(col, row)) == (col, row)
    assert IP.oddr_to_pseudo_hex(3, 1) == (7, 1) and IP.oddr_to_pseudo_hex(3, 2) == (6, 2)
    x, y = IP.pseudo_hex_to_cartesian((4, 2))
    assert x == 2.0 and y == 2 * np.sqrt(3) / 2


def _cell(grid, col, row):
    x, y = IP.pseudo_hex_to_oddr(col, row)
    return grid[y, x].numpy().astype(np.uint8)


def test_window_rules_one_by_one(slide):
    g8 = IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=8)
    # identity size: the bytes of the slide, planar (INNER_A: array_row 20, array_col 40, centre x 20, y 15)
    assert np.array_equal(_cell(g8, 40, 20), slide[11:19, 16:24].transpose(2, 0, 1))
    # window_size=None is patch_size
    assert torch.equal(IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=None), g8)
    # an odd window: 2 * (5 // 2) = 4 pixels, resized to 8
    g5 = IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=5)
    assert torch.equal(g5, IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=4))
    assert np.array_equal(_cell(g5, 40, 20), W.pillow_patch(slide, 20, 15, 4, 8))
    assert not torch.equal(g5, IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=6))
    # half to even: (24.5, 20.5) -> (24, 20); (25.5, 21.5) -> (26, 22)
    assert np.array_equal(_cell(g8, 20, 60), W.pillow_patch(slide, 24, 20, 8, 8))
    assert np.array_equal(_cell(g8, 21, 61), W.pillow_patch(slide, 26, 22, 8, 8))
    assert not np.array_equal(_cell(g8, 20, 60), W.pillow_patch(slide, 25, 21, 8, 8))
    # in_tissue == 0: its cell (row 30, col 30 -> x 15) stays zero; 15 of the 16 rows fill a cell
    assert not g8[30, 15].any()
    assert int(g8.reshape(78, 64, -1).amax(-1).gt(0).sum()) == 15
    # a float window: that fraction of the slide's WIDTH (0.2 * 61 -> 12), not of the patch size
    gf = IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=0.2)
    assert torch.equal(gf, IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=12))
    # corners: the edge is replicated (CORNER_BR: array_row 77, array_col 127, centre (60, 46))
    g12 = IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=12)
    assert np.array_equal(_cell(g12, 127, 77), W.pillow_patch(slide, WS - 1, HS - 1, 12, 8))
    assert np.array_equal(_cell(g12, 127, 77), W.patch(slide, WS - 1, HS - 1, 12, 8))
    with pytest.raises(ValueError, match="float or int"):
        IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size='8')
    with pytest.raises(ValueError, match="empty window"):
        IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=1)
    with pytest.raises(ValueError, match="HIP device"):
        IP.grid_from_wsi_visium(slide, SR2, patch_size=8, raw_uint8=True)


def _tree(tmp_path, name, rows):
    d = tmp_path / name / 'outs' / 'spatial'
    d.mkdir(parents=True)
    with open(str(d / 'tissue_positions.csv'), 'w') as fh:
        fh.write('barcode,in_tissue,array_row,array_col,pxl_row_in_fullres,pxl_col_in_fullres\n')
        for r in rows:
            fh.write('%s,%d,%d,%d,%s,%s\n' % r)
    return str(tmp_path / name)


def test_stated_refusals(tmp_path, slide, capsys):
    ok = ('A-1', 1, 2, 2, 10, 10)
    # a rounded centre outside the slide: names the barcode
    for bad in (('OUT_X-1', 1, 4, 4, 10, WS), ('OUT_Y-1', 1, 4, 4, HS, 10), ('NEG-1', 1, 4, 4, -1, 10),
                ('ROUNDS_OUT-1', 1, 4, 4, 10, WS - 0.4)):
        with pytest.raises(ValueError, match=bad[0]):
            IP.grid_from_wsi_visium(slide, _tree(tmp_path, 'c_' + bad[0], [ok, bad]), patch_size=8, window_size=8)
    IP.grid_from_wsi_visium(slide, _tree(tmp_path, 'c_in', [ok, ('IN-1', 1, 4, 4, 10, WS - 0.6)]), patch_size=8, window_size=8)
    # ... but not for a spot outside the tissue
    IP.grid_from_wsi_visium(slide, _tree(tmp_path, 'c_off', [ok, ('OFF-1', 0, 4, 4, 10, WS + 5)]), patch_size=8, window_size=8)
    # two spots on one cell
    with pytest.raises(ValueError, match="A-1 and B-1 both map to cell"):
        IP.grid_from_wsi_visium(slide, _tree(tmp_path, 'dup', [ok, ('B-1', 1, 2, 2, 20, 20)]), patch_size=8, window_size=8)
    # a slide that is not RGB
    for bad_slide in (slide[:, :, 0], np.concatenate([slide, slide[:, :, :1]], 2)):
        with pytest.raises(ValueError, match="RGB"):
            IP.grid_from_wsi_visium(bad_slide, SR2, patch_size=8, window_size=8)
    grey = tmp_path / 'grey.png'
    Image.fromarray(slide[:, :, 0]).save(str(grey))
    with pytest.raises(ValueError, match="RGB"):
        IP.grid_from_wsi_visium(str(grey), SR2, patch_size=8, window_size=8)
    with pytest.raises(ValueError, match="uint8"):
        IP.grid_from_wsi_visium(slide.astype(np.float32), SR2, patch_size=8, window_size=8)
    # outside the 78 x 64 grid: skipped with the reference's warning - x_ind == 64 too
    capsys.readouterr()
    g = IP.grid_from_wsi_visium(slide, _tree(tmp_path, 'far', [ok, ('COL64-1', 1, 2, 128, 20, 20), ('ROW78-1', 1, 78, 2, 20, 20)]),
                                patch_size=8, window_size=8)
    out = capsys.readouterr().out
    assert "Warning: column 64 row 2 outside bounds of Visium array" in out
    assert "Warning: column 1 row 78 outside bounds of Visium array" in out
    assert int(g.reshape(78, 64, -1).amax(-1).gt(0).sum()) == 1
    # the device path's own refusals are raised before a device is touched
    with pytest.raises(ValueError, match="cannot run on the device"):
        IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=8, preprocess_xform=(lambda t: t), device='cuda:0')
    with pytest.raises(ValueError, match="cannot run on the device"):
        IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=8, device='cuda:0',
                                preprocess_xform=T.Compose([T.ToTensor(), T.Normalize((.5,) * 3, (.2,) * 3), T.ToTensor()]))
    with pytest.raises(ValueError, match="device=None"):
        IP.grid_from_wsi_visium(slide, SR2, patch_size=8, window_size=34, device='cuda:0', raw_uint8=True)


def _expected_files(grid_u8, slide_name):
    files = {}
    for oddr_x in range(64):
        for oddr_y in range(78):
            if grid_u8[oddr_y, oddr_x].max() > 0:
                x_vis, y_vis = IP.oddr_to_pseudo_hex(oddr_x, oddr_y)
                buf = io.BytesIO()
                Image.fromarray(np.moveaxis(grid_u8[oddr_y, oddr_x], 0, 2)).save(buf, "JPEG")
                files["%s_%d_%d.jpg" % (slide_name, x_vis, y_vis)] = buf.getvalue()
    return files


def test_save_visium_patches_writes_the_reference_files(tmp_path, golden):
    dest = tmp_path / 'patches'
    IP.save_visium_patches(SLIDE, SR2, str(dest), patch_size=8, window_size=12)
    want = _expected_files(golden['grid_2'], 'wsi_sr2')            # the slide name: the stem of the spaceranger directory
    assert len(want) == 15 and 'wsi_sr2_127_77.jpg' in want and 'wsi_sr2_0_0.jpg' in want and 'wsi_sr2_41_21.jpg' in want
    assert sorted(os.listdir(str(dest))) == sorted(want)
    for name, data in want.items():
        assert open(str(dest / name), 'rb').read() == data, name
    # window_size=None (the default here): patch_size
    dest2 = tmp_path / 'patches2'
    IP.save_visium_patches(SLIDE, SR1, str(dest2), patch_size=8)
    assert len(os.listdir(str(dest2))) == 13 and 'wsi_sr1_0_0.jpg' in os.listdir(str(dest2))
    # the multi-array form: one sub-directory per slide, named by the image's stem
    img2 = tmp_path / 'second.png'
    shutil.copy(SLIDE, str(img2))
    top = tmp_path / 'all'
    IP.save_visium_patches_all([SLIDE, str(img2)], [SR2, SR1], str(top), patch_size=8, window_size=12)
    assert sorted(os.listdir(str(top))) == ['second', 'wsi_slide']
    assert sorted(os.listdir(str(top / 'wsi_slide'))) == sorted(want)
    assert len(os.listdir(str(top / 'second'))) == 13
    for name, data in want.items():
        assert open(str(top / 'wsi_slide' / name), 'rb').read() == data


def test_new_symbols_are_declared_bound_and_exported():
    from gridnext_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = _lib.lib()
    for name, nargs in (('gnx_wsi_patch_grid_u8', 14), ('gnx_wsi_patch_grid_u8_f32', 15)):
        assert name in _lib.PARAMS, "%s is not declared in the header" % name
        assert len(_lib.PARAMS[name]) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(handle, name)
    assert 'imgprocess.py:198-236' in text
    import gridnext_amd as ga
    assert ga.imgprocess is IP
