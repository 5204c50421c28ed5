"""From a whole-slide image (WSI) to a Visium array's patch grid, on the host and on the device.

The reference's image workflow starts here (gridnext/imgprocess.py): `grid_from_wsi_visium` cuts a window around every
in-tissue spot of the full-resolution image, resizes it with Pillow and places it in the (78, 64, 3, P, P) odd-right grid that
`GridNetHexOddr` reads; `save_visium_patches` writes that grid out as one JPEG per spot, the files `PatchGridDataset` reads.
The names and results below are the reference's:

    from gridnext_amd.imgprocess import grid_from_wsi_visium, save_visium_patches, save_visium_patches_all

  * `device=None` is the host path: the reference's arithmetic (window of the edge-padded slide, `Image.resize`, i.e. BICUBIC)
    without the padded copy of the slide;
  * with a HIP `device` the decoded slide is uploaded once as uint8 (Hs, Ws, 3) and ONE gather cuts, resizes and places every
    patch (gnx_wsi_patch_grid_u8 / gnx_wsi_patch_grid_u8_f32, csrc/wsi_patches.hip): Pillow's bytes, bit for bit.
    `raw_uint8=True` returns the uint8 grid on that device - what `GridNetHexOddr` over a `DenseNet` (and its
    `set_input_transform`) consumes as it is.  There is no CPU fallback on this path.

Stated differences from the reference, all raised on the host before anything is launched: a spot whose odd-right index is
outside the 78 x 64 grid is skipped with the reference's warning (the reference lets x_ind == 64 through to an IndexError); a
rounded spot centre outside the slide raises ValueError naming the barcode (the reference wraps or truncates its slice); two
spots that map to one cell raise; a slide that is not RGB raises.

Out of scope (not implemented here): `remove_color_cast` / `scale_rgb`, `distance_um_to_px`, `to_splotch_annots`,
`pseudo_visium_spots`, and a dataset class that serves arrays straight from slides.
"""
import glob
import os
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from . import _lib as L
from . import transforms as T
from .image_datasets import to_tensor

Image.MAX_IMAGE_PIXELS = None      # whole-slide images exceed Pillow's decompression-bomb guard (as in the reference)

VISIUM_H_ST = 78  # Visium arrays contain 78 rows (height)
VISIUM_W_ST = 64  # ...each row contains 64 spots (width)

_POSITION_COLUMNS = ["in_tissue", "array_row", "array_col", "pxl_row_in_fullres", "pxl_col_in_fullres"]


# ---------------------------------------------------------------------------------------------- coordinate helpers
def pseudo_hex_to_oddr(col, row):
    """Visium pseudo-hex (col doubles along a row) -> odd-right (x, y)."""
    if row % 2 == 0:
        x = col / 2
    else:
        x = (col - 1) / 2
    y = row
    return int(x), int(y)


def oddr_to_pseudo_hex(col, row):
    y_vis = row
    x_vis = col * 2
    if row % 2 == 1:
        x_vis += 1
    return int(x_vis), int(y_vis)


def pseudo_hex_to_cartesian(c):
    x, y = c
    return (x / 2, y * np.sqrt(3) / 2)


# ---------------------------------------------------------------------------------------------- position files
def visium_find_position_file(spaceranger_dir, hd_binning=None):
    """The file under `spaceranger_dir` that maps barcodes to array / pixel coordinates: the first *.csv (searched
    recursively) with "tissue_positions" in its path - tissue_positions.csv (Spaceranger >= 2) or tissue_positions_list.csv."""
    if hd_binning is not None:
        raise NotImplementedError("Visium HD binned outputs (tissue_positions.parquet) are not implemented")
    for pos_path in glob.glob(str(spaceranger_dir) + '/**/*.csv', recursive=True):
        if os.path.exists(pos_path) and "tissue_positions" in pos_path:
            return pos_path
    raise ValueError("Cannot locate position file for %s" % spaceranger_dir)


def visium_get_positions_fromfile(position_file):
    import pandas as pd
    position_file = str(position_file)
    if position_file.endswith('.parquet'):
        raise NotImplementedError("parquet position files (Visium HD) are not implemented")
    with open(position_file, 'r') as fh:          # a header line starting with "barcode": Spaceranger >= 2
        has_header = next(iter(fh)).startswith('barcode')
    if has_header:
        return pd.read_csv(position_file, index_col=0, header=0)
    return pd.read_csv(position_file, index_col=0, header=None, names=_POSITION_COLUMNS)


def visium_get_positions(spaceranger_dir, hd_binning=None):
    """DataFrame indexed by barcode with in_tissue, array_row, array_col, pxl_row_in_fullres, pxl_col_in_fullres."""
    return visium_get_positions_fromfile(visium_find_position_file(spaceranger_dir, hd_binning=hd_binning))


# ---------------------------------------------------------------------------------------------- slide, window, spots
def _decode_slide(fullres_imgfile):
    """uint8 (Hs, Ws, 3): a numpy array, or a torch tensor when one was passed (it stays on its device)."""
    if torch.is_tensor(fullres_imgfile):
        img = fullres_imgfile
        if img.dtype != torch.uint8:
            raise ValueError("a decoded slide must be uint8 (got %s)" % img.dtype)
    elif isinstance(fullres_imgfile, np.ndarray):
        img = fullres_imgfile
        if img.dtype != np.uint8:
            raise ValueError("a decoded slide must be uint8 (got %s)" % img.dtype)
    else:
        img = np.array(Image.open(fullres_imgfile))
        if img.dtype != np.uint8:
            raise ValueError("%s: not an 8-bit RGB image (decodes to %s)" % (fullres_imgfile, img.dtype))
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("the slide must be RGB, (Hs, Ws, 3); got shape %s" % (tuple(img.shape),))
    return img


def _window_size(window_size, patch_size, xdim):
    if window_size is None:
        return int(patch_size)
    if isinstance(window_size, float):
        return int(window_size * xdim)         # a fraction of the slide's WIDTH (imgprocess.py:190-191)
    if isinstance(window_size, (int, np.integer)) and not isinstance(window_size, bool):
        return int(window_size)
    raise ValueError("Window size must be a float or int")


def _spot_table(spaceranger_dir, ydim, xdim):
    """int32 [n][4] = {x_px, y_px, grid_row, grid_col} of the in-tissue spots that fall into the grid, in file order."""
    df = visium_get_positions(spaceranger_dir)
    df = df[df['in_tissue'] == 1]
    spots, taken = [], {}
    for i in range(len(df)):
        row = df.iloc[i]
        x_ind, y_ind = pseudo_hex_to_oddr(row['array_col'], row['array_row'])
        x_px = int(np.rint(row['pxl_col_in_fullres']))      # fractional pixel coordinates (rare): half to even
        y_px = int(np.rint(row['pxl_row_in_fullres']))
        if y_ind >= VISIUM_H_ST or x_ind >= VISIUM_W_ST:
            print("Warning: column %d row %d outside bounds of Visium array" % (x_ind, y_ind))
            continue
        barcode = df.index[i]
        if y_ind < 0 or x_ind < 0:
            raise ValueError("spot %s: negative array position (col %r, row %r)" % (barcode, row['array_col'], row['array_row']))
        if not (0 <= x_px < xdim and 0 <= y_px < ydim):
            raise ValueError("spot %s: centre (x %d, y %d) lies outside the %d x %d slide" % (barcode, x_px, y_px, xdim, ydim))
        if (y_ind, x_ind) in taken:
            raise ValueError("spots %s and %s both map to cell (row %d, col %d)" % (taken[(y_ind, x_ind)], barcode, y_ind, x_ind))
        taken[(y_ind, x_ind)] = barcode
        spots.append((x_px, y_px, y_ind, x_ind))
    return np.asarray(spots, dtype=np.int32).reshape(-1, 4)


def _window(img, x_px, y_px, half):
    """Rows and columns [c - half, c + half) of the edge-padded slide = every coordinate clamped to the slide."""
    y0, x0 = y_px - half, x_px - half
    if y0 >= 0 and x0 >= 0 and y0 + 2 * half <= img.shape[0] and x0 + 2 * half <= img.shape[1]:
        return np.ascontiguousarray(img[y0:y0 + 2 * half, x0:x0 + 2 * half])
    rows = np.clip(np.arange(y0, y0 + 2 * half), 0, img.shape[0] - 1)
    cols = np.clip(np.arange(x0, x0 + 2 * half), 0, img.shape[1] - 1)
    return np.ascontiguousarray(img[np.ix_(rows, cols)])


def _device_norm(preprocess_xform):
    """(mean, std) of a transform the kernel's float form computes: `transforms.Normalize` or a Compose of [ToTensor] Normalize."""
    steps = preprocess_xform.transforms if isinstance(preprocess_xform, T.Compose) else [preprocess_xform]
    steps = list(steps)
    if len(steps) == 2 and isinstance(steps[0], T.ToTensor):
        steps = steps[1:]
    if len(steps) == 1 and isinstance(steps[0], T.Normalize) and len(steps[0].mean) == 3 and len(steps[0].std) == 3:
        return steps[0].mean, steps[0].std
    raise ValueError("preprocess_xform %r cannot run on the device: only transforms.Normalize (three channels), or a Compose of "
                     "[ToTensor] Normalize, is computed there; take device=None for any other callable" % (preprocess_xform,))


_TABLES = {}         # (window, P, device) -> (coef, bnd) device int32


def _device_tables(win, P, dev):
    key = (win, P, str(dev))
    hit = _TABLES.get(key)
    if hit is None:
        if len(_TABLES) >= 64:
            _TABLES.clear()
        hit = _TABLES[key] = tuple(torch.from_numpy(a).to(dev) for a in T.axis_tables(win, P, filter='bicubic'))
    return hit


def _grid_on_device(img, spots, half, P, dev, norm, out_float):
    """The kernel call: slide -> (78, 64, 3, P, P) uint8 (or ToTensor / Normalize of those bytes as float32) on `dev`."""
    dev = torch.device(dev)
    if dev.type != 'cuda':
        raise RuntimeError("grid_from_wsi_visium(device=%s): the device path runs on a HIP device only; device=None is the host "
                           "path" % dev)
    ks = T.axis_ksize(2 * half, P, 'bicubic')
    if ks > T.MAX_KSIZE:
        raise ValueError("a %d-pixel window is more than 4x the %d-pixel patch, which the device path does not resample "
                         "(ksize %d > %d): take device=None" % (2 * half, P, ks, T.MAX_KSIZE))
    slide = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
    slide = slide.to(dev).contiguous()                       # the one upload (none for a slide that is already resident)
    Hs, Ws = int(slide.shape[0]), int(slide.shape[1])
    out = torch.zeros((VISIUM_H_ST, VISIUM_W_ST, 3, P, P), device=dev, dtype=torch.float32 if out_float else torch.uint8)
    coef, bnd = _device_tables(2 * half, P, dev)
    spots = np.ascontiguousarray(spots, dtype=np.int32)
    with torch.cuda.device(dev):
        args = (slide.data_ptr(), Hs, Ws, spots.ctypes.data, len(spots), half, P, VISIUM_H_ST, VISIUM_W_ST,
                L.ptr(coef, torch.int32), L.ptr(bnd, torch.int32), ks, out.data_ptr())
        if out_float:
            L.call('gnx_wsi_patch_grid_u8_f32', *args, L.ptr(norm), L.stream())
        else:
            L.call('gnx_wsi_patch_grid_u8', *args, L.stream())
    return out


# ---------------------------------------------------------------------------------------------- the public functions
def grid_from_wsi_visium(fullres_imgfile, spaceranger_dir, patch_size=256, window_size=256, preprocess_xform=None,
                         device=None, raw_uint8=False):
    """Patches centred at each in-tissue Visium spot, as the odd-right grid (78, 64, 3, patch_size, patch_size).

    fullres_imgfile: path of the full-resolution image, or the decoded slide itself (numpy / torch uint8 (Hs, Ws, 3); repeated
        calls then do not decode - or upload - again).
    spaceranger_dir: directory holding Spaceranger's output (its tissue_positions*.csv is searched recursively).
    window_size: the region cut around a spot before it is resized to patch_size - None: patch_size; int: pixels; float: that
        fraction of the slide's width.  The window is rows and columns [c - w//2, c - w//2 + 2 (w//2)) of the edge-padded
        slide (an odd w gives w - 1), c the spot's pixel coordinate rounded half to even.
    preprocess_xform: applied to ToTensor of each patch.
    device: None - the host path, the reference's result: float32 holding the patch bytes as 0..255 (the reference never
        divides by 255 here), or xform(to_tensor(patch)) per patch.  A HIP device - the kernel path: the same floats on that
        device (preprocess_xform: `transforms.Normalize`, or a Compose of [ToTensor] Normalize; any other callable is
        refused), or with raw_uint8=True the uint8 grid.
    Cells without a spot are zero."""
    img = _decode_slide(fullres_imgfile)
    ydim, xdim = int(img.shape[0]), int(img.shape[1])
    P = int(patch_size)
    if P <= 0:
        raise ValueError("patch_size must be positive, got %r" % (patch_size,))
    w = _window_size(window_size, P, xdim)
    half = w // 2
    if half < 1:
        raise ValueError("window_size %r gives an empty window (%d pixels)" % (window_size, 2 * half))
    if device is None and raw_uint8:
        raise ValueError("raw_uint8=True returns the grid on a HIP device: pass device=")
    norm = None
    if device is not None and preprocess_xform is not None and not raw_uint8:
        norm = _device_norm(preprocess_xform)
    spots = _spot_table(spaceranger_dir, ydim, xdim)

    if device is not None:
        dev = torch.device(device)
        if raw_uint8:
            return _grid_on_device(img, spots, half, P, dev, None, False)
        if norm is None:            # the patch bytes as float32 0..255: the uint8 grid, converted (exact) where it lies
            return _grid_on_device(img, spots, half, P, dev, None, False).float()
        sd = torch.tensor(norm[1], dtype=torch.float32)
        nrm = torch.cat([torch.tensor(norm[0], dtype=torch.float32), sd, 1.0 / sd]).to(dev)
        return _grid_on_device(img, spots, half, P, dev, nrm, True)

    if torch.is_tensor(img):
        img = img.cpu().numpy()
    img_tensor = torch.zeros((VISIUM_H_ST, VISIUM_W_ST, 3, P, P))
    for x_px, y_px, y_ind, x_ind in spots.tolist():
        patch = np.array(Image.fromarray(_window(img, x_px, y_px, half)).resize((P, P)))
        if preprocess_xform is not None:
            patch = preprocess_xform(to_tensor(Image.fromarray(patch)))
        else:
            patch = torch.from_numpy(patch).permute(2, 0, 1)
        img_tensor[y_ind, x_ind] = patch
    return img_tensor.float()


def save_visium_patches(img_file, spaceranger_dir, dest_dir, patch_size=256, window_size=None, device=None):
    """Write the patch of every spot of one array as "<slide>_<x_vis>_<y_vis>.jpg" under `dest_dir` (Visium indexing, the
    directory layout the patch datasets read); <slide> is the stem of `spaceranger_dir`.  As in the reference a cell is written
    when its patch has a non-zero byte.  With a HIP `device` the patches are cut there and the uint8 grid comes back in one
    copy; the JPEG encoding is the host's either way."""
    if device is None:
        patch_grid = grid_from_wsi_visium(img_file, spaceranger_dir, patch_size=patch_size, window_size=window_size)
        patch_grid = patch_grid.numpy().astype(np.uint8)
    else:
        patch_grid = grid_from_wsi_visium(img_file, spaceranger_dir, patch_size=patch_size, window_size=window_size,
                                          device=device, raw_uint8=True).cpu().numpy()
    if not os.path.exists(dest_dir):
        os.mkdir(dest_dir)
    slide = str(Path(spaceranger_dir).stem)
    filled = patch_grid.reshape(VISIUM_H_ST, VISIUM_W_ST, -1).any(-1)
    for oddr_x in range(VISIUM_W_ST):
        for oddr_y in range(VISIUM_H_ST):
            if filled[oddr_y, oddr_x]:
                patch = np.moveaxis(patch_grid[oddr_y, oddr_x], 0, 2)      # channels last
                x_vis, y_vis = oddr_to_pseudo_hex(oddr_x, oddr_y)
                Image.fromarray(patch).save(os.path.join(dest_dir, "%s_%d_%d.jpg" % (slide, x_vis, y_vis)), "JPEG")


def save_visium_patches_all(wsi_files, spaceranger_dirs, dest_dir, patch_size=256, window_size=None, device=None):
    """`save_visium_patches` for several arrays: one sub-directory of `dest_dir` per slide, named by the image file's stem."""
    if not os.path.isdir(dest_dir):
        os.mkdir(dest_dir)
    for img_file, srd in zip(wsi_files, spaceranger_dirs):
        print("%s : %s ..." % (img_file, srd))
        slide = str(Path(img_file).stem)
        save_visium_patches(img_file, srd, os.path.join(dest_dir, slide), patch_size, window_size, device=device)
