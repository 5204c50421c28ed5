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

`remove_color_cast` / `scale_rgb` are SpaCell's white balance (imgprocess.py:49-67): the 99th percentile of the whole slide per
channel, then `Image.point(i -> i * 255 / p)` on every byte.  A PIL image goes through Pillow as in the reference; a numpy
array or CPU tensor through the same arithmetic restated on a 3 x 256 histogram and a 3 x 256 table; a HIP tensor through
gnx_rgb_hist_u8 / gnx_rgb_lut_u8 (csrc/colorcast.hip), the percentile and the table computed on the host in between - the
same bytes on all three.  `grid_from_wsi_visium(..., remove_cast=True)` applies it to the decoded slide before the windows
are cut.  `cast_tables(img)` returns the 3 x 256 tables alone, and `cast_lut=` hands such tables to the cut: on the device the
table is folded into the gather (gnx_wsi_patch_grid_u8_lut / _u8_f32_lut), so a resident slide is never written and never
copied - what `SlideGridDataset` / `SlidePatchDataset` (image_datasets.py) rely on to serve any patch and window size from
one resident slide.  `patches_from_wsi` is the same gather for an explicit list of centres.  `distance_um_to_px` is the
reference's estimate of a physical distance in pixels (host only).

Out of scope (not implemented here): `to_splotch_annots`, `pseudo_visium_spots`, Visium HD.
"""
import glob
import math
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


def _check_cast_lut(cast_lut, remove_cast):
    """`cast_lut` as it was given, checked: a (3, 256) uint8 numpy array or tensor, and not together with remove_cast."""
    if cast_lut is None:
        return None
    if remove_cast:
        raise ValueError("cast_lut= and remove_cast=True both replace the slide's bytes: pass one of them")
    if torch.is_tensor(cast_lut):
        ok = cast_lut.dtype == torch.uint8
    elif isinstance(cast_lut, np.ndarray):
        ok = cast_lut.dtype == np.uint8
    else:
        raise ValueError("cast_lut must be a (3, 256) uint8 numpy array or tensor, got %s" % type(cast_lut).__name__)
    if not ok or tuple(cast_lut.shape) != (3, 256):
        raise ValueError("cast_lut must be uint8 of shape (3, 256), got %s of shape %s" % (cast_lut.dtype, tuple(cast_lut.shape)))
    return cast_lut


def _lut_host(cast_lut):
    return cast_lut.cpu().numpy() if torch.is_tensor(cast_lut) else cast_lut


def _grid_on_device(img, spots, half, P, dev, norm, out_float, remove_cast=False, cast_lut=None,
                    grid=(VISIUM_H_ST, VISIUM_W_ST), out=None):
    """The kernel call: slide -> `grid` + (3, P, P) uint8 (or ToTensor / Normalize of those bytes as float32) on `dev`.  With
    cast_lut (checked; (3, 256) uint8) the table is folded into the gather (the _lut entry points): the slide is only read.
    out: the tensor to fill (every listed cell is written, no other); None: a zero-filled one."""
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
    if remove_cast:
        if torch.is_tensor(img) and slide.data_ptr() == img.data_ptr():
            cast_lut = cast_tables(slide)                    # the caller's resident tensor: folded into the gather, no copy
        else:
            slide = remove_color_cast(slide, inplace=True)   # this call's own upload: in place
    Hs, Ws = int(slide.shape[0]), int(slide.shape[1])
    dtype = torch.float32 if out_float else torch.uint8
    if out is None:
        out = torch.zeros(tuple(grid) + (3, P, P), device=dev, dtype=dtype)
    coef, bnd = T.device_axis_tables(2 * half, P, 0, P, 'bicubic', dev)
    spots = np.ascontiguousarray(spots, dtype=np.int32)
    table = None
    if cast_lut is not None:
        if torch.is_tensor(cast_lut):
            table = cast_lut.to(dev).contiguous()
        else:
            table = torch.from_numpy(np.ascontiguousarray(cast_lut)).to(dev)
    with torch.cuda.device(dev):
        args = (slide.data_ptr(), Hs, Ws, spots.ctypes.data, len(spots), half, P, int(grid[0]), int(grid[1]),
                L.ptr(coef, torch.int32), L.ptr(bnd, torch.int32), ks, out.data_ptr())
        if out_float:
            args += (L.ptr(norm),)
        name = 'gnx_wsi_patch_grid_u8_f32' if out_float else 'gnx_wsi_patch_grid_u8'
        if table is None:
            L.call(name, *args, L.stream())
        else:
            L.call(name + '_lut', *args, table.data_ptr(), L.stream())
    return out


# ---------------------------------------------------------------------------------------------- colour cast
_CHANNELS = ('red', 'green', 'blue')


def _percentile99_from_hist(h):
    """np.percentile(values, q=99) (method 'linear', numpy's two-sided lerp) of the values counted in the 256-bin histogram h."""
    h = np.asarray(h).astype(np.int64)
    n = int(h.sum())
    if n == 0:
        raise ValueError("the 99th percentile of an empty slide is undefined")
    cum = np.cumsum(h)
    vi = (n - 1) * 0.99                        # the virtual index into the sorted values
    if vi >= n - 1:                            # (n == 1)
        lo = hi = n - 1
    else:
        lo = int(math.floor(vi))
        hi = lo + 1
    g = vi - lo
    a = int(np.searchsorted(cum, lo, side='right'))        # the sorted values at lo and hi
    b = int(np.searchsorted(cum, hi, side='right'))
    d = float(b - a)
    return b - d * (1 - g) if g >= 0.5 else a + d * g


def _lut_from_scale(scale):
    """Pillow's table for `point(lambda i: i * scale)` on an 8-bit band: clip(round(i * scale), 0, 255), Python's round."""
    if not math.isfinite(scale):
        raise ValueError("a channel scale must be finite, got %r" % (scale,))
    return np.array([min(max(round(i * scale), 0), 255) for i in range(256)], dtype=np.uint8)


def _cast_scales(hist):
    """255 / p99 per channel from the (3, 256) histogram; a channel whose percentile is 0 cannot be scaled."""
    scales = []
    for c in range(3):
        p = _percentile99_from_hist(hist[c])
        if p == 0:
            raise ValueError("the 99th percentile of the %s channel is 0: the colour cast cannot be removed" % _CHANNELS[c])
        scales.append(255 / p)
    return scales


def _hist_host(a):
    return np.stack([np.bincount(a[:, :, c].ravel(), minlength=256) for c in range(3)])


def _hist_device(slide):
    """(3, 256) int64 on the host: gnx_rgb_hist_u8 on the contiguous resident slide, one 6 KB copy back."""
    n = int(slide.shape[0]) * int(slide.shape[1])
    hist = torch.empty(3 * 256, device=slide.device, dtype=torch.int64)
    nws = L.query('gnx_rgb_hist_u8_workspace', n)
    ws = torch.empty(nws // 8, device=slide.device, dtype=torch.int64) if nws else None
    with torch.cuda.device(slide.device):
        L.call('gnx_rgb_hist_u8', slide.data_ptr(), n, hist.data_ptr(), None if ws is None else ws.data_ptr(), L.stream())
    return hist.cpu().numpy().reshape(3, 256)


def cast_tables(img):
    """The (3, 256) uint8 numpy tables `remove_color_cast(img)` applies: table[c][i] = clip(round(i * 255 / p99 of channel c)).
    img: a PIL image, or a decoded slide, numpy or torch uint8 (H, W, 3); a HIP tensor is counted where it lies
    (gnx_rgb_hist_u8) and 6 KB come back.  Raises what `remove_color_cast` raises (a channel whose percentile is 0).
    `grid_from_wsi_visium(..., cast_lut=)` cuts the corrected patches with them, the slide left as it is."""
    if isinstance(img, Image.Image):
        hist = _hist_host(np.array(img.convert('RGB')))
    else:
        img = _decode_slide(img)
        if torch.is_tensor(img) and img.is_cuda:
            hist = _hist_device(img.contiguous())
        else:
            hist = _hist_host(img.numpy() if torch.is_tensor(img) else img)
    return np.stack([_lut_from_scale(s) for s in _cast_scales(hist)])


def _apply_luts(img, luts, inplace):
    """img: numpy / torch uint8 (H, W, 3) (checked); luts: uint8 (3, 256), or None: the colour-cast tables of img itself."""
    if torch.is_tensor(img):
        if not img.is_contiguous():
            if inplace:
                raise ValueError("inplace=True needs a contiguous tensor (a non-contiguous one is copied first)")
            img = img.contiguous()
            inplace = True                      # the copy is ours
        if luts is None:
            luts = cast_tables(img)
        if img.is_cuda:
            out = img if inplace else torch.empty_like(img)
            table = torch.from_numpy(np.ascontiguousarray(luts)).to(img.device)
            with torch.cuda.device(img.device):
                L.call('gnx_rgb_lut_u8', img.data_ptr(), out.data_ptr(), int(img.shape[0]) * int(img.shape[1]),
                       table.data_ptr(), L.stream())
            return out
        a = img.numpy()
        out = img if inplace else torch.empty_like(img)
        _apply_luts_host(a, luts, out.numpy())
        return out
    if inplace:
        raise ValueError("inplace=True is for torch tensors")
    return _apply_luts_host(img, cast_tables(img) if luts is None else luts, np.empty_like(img))


def _apply_luts_host(a, luts, out):
    for c in range(3):
        out[:, :, c] = luts[c][a[:, :, c]]
    return out


def scale_rgb(img, r_scale, g_scale, b_scale, inplace=False):
    """Every channel multiplied by its scale as Pillow's `point` does it: byte i -> clip(round(i * scale), 0, 255), so a
    negative scale gives 0.  img: a PIL image (returns a PIL image: the reference's split / point / merge), or a decoded slide,
    numpy or torch uint8 (H, W, 3) (returns the same kind, a tensor on its device; a HIP tensor runs gnx_rgb_lut_u8).
    inplace=True (tensors only) overwrites img and returns it."""
    scales = (r_scale, g_scale, b_scale)
    for s in scales:
        if not math.isfinite(s):
            raise ValueError("a channel scale must be finite, got %r" % (s,))
    if isinstance(img, Image.Image):
        if inplace:
            raise ValueError("inplace=True is for torch tensors")
        source = img.split()
        return Image.merge('RGB', [source[c].point(lambda i, s=scales[c]: i * s) for c in range(3)])
    img = _decode_slide(img)
    return _apply_luts(img, np.stack([_lut_from_scale(s) for s in scales]), inplace)


def remove_color_cast(img, inplace=False):
    """SpaCell's white balance: every channel scaled by 255 / (its 99th percentile over the whole slide), so that the background
    turns white.  img and the result as in `scale_rgb`; all three kinds give the same bytes.  A HIP tensor is counted and
    scaled where it lies (gnx_rgb_hist_u8, one 6 KB copy to the host for the percentiles and the tables, gnx_rgb_lut_u8);
    inplace=True (tensors only) overwrites it, so a slide needs no second copy.  A channel whose percentile is 0 raises
    ValueError before anything is written."""
    if isinstance(img, Image.Image):
        if inplace:
            raise ValueError("inplace=True is for torch tensors")
        img = img.convert('RGB')
        img_array = np.array(img)
        scales = []
        for c in range(3):
            p = np.percentile(img_array[:, :, c].ravel(), q=99)
            if p == 0:
                raise ValueError("the 99th percentile of the %s channel is 0: the colour cast cannot be removed" % _CHANNELS[c])
            scales.append(255 / p)
        return scale_rgb(img, *scales)
    return _apply_luts(_decode_slide(img), None, inplace)


# ---------------------------------------------------------------------------------------------- image resolution
def distance_um_to_px(spaceranger_dir, distance_um, random_state=None):
    """Number of full-resolution pixels that span `distance_um` (the reference's estimate, imgprocess.py:89-109): over up to 10
    positions of the array (`DataFrame.sample(n=10, random_state=random_state)` when there are more), the mean ratio of pairwise
    pixel distance to pairwise Cartesian array distance is the length of one centre-to-centre step, 100 um."""
    positions = visium_get_positions(spaceranger_dir)
    if len(positions) > 10:
        positions = positions.sample(n=10, random_state=random_state)
    px = np.array(list(zip(positions['pxl_col_in_fullres'], positions['pxl_row_in_fullres'])), dtype=np.float64)
    cart = np.array([pseudo_hex_to_cartesian(c) for c in zip(positions['array_col'], positions['array_row'])], dtype=np.float64)
    i, j = np.triu_indices(len(px), k=1)
    px_dist = np.sqrt(np.sum((px[i] - px[j]) ** 2, axis=1))
    cart_dist = np.sqrt(np.sum((cart[i] - cart[j]) ** 2, axis=1))
    d100 = np.mean(px_dist / cart_dist)
    return int(np.rint(distance_um * d100 / 100))


# ---------------------------------------------------------------------------------------------- the public functions
def _geometry(img, patch_size, window_size):
    """(P, half) of a call, checked."""
    P = int(patch_size)
    if P <= 0:
        raise ValueError("patch_size must be positive, got %r" % (patch_size,))
    w = _window_size(window_size, P, int(img.shape[1]))
    half = w // 2
    if half < 1:
        raise ValueError("window_size %r gives an empty window (%d pixels)" % (window_size, 2 * half))
    return P, half


def _norm_vector(norm, dev):
    """{mean[3], std[3], 1/std[3]} on `dev`, what the float entry points take."""
    sd = torch.tensor(norm[1], dtype=torch.float32)
    return torch.cat([torch.tensor(norm[0], dtype=torch.float32), sd, 1.0 / sd]).to(dev)


def _host_patch(img, x_px, y_px, half, P, preprocess_xform):
    """One window through Pillow: (3, P, P), the bytes (as they are) or preprocess_xform(to_tensor(patch))."""
    patch = np.array(Image.fromarray(_window(img, x_px, y_px, half)).resize((P, P)))
    if preprocess_xform is not None:
        return preprocess_xform(to_tensor(Image.fromarray(patch)))
    return torch.from_numpy(patch).permute(2, 0, 1)


def grid_from_wsi_visium(fullres_imgfile, spaceranger_dir, patch_size=256, window_size=256, preprocess_xform=None,
                         device=None, raw_uint8=False, remove_cast=False, cast_lut=None):
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
    remove_cast: `remove_color_cast` of the whole decoded slide before the windows are cut - through Pillow on the host path,
        through the kernels on the device path (in place on the upload this call made; a resident tensor that was passed in
        is only read: its `cast_tables` are folded into the gather, nothing slide-sized is allocated).
    cast_lut: a (3, 256) uint8 array or tensor (`cast_tables` of this or another slide, any per-channel byte map): every
        slide byte of channel c counts as cast_lut[c][byte].  The host path applies it to the decoded slide; the device path
        folds it into the gather (gnx_wsi_patch_grid_u8_lut / _u8_f32_lut) and leaves the slide as it is.  Not together with
        remove_cast (ValueError).
    Cells without a spot are zero."""
    cast_lut = _check_cast_lut(cast_lut, remove_cast)
    img = _decode_slide(fullres_imgfile)
    ydim, xdim = int(img.shape[0]), int(img.shape[1])
    P, half = _geometry(img, patch_size, window_size)
    if device is None and raw_uint8:
        raise ValueError("raw_uint8=True returns the grid on a HIP device: pass device=")
    norm = None
    if device is not None and preprocess_xform is not None and not raw_uint8:
        norm = _device_norm(preprocess_xform)
    spots = _spot_table(spaceranger_dir, ydim, xdim)

    if device is not None:
        dev = torch.device(device)
        if raw_uint8:
            return _grid_on_device(img, spots, half, P, dev, None, False, remove_cast, cast_lut)
        if norm is None:            # the patch bytes as float32 0..255: the uint8 grid, converted (exact) where it lies
            return _grid_on_device(img, spots, half, P, dev, None, False, remove_cast, cast_lut).float()
        return _grid_on_device(img, spots, half, P, dev, _norm_vector(norm, dev), True, remove_cast, cast_lut)

    if torch.is_tensor(img):
        img = img.cpu().numpy()
    if remove_cast:
        img = np.array(remove_color_cast(Image.fromarray(img)))
    if cast_lut is not None:
        img = _apply_luts_host(img, _lut_host(cast_lut), np.empty_like(img))
    img_tensor = torch.zeros((VISIUM_H_ST, VISIUM_W_ST, 3, P, P))
    for x_px, y_px, y_ind, x_ind in spots.tolist():
        img_tensor[y_ind, x_ind] = _host_patch(img, x_px, y_px, half, P, preprocess_xform)
    return img_tensor.float()


def patches_from_wsi(slide, centres, patch_size=256, window_size=None, device=None, raw_uint8=False, cast_lut=None,
                     preprocess_xform=None, out=None):
    """The patches of `grid_from_wsi_visium` for an explicit list of centres: (N, 3, patch_size, patch_size), row i the window
    around centres[i] = (x_px, y_px) (integers, full-resolution pixels), resized - the same gather with a 1 x N grid.

    slide: path of the image or the decoded slide (numpy / torch uint8 (Hs, Ws, 3); a HIP tensor is only read).
    window_size, device, raw_uint8, cast_lut, preprocess_xform: as in `grid_from_wsi_visium`, and the same refusals: a centre
        outside the slide, a window above 4x the patch on the device, a slide that is not RGB.
    out: the tensor to fill instead of a new one - a contiguous view of N rows (N, 3, P, P) of the result's dtype on `device`
        (the host for device=None), e.g. rows of one batch buffer filled from several slides.  It is returned."""
    cast_lut = _check_cast_lut(cast_lut, False)
    img = _decode_slide(slide)
    ydim, xdim = int(img.shape[0]), int(img.shape[1])
    P, half = _geometry(img, patch_size, window_size)
    if device is None and raw_uint8:
        raise ValueError("raw_uint8=True returns the patches on a HIP device: pass device=")
    norm = None
    if device is not None and preprocess_xform is not None and not raw_uint8:
        norm = _device_norm(preprocess_xform)
    centres = np.asarray(centres)
    if centres.size == 0:
        centres = centres.reshape(0, 2)
    if centres.ndim != 2 or centres.shape[1] != 2 or not np.issubdtype(centres.dtype, np.integer):
        raise ValueError("centres must be N pairs of integers (x_px, y_px), got %s of shape %s" % (centres.dtype, centres.shape))
    N = len(centres)
    for i, (x_px, y_px) in enumerate(centres.tolist()):
        if not (0 <= x_px < xdim and 0 <= y_px < ydim):
            raise ValueError("centre %d: (x %d, y %d) lies outside the %d x %d slide" % (i, x_px, y_px, xdim, ydim))
    want_dtype = torch.uint8 if raw_uint8 else torch.float32
    want_dev = torch.device('cpu') if device is None else torch.device(device)
    if out is not None:
        same_dev = out.device.type == want_dev.type and (want_dev.index is None or out.device.index == want_dev.index)
        if tuple(out.shape) != (N, 3, P, P) or out.dtype != want_dtype or not out.is_contiguous() or not same_dev:
            raise ValueError("out must be a contiguous %s tensor of shape %s on %s, got %s %s on %s%s"
                             % (want_dtype, (N, 3, P, P), want_dev, out.dtype, tuple(out.shape), out.device,
                                "" if out.is_contiguous() else " (not contiguous)"))

    if device is not None:
        spots = np.zeros((N, 4), dtype=np.int32)
        spots[:, :2] = centres
        spots[:, 3] = np.arange(N)
        if N == 0:
            return out if out is not None else torch.zeros((0, 3, P, P), device=want_dev, dtype=want_dtype)
        as_float = norm is not None
        direct = out if (out is not None and (raw_uint8 or as_float)) else None
        got = _grid_on_device(img, spots, half, P, want_dev, _norm_vector(norm, want_dev) if as_float else None, as_float,
                              False, cast_lut, grid=(1, N), out=None if direct is None else direct.view(1, N, 3, P, P))
        got = got.view(N, 3, P, P)
        if raw_uint8 or as_float:
            return got
        return got.float() if out is None else out.copy_(got)      # the bytes as float32 0..255 (exact)

    if torch.is_tensor(img):
        img = img.cpu().numpy()
    if cast_lut is not None:
        img = _apply_luts_host(img, _lut_host(cast_lut), np.empty_like(img))
    res = out if out is not None else torch.zeros((N, 3, P, P))
    for i, (x_px, y_px) in enumerate(centres.tolist()):
        res[i] = _host_patch(img, x_px, y_px, half, P, preprocess_xform)
    return res


def save_visium_patches(img_file, spaceranger_dir, dest_dir, patch_size=256, window_size=None, device=None, remove_cast=False,
                        cast_lut=None):
    """Write the patch of every spot of one array as "<slide>_<x_vis>_<y_vis>.jpg" under `dest_dir` (Visium indexing, the
    directory layout the patch datasets read); <slide> is the stem of `spaceranger_dir`.  As in the reference a cell is written
    when its patch has a non-zero byte.  With a HIP `device` the patches are cut there and the uint8 grid comes back in one
    copy; the JPEG encoding is the host's either way.  remove_cast, cast_lut: as in `grid_from_wsi_visium`."""
    if device is None:
        patch_grid = grid_from_wsi_visium(img_file, spaceranger_dir, patch_size=patch_size, window_size=window_size,
                                          remove_cast=remove_cast, cast_lut=cast_lut)
        patch_grid = patch_grid.numpy().astype(np.uint8)
    else:
        patch_grid = grid_from_wsi_visium(img_file, spaceranger_dir, patch_size=patch_size, window_size=window_size,
                                          device=device, raw_uint8=True, remove_cast=remove_cast,
                                          cast_lut=cast_lut).cpu().numpy()
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


def save_visium_patches_all(wsi_files, spaceranger_dirs, dest_dir, patch_size=256, window_size=None, device=None,
                            remove_cast=False, cast_lut=None):
    """`save_visium_patches` for several arrays: one sub-directory of `dest_dir` per slide, named by the image file's stem.
    (One cast_lut serves every slide; remove_cast takes each slide's own tables.)"""
    if not os.path.isdir(dest_dir):
        os.mkdir(dest_dir)
    for img_file, srd in zip(wsi_files, spaceranger_dirs):
        print("%s : %s ..." % (img_file, srd))
        slide = str(Path(img_file).stem)
        save_visium_patches(img_file, srd, os.path.join(dest_dir, slide), patch_size, window_size, device=device,
                            remove_cast=remove_cast, cast_lut=cast_lut)
