"""Image-patch datasets feeding the f∘g path (API surface of /root/reference/gridnext/image_datasets.py).

`PatchDataset` (:20-122): one item per annotated spot image -> (patch (3, P, P) float32 in [0, 1], label int64);
`PatchGridDataset` (:125-232): one item per array -> (patches (H_ST, W_ST, 3, P, P) float32, zeros where the array has
no spot image; labels (H_ST, W_ST) int64, class id + 1, 0 = background).  Spot images are files named
"*_<array_x>_<array_y>.<ext>" inside one directory per array; Visium array coordinates are mapped to odd-right grid
positions.  The default transform is torchvision's `ToTensor()` semantics (uint8 HWC -> float CHW / 255) written out
here because torchvision is not a dependency of this package; any callable taking a PIL image can be passed instead.

New here: `SlideGridDataset` / `SlidePatchDataset` yield the same items cut straight out of the whole-slide images
(`imgprocess`): no patch files; on a HIP device the slides stay resident and every item is one gather.
"""
import glob
import os
import re
from pathlib import Path

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from . import transforms as _transforms
from .count_datasets import _check_files, _label_names, read_annotfile
from .utils import pseudo_hex_to_oddr

Image.MAX_IMAGE_PIXELS = None


def to_tensor(img):
    """PIL image -> float32 CHW in [0, 1] (what torchvision.transforms.ToTensor does for 8-bit images)."""
    arr = np.array(img)                       # copy: PIL's buffer is read-only
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1)
    return t.float().div(255) if t.dtype == torch.uint8 else t.float()


def to_tensor_u8(img):
    """PIL image -> uint8 CHW, NOT divided: the / 255 of ToTensor then happens on the device, inside the stem kernel
    (`gridnext_amd.DenseNet` takes uint8 patches; a quarter of the bytes over PCIe and out of HBM)."""
    arr = np.array(img)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    if arr.dtype != np.uint8:
        raise TypeError("raw_uint8 needs 8-bit images (got %s)" % arr.dtype)
    return torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).contiguous()


def _preprocess(img_transforms, raw_uint8):
    """(per-image callable, device transform or None) of a dataset.  `raw_uint8` with a `transforms.Compose` that has a device
    plan: decode only - uint8 patches at their stored size - and hand the transform on as `dataset.device_transform`
    (`DenseNet.set_input_transform`); such a Compose without a device plan is refused, naming the step.  Everything else:
    the given callable, or ToTensor / its uint8 form."""
    if img_transforms is None:
        return (to_tensor_u8 if raw_uint8 else to_tensor), None
    if raw_uint8 and isinstance(img_transforms, _transforms.Compose):
        if img_transforms.device_plan() is None:
            raise ValueError("raw_uint8=True needs a transform that can run on the device ([Resize] [CenterCrop] ToTensor "
                             "[Normalize]): %s" % img_transforms.device_plan_refusal())
        return to_tensor_u8, img_transforms
    return img_transforms, None


def _spot_labels(annot_file, position_file, Visium, afile_delim, class_names):
    if Visium:
        coords, strs = read_annotfile(annot_file, position_file=position_file, Visium=True, afile_delim=afile_delim)
        return dict(zip(coords, np.searchsorted(class_names, strs)))
    coords, ids = read_annotfile(annot_file, Visium=False, afile_delim=afile_delim)
    return dict(zip(coords, ids))


class PatchDataset(Dataset):
    def __init__(self, img_files, annot_files=None, position_files=None, Visium=True,
                 img_transforms=None, afile_delim=',', img_ext='jpg', verbose=False, raw_uint8=False):
        super().__init__()
        self.raw_uint8 = raw_uint8            # addition: yield uint8 patches (ToTensor's / 255 is fused into the stem kernel)
        _check_files(img_files, annot_files, position_files, Visium, 'img_files')
        names = None
        if Visium and annot_files is not None:
            names = _label_names(annot_files, position_files, ',')
            self.classes = names
        self.afile_delim = afile_delim
        self.imgpath_mapping, self.annotations = [], []
        skipped = 0
        if annot_files is not None:
            for i, (imdir, afile) in enumerate(zip(img_files, annot_files)):
                lookup = _spot_labels(afile, position_files[i] if Visium else None, Visium, afile_delim, names)
                for imfile in glob.glob(os.path.join(imdir, '*.' + img_ext)):
                    cstr = '_'.join(Path(imfile).stem.split('_')[-2:])
                    if cstr not in lookup:
                        skipped += 1
                        if verbose:
                            print(cstr, 'image patch missing annotation (skipping)')
                        continue
                    self.annotations.append(lookup[cstr])
                    self.imgpath_mapping.append(imfile)
        else:
            for imdir in img_files:
                self.imgpath_mapping += glob.glob(os.path.join(imdir, '*.' + img_ext))
        self.preprocess, self.device_transform = _preprocess(img_transforms, raw_uint8)
        if annot_files is not None and verbose:
            print('%d image patches without annotation' % skipped)

    def __len__(self):
        return len(self.imgpath_mapping)

    def __getitem__(self, idx):
        img = self.preprocess(Image.open(self.imgpath_mapping[idx]))
        label = torch.tensor(self.annotations[idx]).long() if len(self.annotations) > 0 else torch.empty(0)
        return (img if self.raw_uint8 else img.float()), label


class PatchGridDataset(Dataset):
    def __init__(self, img_files, annot_files=None, position_files=None, Visium=True,
                 img_transforms=None, afile_delim=',', img_ext='jpg', h_st=78, w_st=64, raw_uint8=False):
        super().__init__()
        self.raw_uint8 = raw_uint8            # addition: yield a uint8 patch grid (245 MB instead of 981 MB at 128 px)
        _check_files(img_files, annot_files, position_files, Visium, 'img_files')
        if Visium and annot_files is not None:
            self.classes = _label_names(annot_files, position_files, ',')
        self.img_files, self.annot_files, self.position_files = img_files, annot_files, position_files
        self.h_st, self.w_st, self.Visium = h_st, w_st, Visium
        self.afile_delim, self.img_ext = afile_delim, img_ext
        self.preprocess, self.device_transform = _preprocess(img_transforms, raw_uint8)

    def __len__(self):
        return len(self.img_files)

    def __getitem__(self, idx):
        lookup = None
        if self.annot_files is not None:
            lookup = _spot_labels(self.annot_files[idx], self.position_files[idx] if self.Visium else None,
                                  self.Visium, self.afile_delim, getattr(self, 'classes', None))
        grid = None
        labels = torch.zeros((self.h_st, self.w_st), dtype=torch.int64)
        pattern = re.compile(r".*_(\d+)_(\d+)\.%s$" % re.escape(self.img_ext))
        for fname in sorted(os.listdir(str(self.img_files[idx]))):
            hit = pattern.match(fname)
            if hit is None:
                continue
            ax, ay = int(hit.group(1)), int(hit.group(2))
            patch = self.preprocess(Image.open(os.path.join(self.img_files[idx], fname)))
            if grid is None:
                grid = torch.zeros((self.h_st, self.w_st) + tuple(patch.shape),
                                   dtype=torch.uint8 if self.raw_uint8 else torch.float32)
            x, y = pseudo_hex_to_oddr(ax, ay) if self.Visium else (ax, ay)
            if lookup is not None:
                cstr = '%d_%d' % (ax, ay)
                if cstr in lookup:
                    labels[y, x] = int(lookup[cstr]) + 1            # 0 is reserved for background
            grid[y, x] = patch
        return (grid if self.raw_uint8 else grid.float()), labels.long()


# ---------------------------------------------------------------------------------------------- arrays straight from slides
class _SlideSource:
    """What `SlideGridDataset` and `SlidePatchDataset` share: the slides (decoded on first use; on a HIP device resident under a
    least-recently-used byte cap), and per slide, computed once and kept whatever the cap, the spot table, the labels and - with
    remove_cast - the colour-cast tables.  A resident slide is only ever read: the table is folded into the gather
    (imgprocess: `cast_lut=`), so one slide serves any patch and window size."""

    def __init__(self, wsi_files, spaceranger_dirs, annot_files, patch_size, window_size, device, remove_cast, img_transforms,
                 raw_uint8, afile_delim, resident_bytes, augment=None):
        from . import imgprocess as IP
        if augment is not None and not isinstance(augment, _transforms.Augment):
            raise TypeError("augment must be a transforms.Augment or None, got %r" % (augment,))
        self.augment = augment
        self._cells = {}                                     # slide index -> int32 [n] row * grid width + col (device or host)
        if len(wsi_files) != len(spaceranger_dirs):
            raise ValueError('Length of wsi_files and spaceranger_dirs must match.')
        self.wsi_files, self.spaceranger_dirs, self.annot_files = list(wsi_files), list(spaceranger_dirs), annot_files
        self.position_files = [IP.visium_find_position_file(d) for d in self.spaceranger_dirs]
        _check_files(self.wsi_files, annot_files, self.position_files, True, 'wsi_files')
        self.patch_size, self.window_size = int(patch_size), window_size
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != 'cuda':
            raise RuntimeError("device=%s: the device path runs on a HIP device only; device=None is the host path" % self.device)
        self.remove_cast, self.raw_uint8, self.afile_delim = bool(remove_cast), bool(raw_uint8), afile_delim
        if resident_bytes is not None and resident_bytes < 0:
            raise ValueError("resident_bytes must be None (no cap) or >= 0, got %r" % (resident_bytes,))
        self.resident_bytes = resident_bytes
        # the transform: None; with raw_uint8 a Compose with a device plan, handed on; without, [ToTensor] [Normalize]
        self.device_transform, self._norm = None, None
        if img_transforms is not None:
            if raw_uint8:
                if not isinstance(img_transforms, _transforms.Compose):
                    raise ValueError("img_transforms %r: with raw_uint8=True only a transforms.Compose that can run on the "
                                     "device ([Resize] [CenterCrop] ToTensor [Normalize]) is handed on" % (img_transforms,))
                _, self.device_transform = _preprocess(img_transforms, True)
            else:
                steps = list(img_transforms.transforms) if isinstance(img_transforms, _transforms.Compose) else [img_transforms]
                if not (len(steps) == 1 and isinstance(steps[0], _transforms.ToTensor)):
                    try:
                        self._norm = IP._device_norm(img_transforms)
                    except ValueError:
                        raise ValueError("img_transforms %r: a slide dataset computes ToTensor, or [ToTensor] Normalize (three "
                                         "channels), itself; a transform that resizes or crops needs raw_uint8=True"
                                         % (img_transforms,)) from None
        if annot_files is not None:
            self.classes = _label_names(annot_files, self.position_files, ',')
        self._spots = [None] * len(self.wsi_files)          # int32 [n][4] {x_px, y_px, grid_row, grid_col}
        self._luts = [None] * len(self.wsi_files)           # (3, 256) uint8, host (and on the device once used there)
        self._dev_luts = [None] * len(self.wsi_files)
        self._resident, self._clock = {}, 0                 # slide index -> [tensor, last use]
        self._norm_dev = None

    # ---- per slide, once
    def spots(self, i):
        if self._spots[i] is None:
            from . import imgprocess as IP
            src = self.wsi_files[i]
            if torch.is_tensor(src) or isinstance(src, np.ndarray):
                ydim, xdim = int(src.shape[0]), int(src.shape[1])
            else:
                with Image.open(src) as im:                  # the header: nothing is decoded
                    xdim, ydim = im.size
            self._spots[i] = IP._spot_table(self.spaceranger_dirs[i], ydim, xdim)
        return self._spots[i]

    def spot_labels(self, i):
        """int64 [n]: class id + 1 of spot k of `spots(i)`, 0 for a spot without annotation (PatchGridDataset's rule, the
        coordinate string being the one `save_visium_patches` names the spot's file by)."""
        from . import imgprocess as IP
        spots = self.spots(i)
        labels = np.zeros(len(spots), dtype=np.int64)
        if self.annot_files is not None:
            lookup = _spot_labels(self.annot_files[i], self.position_files[i], True, self.afile_delim, self.classes)
            for k, (_, _, y_ind, x_ind) in enumerate(spots.tolist()):
                cstr = '%d_%d' % IP.oddr_to_pseudo_hex(x_ind, y_ind)
                if cstr in lookup:
                    labels[k] = int(lookup[cstr]) + 1
        return labels

    def _decode(self, i):
        from . import imgprocess as IP
        return IP._decode_slide(self.wsi_files[i])

    def cast_lut(self, i, slide):
        """The slide's colour-cast tables (None without remove_cast): computed from `slide` the first time, then kept."""
        if not self.remove_cast:
            return None
        if self._luts[i] is None:
            from . import imgprocess as IP
            self._luts[i] = IP.cast_tables(slide)
        if self.device is None:
            return self._luts[i]
        if self._dev_luts[i] is None:
            self._dev_luts[i] = torch.from_numpy(self._luts[i]).to(self.device)
        return self._dev_luts[i]

    # ---- the slide
    def slide(self, i):
        """Slide i where the gather reads it: a numpy array (device=None), else a tensor on the device, resident under the cap."""
        if self.device is None:
            img = self._decode(i)
            return img.cpu().numpy() if torch.is_tensor(img) else img
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError("a slide dataset on a HIP device cuts its patches on that device in the calling process: use "
                               "DataLoader(num_workers=0)")
        self._clock += 1
        hit = self._resident.get(i)
        if hit is not None:
            hit[1] = self._clock
            return hit[0]
        img = self._decode(i)
        img = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
        size = img.numel()
        cap = self.resident_bytes
        if cap is not None:                                  # least recently used out, until this one fits (or none is left)
            while self._resident and sum(t.numel() for t, _ in self._resident.values()) + size > cap:
                del self._resident[min(self._resident, key=lambda k: self._resident[k][1])]
        t = img.to(self.device).contiguous()
        if cap is None or size <= cap:
            self._resident[i] = [t, self._clock]
        return t

    def resident(self):
        """Indices of the slides that are resident now."""
        return sorted(self._resident)

    def norm(self):
        if self._norm is None or self.device is None:
            return None
        if self._norm_dev is None:
            from . import imgprocess as IP
            self._norm_dev = IP._norm_vector(self._norm, self.device)
        return self._norm_dev

    def gather(self, i, spots, grid, out=None, raw=None):
        """`grid` + (3, P, P) of slide i: one gather on the current stream (device), or the per-window Pillow call (host).
        raw: the bytes (True) or the floats (False) whatever the dataset yields; None: what it yields."""
        from . import imgprocess as IP
        raw = self.raw_uint8 if raw is None else raw
        slide = self.slide(i)
        P, half = IP._geometry(slide, self.patch_size, self.window_size)
        lut = self.cast_lut(i, slide)
        if self.device is not None:
            return IP._grid_on_device(slide, spots, half, P, self.device, None if raw else self.norm(), not raw, False, lut,
                                      grid=grid, out=out)
        if lut is not None:
            slide = IP._apply_luts_host(slide, lut, np.empty_like(slide))
        xform = None
        if not raw:
            xform = (lambda t: t) if self._norm is None else _transforms.Normalize(*self._norm)
        res = out if out is not None else torch.zeros(tuple(grid) + (3, P, P), dtype=torch.uint8 if raw else torch.float32)
        for x_px, y_px, r, c in np.asarray(spots).tolist():
            res[r, c] = IP._host_patch(slide, x_px, y_px, half, P, xform)
        return res

    def augmented(self, i, spots, out, out_rows=None):
        """The patches at `spots` (their rows and columns are ignored) of slide i, gathered as bytes into a compact scratch
        buffer (1, n), then written by `self.augment.apply` - one draw for the n patches, in the order of `spots` - to the
        rows `out_rows` (None: 0 .. n - 1) of `out`: bytes, or with raw_uint8=False the floats of the dataset's transform."""
        n, P = len(spots), self.patch_size
        if n == 0:
            return out
        compact = np.array(spots, dtype=np.int32).reshape(n, 4)
        compact[:, 2], compact[:, 3] = 0, np.arange(n)
        scratch = torch.empty((1, n, 3, P, P), dtype=torch.uint8, device='cpu' if self.device is None else self.device)
        self.gather(i, compact, (1, n), out=scratch, raw=True)
        norm = None if self.raw_uint8 else (self._norm if self.device is None else self.norm())
        return self.augment.apply(scratch[0], out=out, out_rows=out_rows, out_float=not self.raw_uint8, norm=norm)

    def batch(self, picks):
        """(buffer (B, 3, P, P), rows): the patches of `picks`, a batch of (slide, x_px, y_px), from ONE gather per slide into one
        buffer - the picks stably sorted by slide; pick b is buffer[rows[b]].  With `augment` the gather of a slide goes to a
        scratch buffer and `Augment.apply` - one draw per slide of the batch, for its patches in batch order - writes the rows."""
        P = self.patch_size
        buf = torch.empty((len(picks), 3, P, P), dtype=torch.uint8 if self.raw_uint8 else torch.float32,
                          device='cpu' if self.device is None else self.device)
        order = sorted(range(len(picks)), key=lambda b: picks[b][0])                      # by slide, stable
        rows = [None] * len(picks)
        at = 0
        while at < len(order):
            slide = picks[order[at]][0]
            end = at
            while end < len(order) and picks[order[end]][0] == slide:
                end += 1
            n = end - at
            spots = np.zeros((n, 4), dtype=np.int32)
            for j in range(n):
                _, spots[j, 0], spots[j, 1] = picks[order[at + j]]
                spots[j, 3] = j
                rows[order[at + j]] = at + j
            if self.augment is not None:
                self.augmented(slide, spots, buf[at:end])
            else:
                self.gather(slide, spots, (1, n), out=buf[at:end].view(1, n, 3, P, P))
            at = end
        return buf, rows

    def cells(self, i, width):
        """int32 [n]: grid_row * width + grid_col of the spots of slide i, where `Augment.apply` reads it (kept per slide)."""
        if i not in self._cells:
            spots = self.spots(i).astype(np.int64)
            cells = torch.from_numpy((spots[:, 2] * width + spots[:, 3]).astype(np.int32))
            self._cells[i] = cells if self.device is None else cells.to(self.device)
        return self._cells[i]


class SlideGridDataset(Dataset):
    """One item per array, cut straight out of its whole-slide image: (grid (78, 64, 3, P, P), labels (78, 64) int64) - what
    `PatchGridDataset` yields over the files `save_visium_patches_all` writes, without the files: no JPEG is encoded or
    decoded, the bytes are Pillow's resize of the slide's windows as they are.

    wsi_files / spaceranger_dirs: per array, the full-resolution image (a path, or a decoded uint8 (Hs, Ws, 3) array / tensor)
        and Spaceranger's output directory (its tissue_positions*.csv is found with `visium_find_position_file`).
    annot_files: Loupe annotation CSVs, or None (all labels 0).  Labels follow `PatchGridDataset`: class id + 1 at the
        odd-right cell of every in-tissue spot that has an annotation, 0 elsewhere; `classes` as there.  Stated difference: an
        in-tissue spot whose patch is all zero keeps its label (`save_visium_patches` writes no file for it).
    patch_size, window_size, remove_cast: as in `imgprocess.grid_from_wsi_visium` (window_size=None: patch_size).
    device: None - the host path, a CPU grid.  A HIP device - slide i is decoded and uploaded on first use and stays resident;
        `resident_bytes` caps the sum of resident slides (None: no cap; 0: upload per item and release; least recently used
        goes first).  Every item is then ONE gather on the current stream, with the slide's colour-cast tables (computed once)
        folded in when remove_cast: a resident slide is never written.  Not inside a DataLoader worker: num_workers=0.
    raw_uint8=True: the bytes.  False: float32 - ToTensor (/ 255), then Normalize when img_transforms is [ToTensor] Normalize -
        the floats `PatchGridDataset` yields for the same bytes (the _f32 form of the gather on a device).
    img_transforms: with raw_uint8=True a `transforms.Compose` with a device plan ([Resize] [CenterCrop] ToTensor [Normalize])
        is handed on as `dataset.device_transform` for `DenseNet.set_input_transform` (the stored size is patch_size); any
        other callable raises, naming it.
    augment: None - every path allocates and launches exactly what it does without the argument.  A `transforms.Augment` -
        train-time flips, quarter turns and brightness / contrast jitter of every patch: the gather writes the bytes of the
        in-tissue spots into a compact scratch buffer, and `Augment.apply` draws once per spot, in the spot table's order, and
        writes the item from it (`gnx_patch_augment_u8` / `_u8_f32` on a device, torch ops on the host; with raw_uint8=False
        the floats of the dataset's transform of the augmented bytes).  Cells without a spot stay zero.  device=None takes the
        same draws: equal seeds and an equal order of items give equal items on the host and on the device, bit for bit.  An
        augmented array has new bytes every epoch, so a frozen classifier's row cache (`enable_f_cache`) misses every time."""

    def __init__(self, wsi_files, spaceranger_dirs, annot_files=None, patch_size=256, window_size=None, device=None,
                 remove_cast=False, img_transforms=None, raw_uint8=True, afile_delim=',', resident_bytes=None, augment=None):
        super().__init__()
        self._src = _SlideSource(wsi_files, spaceranger_dirs, annot_files, patch_size, window_size, device, remove_cast,
                                 img_transforms, raw_uint8, afile_delim, resident_bytes, augment)
        self.raw_uint8, self.device_transform = self._src.raw_uint8, self._src.device_transform
        if annot_files is not None:
            self.classes = self._src.classes
        self.h_st, self.w_st = 78, 64
        self._labels = {}

    def __len__(self):
        return len(self._src.wsi_files)

    def resident(self):
        return self._src.resident()

    def __getitem__(self, idx):
        idx = range(len(self))[idx]
        spots = self._src.spots(idx)
        if idx not in self._labels:
            labels = torch.zeros((self.h_st, self.w_st), dtype=torch.int64)
            if len(spots):
                labels[torch.from_numpy(spots[:, 2].astype(np.int64)), torch.from_numpy(spots[:, 3].astype(np.int64))] = \
                    torch.from_numpy(self._src.spot_labels(idx))
            self._labels[idx] = labels
        if self._src.augment is not None:
            src = self._src
            grid = torch.zeros((self.h_st, self.w_st, 3, src.patch_size, src.patch_size),
                               dtype=torch.uint8 if src.raw_uint8 else torch.float32,
                               device='cpu' if src.device is None else src.device)
            return src.augmented(idx, spots, grid, src.cells(idx, self.w_st)), self._labels[idx].clone()
        return self._src.gather(idx, spots, (self.h_st, self.w_st)), self._labels[idx].clone()


class SlidePatchDataset(Dataset):
    """One item per annotated in-tissue spot, cut straight out of its slide: (patch (3, P, P), label int64) - `PatchDataset`
    without the files.  Arguments as `SlideGridDataset`.  With annot_files=None every in-tissue spot is an item and the label
    is an empty tensor, as in `PatchDataset`.  Arrays come in the order given, the spots of an array in the order of its
    position file.  `__getitem__` is a one-centre gather; `__getitems__` (what a DataLoader's fetcher calls with a batch of
    indices) makes ONE gather per slide into one (B, 3, P, P) buffer and returns its rows.  With `augment` the gather of a slide
    goes to a scratch buffer and `Augment.apply` - one draw per slide of the batch, for its patches in batch order - writes
    the buffer's rows from it; the draws depend on how the items are batched."""

    def __init__(self, wsi_files, spaceranger_dirs, annot_files=None, patch_size=256, window_size=None, device=None,
                 remove_cast=False, img_transforms=None, raw_uint8=True, afile_delim=',', resident_bytes=None, augment=None):
        super().__init__()
        self._src = _SlideSource(wsi_files, spaceranger_dirs, annot_files, patch_size, window_size, device, remove_cast,
                                 img_transforms, raw_uint8, afile_delim, resident_bytes, augment)
        self.raw_uint8, self.device_transform = self._src.raw_uint8, self._src.device_transform
        if annot_files is not None:
            self.classes = self._src.classes
        self.items, self.annotations = [], []               # (slide, x_px, y_px) and, with annotations, the class id
        for i in range(len(self._src.wsi_files)):
            spots, labels = self._src.spots(i), self._src.spot_labels(i)
            for k, (x_px, y_px, _, _) in enumerate(spots.tolist()):
                if annot_files is None:
                    self.items.append((i, x_px, y_px))
                elif labels[k] > 0:
                    self.items.append((i, x_px, y_px))
                    self.annotations.append(int(labels[k]) - 1)

    def __len__(self):
        return len(self.items)

    def resident(self):
        return self._src.resident()

    def _label(self, idx):
        return torch.tensor(self.annotations[idx]).long() if len(self.annotations) > 0 else torch.empty(0)

    def __getitem__(self, idx):
        return self.__getitems__([idx])[0]

    def __getitems__(self, indices):
        indices = [range(len(self))[int(k)] for k in indices]
        buf, rows = self._src.batch([self.items[k] for k in indices])
        return [(buf[rows[b]], self._label(indices[b])) for b in range(len(indices))]
