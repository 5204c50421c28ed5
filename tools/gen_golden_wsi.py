#!/usr/bin/env python3
"""Golden vectors for gridnext_amd.imgprocess: writes a small synthetic slide and two Spaceranger-style position trees under
tests/golden/files/ and records what the REFERENCE's grid_from_wsi_visium returns for them (tests/golden/wsi_grid.npz).
Build container only (imports /root/reference, read-only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_wsi.py

The reference's imgprocess imports torchvision.transforms, which is not installed: a stand-in module with the four names it
uses (Compose, ToPILImage, ToTensor, Normalize - torchvision's arithmetic for 8-bit RGB) is injected into sys.modules first.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class _ToPILImage:
    def __call__(self, t):                      # uint8 CHW tensor -> PIL RGB
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[0] == 3
        return Image.fromarray(np.ascontiguousarray(t.permute(1, 2, 0).numpy()))


class _ToTensor:
    def __call__(self, img):                    # PIL 8-bit -> float32 CHW in [0, 1]
        return torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(255)


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean = torch.tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return (t - mean) / std


tv = types.ModuleType('torchvision')
tvt = types.ModuleType('torchvision.transforms')
tvt.Compose, tvt.ToPILImage, tvt.ToTensor, tvt.Normalize = _Compose, _ToPILImage, _ToTensor, _Normalize
tv.transforms = tvt
sys.modules['torchvision'], sys.modules['torchvision.transforms'] = tv, tvt
sys.path.insert(0, '/root/reference')
from gridnext.imgprocess import grid_from_wsi_visium      # noqa: E402

FILES = os.path.join(ROOT, 'tests', 'golden', 'files')
HS, WS = 47, 61
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (patch_size, window_size)
PAIRS = [(8, 8), (8, None), (8, 12), (12, 8), (8, 5), (8, 30), (7, 9), (8, 0.2)]

# the slide: random bytes over a gradient, so that a shifted or mirrored window shows
rng = np.random.RandomState(11)
yy, xx = np.mgrid[0:HS, 0:WS]
slide = np.stack([(4 * xx) % 256, (5 * yy) % 256, (3 * xx + 2 * yy) % 256], -1).astype(np.int64)
slide = ((slide + rng.randint(0, 64, size=slide.shape)) % 256).astype(np.uint8)
slide[slide == 0] = 1                           # (no all-zero patch: save_visium_patches would skip the cell)
os.makedirs(FILES, exist_ok=True)
Image.fromarray(slide).save(os.path.join(FILES, 'wsi_slide.png'))

# (barcode, in_tissue, array_row, array_col, pxl_row, pxl_col): array_col has the parity of array_row (Visium pseudo-hex)
SPOTS = [
    ('CORNER_TL-1', 1, 0, 0, 0, 0),
    ('CORNER_TR-1', 1, 0, 126, 0, WS - 1),
    ('CORNER_BL-1', 1, 77, 1, HS - 1, 0),
    ('CORNER_BR-1', 1, 77, 127, HS - 1, WS - 1),
    ('EDGE_TOP-1', 1, 0, 60, 0, 30),
    ('EDGE_LEFT-1', 1, 38, 0, 23, 0),
    ('EDGE_RIGHT-1', 1, 39, 127, 23, WS - 1),
    ('EDGE_BOTTOM-1', 1, 77, 61, HS - 1, 30),
    ('INNER_A-1', 1, 20, 40, 15, 20),
    ('INNER_B-1', 1, 21, 41, 16, 33),
    ('INNER_C-1', 1, 40, 70, 25, 40),
    ('INNER_D-1', 1, 50, 30, 30, 17),
    ('NEAR_EDGE-1', 1, 10, 10, 3, 2),
    ('OUTSIDE_TISSUE-1', 0, 30, 30, 20, 20),
    ('HALF_EVEN-1', 1, 60, 20, 20.5, 24.5),     # .5 on an even integer: rounds down (20, 24)
    ('HALF_ODD-1', 1, 61, 21, 21.5, 25.5),      # .5 on an odd integer: rounds up (22, 26)
]

v2 = os.path.join(FILES, 'wsi_sr2', 'spaceranger', 'outs', 'spatial')
v1 = os.path.join(FILES, 'wsi_sr1', 'outs', 'spatial')
os.makedirs(v2, exist_ok=True)
os.makedirs(v1, exist_ok=True)
with open(os.path.join(v2, 'tissue_positions.csv'), 'w') as fh:
    fh.write('barcode,in_tissue,array_row,array_col,pxl_row_in_fullres,pxl_col_in_fullres\n')
    for s in SPOTS:
        fh.write('%s,%d,%d,%d,%s,%s\n' % s)
with open(os.path.join(v1, 'tissue_positions_list.csv'), 'w') as fh:      # Spaceranger < 2: no header, integer pixels
    for s in SPOTS[:14]:
        fh.write('%s,%d,%d,%d,%d,%d\n' % s)

out = {'pairs': np.array([[p, -1 if w is None else w] for p, w in PAIRS], dtype=np.float64)}
slide_file = os.path.join(FILES, 'wsi_slide.png')


def reference_grid(srd, P, w, xform=None):
    with contextlib.redirect_stdout(io.StringIO()):
        g = grid_from_wsi_visium(slide_file, srd, patch_size=P, window_size=w, preprocess_xform=xform)
    assert g.dtype == torch.float32 and tuple(g.shape) == (78, 64, 3, P, P)
    return g


for i, (P, w) in enumerate(PAIRS):
    g = reference_grid(os.path.join(FILES, 'wsi_sr2'), P, w)
    assert bool((g == g.round()).all()) and float(g.min()) >= 0 and float(g.max()) <= 255      # integral, 0..255
    out['grid_%d' % i] = g.numpy().astype(np.uint8)
    print('pair', (P, w), 'filled cells', int((g.reshape(78, 64, -1).amax(-1) > 0).sum()))
g = reference_grid(os.path.join(FILES, 'wsi_sr1'), 8, 12)
out['grid_sr1_8_12'] = g.numpy().astype(np.uint8)
g = reference_grid(os.path.join(FILES, 'wsi_sr2'), 4, 6, _Normalize(MEAN, STD))
out['grid_norm_4_6'] = g.numpy()
out['norm_mean'], out['norm_std'] = np.array(MEAN), np.array(STD)
path = os.path.join(ROOT, 'tests', 'golden', 'wsi_grid.npz')
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path), 'bytes')
