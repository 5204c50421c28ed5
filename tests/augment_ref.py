"""What the augmentation tests share: Pillow as the oracle (Image.transpose, ImageEnhance, convert('L')), the issue's torch
expression of a code, and seeded inputs.  test_augment_ref_host.py proves the package's CPU form (`transforms.augment_patches`,
`color_tables`, `grey_sums`) equal to Pillow bit for bit; the GPU tests then compare the kernels with that CPU form."""
import numpy as np
import torch
from PIL import Image, ImageEnhance

_T = Image.Transpose if hasattr(Image, 'Transpose') else Image
# code = 4 f + r: out = rot90^r(fliplr^f(x))
PIL_OPS = (None, _T.ROTATE_90, _T.ROTATE_180, _T.ROTATE_270, _T.FLIP_LEFT_RIGHT, _T.TRANSPOSE, _T.FLIP_TOP_BOTTOM, _T.TRANSVERSE)
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FIXED_FACTORS = (0.0, 0.3, 0.5, 1.0, 1.0 + 1e-7, 1.0 - 1e-7, 1.5, 2.0)


def hwc(patch):
    """(3, P, P) uint8 tensor -> (P, P, 3) numpy."""
    return np.ascontiguousarray(patch.permute(1, 2, 0).numpy())


def chw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous()


def pil_code(a, code):
    """Image.transpose of the (P, P, 3) array for a code in 0..7."""
    im = Image.fromarray(a)
    return np.array(im if code == 0 else im.transpose(PIL_OPS[code]))


def torch_code(x, code):
    """The defining expression on (..., P, P)."""
    f, r = (code >> 2) & 1, code & 3
    return torch.rot90(x.flip(-1) if f else x, r, (-2, -1))


def pil_jitter(a, fc, fb):
    """ImageEnhance.Contrast(fc), then ImageEnhance.Brightness(fb), of the (P, P, 3) array."""
    im = ImageEnhance.Contrast(Image.fromarray(a)).enhance(fc)
    return np.array(ImageEnhance.Brightness(im).enhance(fb))


def pil_grey_sum(a):
    return int(np.array(Image.fromarray(a).convert('L')).astype(np.int64).sum())


def patches(n, P, seed):
    """Random uint8 (n, 3, P, P); no symmetry, so every wrong index shows."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 3, P, P), dtype=np.uint8))


def scrambled_codes(n, seed):
    """All eight codes if n >= 8, scrambled, cycled over n patches."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(8) for _ in range(n // 8 + 1)])[:n].astype(np.uint8)


def perm_tables(n, seed):
    """A distinct random permutation table per patch and channel, (n, 3, 256) uint8."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(3 * n)]).astype(np.uint8).reshape(n, 3, 256)
