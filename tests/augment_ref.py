"""What the augmentation tests share: Pillow as the oracle (Image.transpose, ImageEnhance, convert('L')), the issue's torch
expression of a code, seeded inputs, and what the GPU tests of both pairs of entry points put their operands on the device
with (nothing here touches a device at import: the host tests import this module too).  test_augment_ref_host.py proves the
package's CPU form (`transforms.augment_patches`, `color_tables`, `grey_sums`) equal to Pillow bit for bit; the GPU tests then
compare the kernels with that CPU form."""
import numpy as np
import torch
from PIL import Image, ImageEnhance

_T = Image.Transpose if hasattr(Image, 'Transpose') else Image
# code = 4 f + r: out = rot90^r(fliplr^f(x))
PIL_OPS = (None, _T.ROTATE_90, _T.ROTATE_180, _T.ROTATE_270, _T.FLIP_LEFT_RIGHT, _T.TRANSPOSE, _T.FLIP_TOP_BOTTOM, _T.TRANSVERSE)
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
FIXED_FACTORS = (0.0, 0.3, 0.5, 1.0, 1.0 + 1e-7, 1.0 - 1e-7, 1.5, 2.0)
DEV = 'cuda:0'
TILE, MAX_BLOCKS = 64, 8192                      # restated from csrc/augment.hip
SENTINEL = 0xA5
BAD_ARG = -1


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


def _codes(n, seed):
    codes = scrambled_codes(n, seed)
    if n == 9:
        assert sorted(codes[:8].tolist()) == list(range(8))
        codes[8] = 8 * 21 + 3                     # acts as its low three bits
    return codes


def _at(host, off, pad=16):
    """The bytes of `host` on the device, `off` bytes into 16-byte aligned storage; (storage, flat uint8 view)."""
    flat = host.contiguous().view(torch.uint8).reshape(-1) if host.dtype != torch.uint8 else host.reshape(-1)
    store = torch.full((off + flat.numel() + pad,), SENTINEL, device=DEV, dtype=torch.uint8)
    assert store.data_ptr() % 16 == 0
    view = store[off:off + flat.numel()]
    view.copy_(flat)
    return store, view


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()
