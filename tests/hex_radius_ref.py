"""Float64 restatement of hexagdly.Conv2d(kernel_size=k, stride=1) for the radius-k tests (test_hex_radius_geometry.py,
test_gpu_hex_radius.py).  Not imported by the package.

Geometry (hexagdly addressing: vertically aligned columns, odd columns shifted down by half a cell; p = column, q = row):
  kernel0 [O][I][2k+1][1]        tap a     -> (dp, dq) = (0, a - k)
  kernel{j} [O][I][2k+1-j][2]    tap (a,b) -> (dp, dq) = ((2b - 1) j, top(j, p) + a),  j = 1..k
  top(j, p) = -k + floor(j/2) + (j odd ? p mod 2 : 0)
Two independent forms: `gather_k` (a shifted gather per tap of that table) and `subconv_k` (hexagdly's published
decomposition into sub-convolutions: kernel0 as a (2k+1) x 1 conv on rows padded by k; kernel{j} as a conv at column dilation 2j
- for odd j separately on the two column parities at column stride 2 - with top pad k - floor(j/2) - (j odd ? parity : 0) and
bottom pad 2k - j - top).  The odd-right Visium grid is the transpose (`oddr`), as oracle/hexconv.py states.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


def n_taps(k):
    return 1 + 3 * k * (k + 1)


def top(k, j, parity):
    return -k + j // 2 + (parity if j % 2 else 0)


def tap_table(k, parity):
    """[(dp, dq, j, a, b)] of a cell whose parity-axis coordinate has `parity`, in hexagdly's parameter order."""
    taps = [(0, a - k, 0, a, 0) for a in range(2 * k + 1)]
    for j in range(1, k + 1):
        for a in range(2 * k + 1 - j):
            for b in (0, 1):
                taps.append(((2 * b - 1) * j, top(k, j, parity) + a, j, a, b))
    return taps


def kernel_shapes(O, I, k):
    return [(O, I, 2 * k + 1, 1)] + [(O, I, 2 * k + 1 - j, 2) for j in range(1, k + 1)]


def gather_k(x, kernels, bias=None):
    """x (B, I, R, C) in hexagdly addressing -> (B, O, R, C)."""
    k = len(kernels) - 1
    B, I, R, C = x.shape
    O = kernels[0].shape[0]
    xp = F.pad(x, (k, k, k, k))
    cols = torch.arange(C, device=x.device)
    out = x.new_zeros((B, O, R, C))
    for parity in (0, 1):
        acc = x.new_zeros((B, O, R, C))
        for dp, dq, j, a, b in tap_table(k, parity):
            w = kernels[j][:, :, a, b]
            sh = xp[:, :, k + dq:k + dq + R, k + dp:k + dp + C]          # x[r + dq, c + dp], zero outside
            acc = acc + torch.einsum('oi,birc->borc', w, sh)
        out = out + acc * ((cols % 2) == parity).to(x.dtype).view(1, 1, 1, C)
    if bias is not None:
        out = out + bias.view(1, O, 1, 1)
    return out


def subconv_k(x, kernels, bias=None):
    """hexagdly's sub-convolution decomposition, x (B, I, R, C) -> (B, O, R, C)."""
    k = len(kernels) - 1
    B, I, R, C = x.shape
    res = F.conv2d(F.pad(x, (0, 0, k, k)), kernels[0], bias)
    for j in range(1, k + 1):
        if j % 2 == 0:
            t = -top(k, j, 0)
            res = res + F.conv2d(F.pad(x, (j, j, t, 2 * k - j - t)), kernels[j], None, dilation=(1, 2 * j))
            continue
        part = torch.zeros_like(res)
        for parity in (0, 1):
            if C - parity <= 0:
                continue                       # no column of this parity
            t = -top(k, j, parity)
            xp = F.pad(x, (j, j, t, 2 * k - j - t))[..., parity:]
            part[..., parity::2] = F.conv2d(xp, kernels[j], None, stride=(1, 2), dilation=(1, 2 * j))
        res = res + part
    return res


def oddr(form, x, kernels, bias=None):
    """The same layer on a Visium odd-right grid (B, I, H, W): hexagdly's column is the Visium row."""
    return form(x.transpose(2, 3), kernels, bias).transpose(2, 3)


class HexConvK64(nn.Module):
    """Float64 twin of gridnext_amd.hexconv.Conv2d(kernel_size=k) in hexagdly addressing (same parameter names: loads its
    state_dict); the oracle's GridNetHexOddr wraps its corrector in the reference's rot90/flip sandwich."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True):
        super().__init__()
        self.kernel_size = kernel_size
        for j, s in enumerate(kernel_shapes(out_channels, in_channels, kernel_size)):
            setattr(self, 'kernel%d' % j, nn.Parameter(torch.zeros(s, dtype=torch.float64)))
        self.bias_tensor = nn.Parameter(torch.zeros(out_channels, dtype=torch.float64)) if bias else None

    def forward(self, x):
        ks = [getattr(self, 'kernel%d' % j) for j in range(self.kernel_size + 1)]
        return gather_k(x, ks, self.bias_tensor)
