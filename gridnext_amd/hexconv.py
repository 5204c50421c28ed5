"""hexagdly-compatible hexagonal convolution layer backed by the HIP kernel.

`Conv2d` takes the constructor arguments, parameter names (`kernel0`, `kernel1`,
..., `bias_tensor`), shapes and default initialisation of `hexagdly.Conv2d`,
which /root/reference/gridnext/gridnet_models.py:130-147 instantiates with
kernel_size=1, stride=1, bias=True - so `import gridnext_amd.hexconv as hexagdly`
is a drop-in for what GridNext uses, and reference checkpoints load by name.

Any `kernel_size` k >= 1 (hexagdly's radius) is implemented, at stride 1.  A
radius-k layer has 1 + 3k(k+1) taps and the parameters `kernel0 [O][I][2k+1][1]`
(the cell's own column) and `kernel{j} [O][I][2k+1-j][2]` for j = 1..k (the two
columns at distance j, left then right), then `bias_tensor [O]`; the tap
geometry is stated in include/gridnext_hip.h (gnx_hexconv_k_*).  For k = 1 it is
the table the reference's corrector uses, on the size-1 kernels.  PARITY
UNPINNED: hexagdly is not available to run against, so the layout of
k >= 2 follows the package's published sub-convolution decomposition and the
hexagonal geometry, checked by tests against a float64 restatement of that
decomposition - as the size-1 layer is against oracle/hexconv.py.
"""
import numbers

import torch
import torch.nn as nn

from . import functional as GF


class Conv2d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, bias=True, debug=False):
        super().__init__()
        if isinstance(kernel_size, bool) or not isinstance(kernel_size, numbers.Integral) or kernel_size < 1:
            raise ValueError("hexagdly.Conv2d: kernel_size must be an integer >= 1, got %r" % (kernel_size,))
        if stride != 1:
            raise NotImplementedError("hexagdly.Conv2d: only stride=1 is implemented")
        k = int(kernel_size)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.debug = k, stride, debug
        self.kernel0 = nn.Parameter(torch.empty(out_channels, in_channels, 2 * k + 1, 1))
        for j in range(1, k + 1):
            setattr(self, 'kernel%d' % j, nn.Parameter(torch.empty(out_channels, in_channels, 2 * k + 1 - j, 2)))
        if bias:
            self.bias_tensor = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias_tensor', None)
        self.reset_parameters()

    def kernels(self):
        """[kernel0, ..., kernel{kernel_size}] in hexagdly's order."""
        return [getattr(self, 'kernel%d' % j) for j in range(self.kernel_size + 1)]

    def reset_parameters(self):
        if self.debug:
            for p in self.kernels() + [self.bias_tensor]:
                if p is not None:
                    nn.init.constant_(p, 1.0)
        else:
            for p in self.kernels():
                nn.init.xavier_uniform_(p)
            if self.bias_tensor is not None:
                nn.init.constant_(self.bias_tensor, 0.01)

    def forward_nhwc(self, x_nhwc, oddr):
        """Channels-last entry used by the grid models: x [B, H, W, C_in] -> [B, H, W, C_out]."""
        if self.kernel_size == 1:
            return GF.hexconv(x_nhwc, self.kernel0, self.kernel1, self.bias_tensor, oddr)
        return GF.hexconv_k(x_nhwc, self.kernels(), self.bias_tensor, oddr)

    def forward(self, x):
        """hexagdly call convention: x (B, C_in, rows, cols) in hexagdly addressing (odd columns shifted down)."""
        y = self.forward_nhwc(x.permute(0, 2, 3, 1), oddr=False)
        return y.permute(0, 3, 1, 2)

    def extra_repr(self):
        return '%d, %d, kernel_size=%d, stride=%d' % (self.in_channels, self.out_channels, self.kernel_size,
                                                     self.stride)
