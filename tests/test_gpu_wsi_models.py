"""`gridnext_amd.imgprocess` with a HIP device: the public functions against their own host path (which
tests/test_imgprocess_host.py pins to the reference's recorded output), on the fixture slide under tests/golden/files/.
Every comparison is torch.equal."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, 'golden', 'files')
SLIDE = os.path.join(FILES, 'wsi_slide.png')
SR2 = os.path.join(FILES, 'wsi_sr2')
SR1 = os.path.join(FILES, 'wsi_sr1')
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


@pytest.mark.parametrize("P,w", [(8, 12), (7, 9), (8, 30), (8, 8), (8, 0.2)])
def test_device_grid_equals_the_host_grid(P, w):
    from gridnext_amd import imgprocess as IP
    from gridnext_amd import transforms as T
    host = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w)
    raw = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w, device=DEV, raw_uint8=True)
    assert raw.dtype == torch.uint8 and raw.device == torch.device(DEV) and tuple(raw.shape) == (78, 64, 3, P, P)
    assert torch.equal(raw.cpu(), host.to(torch.uint8)) and int(raw.view(78, 64, -1).amax(-1).gt(0).sum()) == 15
    flt = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w, device=DEV)
    assert flt.dtype == torch.float32 and flt.device == torch.device(DEV) and torch.equal(flt.cpu(), host)
    # a slide that is already resident, and the headerless position file
    slide = torch.from_numpy(np.array(Image.open(SLIDE))).to(DEV)
    assert torch.equal(IP.grid_from_wsi_visium(slide, SR2, patch_size=P, window_size=w, device=DEV, raw_uint8=True), raw)
    assert torch.equal(IP.grid_from_wsi_visium(slide, SR1, patch_size=P, window_size=w, device=DEV).cpu(),
                       IP.grid_from_wsi_visium(SLIDE, SR1, patch_size=P, window_size=w))
    # Normalize, alone and inside a Compose: the kernel's float form
    norm = T.Normalize(*NORM)
    want = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w, preprocess_xform=norm)
    for xform in (norm, T.Compose([norm]), T.Compose([T.ToTensor(), norm])):
        got = IP.grid_from_wsi_visium(slide, SR2, patch_size=P, window_size=w, preprocess_xform=xform, device=DEV)
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)


def test_device_path_refusals():
    from gridnext_amd import imgprocess as IP
    with pytest.raises(ValueError, match="device=None"):
        IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=8, window_size=34, device=DEV)
    with pytest.raises(ValueError, match="cannot run on the device"):
        IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=8, window_size=8, device=DEV, preprocess_xform=torch.nn.Identity())
    with pytest.raises(RuntimeError, match="HIP device"):
        IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=8, window_size=8, device='cpu')


def test_uint8_grid_through_gridnet_hex_oddr():
    """The device grid is what GridNetHexOddr over a DenseNet consumes as it is: the same logits as the host-extracted bytes."""
    import gridnext_amd as ga
    from gridnext_amd import imgprocess as IP
    P, C = 32, 4
    torch.manual_seed(0)
    f = ga.DenseNet(growth_rate=8, block_config=(2, 2), num_init_features=16, bn_size=2, num_classes=C, small_inputs=False)
    for m in f._bn_modules():
        m.running_mean.normal_(0, 0.1)
        m.running_var.uniform_(0.5, 1.5)
    f.input_norm = NORM
    g = ga.GridNetHexOddr(f, (3, P, P), (IP.VISIUM_H_ST, IP.VISIUM_W_ST), C).to(DEV).eval()
    dev_grid = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=12, device=DEV, raw_uint8=True)
    host_grid = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=12).to(torch.uint8).to(DEV)
    with torch.no_grad():
        got, want = g(dev_grid.unsqueeze(0)), g(host_grid.unsqueeze(0))
    assert got.shape[0] == 1 and got.shape[1] == C and bool(torch.isfinite(want).all())
    assert torch.equal(got, want) and torch.equal(dev_grid, host_grid)


def test_save_visium_patches_on_the_device_writes_the_same_files(tmp_path):
    from gridnext_amd import imgprocess as IP
    a, b = tmp_path / 'host', tmp_path / 'device'
    IP.save_visium_patches(SLIDE, SR2, str(a), patch_size=8, window_size=12)
    IP.save_visium_patches(SLIDE, SR2, str(b), patch_size=8, window_size=12, device=DEV)
    assert sorted(os.listdir(str(a))) == sorted(os.listdir(str(b))) and len(os.listdir(str(a))) == 15
    for name in os.listdir(str(a)):
        assert open(str(a / name), 'rb').read() == open(str(b / name), 'rb').read(), name
