"""`SlideGridDataset` / `SlidePatchDataset` with an `Augment` that holds a `SaturationHueJitter`, on a HIP device against their
own host path (device=None) under the same seed and the same batch structure (tests/test_augment_hs_ref_host.py pins the host
path to Pillow); an `Augment` without the step launches what it launched before the step existed; `train_spotwise` fed by the
augmented device dataset against the same loop fed by the host dataset.  Fixture: tests/slide_fixture.py.  Every image
comparison is torch.equal."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from slide_fixture import SLIDE, SR1, SR2, write_annots

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
KWS = [dict(), dict(remove_cast=True), dict(raw_uint8=False), dict(raw_uint8=False, remove_cast=True, img_transforms='norm')]
IDS = ['uint8', 'uint8_cast', 'float', 'float_cast_norm']


def _steps(hs=True):
    from gridnext_amd import transforms as T
    steps = [T.RandomHorizontalFlip(), T.RandomVerticalFlip(), T.ColorJitter(0.3, 0.5), T.RandomQuarterTurn()]
    return steps + [T.SaturationHueJitter(0.4, 0.25)] if hs else steps


def _both(cls, annots, seed, **kw):
    import gridnext_amd as ga
    from gridnext_amd import transforms as T
    kw = dict(kw)
    if kw.get('img_transforms') == 'norm':
        kw['img_transforms'] = T.Compose([T.ToTensor(), T.Normalize(*NORM)])
    make = getattr(ga, cls)
    args = ([SLIDE, SLIDE], [SR1, SR2], annots)
    return (make(*args, device=DEV, augment=T.Augment(_steps(), seed=seed), **kw),
            make(*args, device=None, augment=T.Augment(_steps(), seed=seed), **kw))


@pytest.mark.parametrize("kw", KWS, ids=IDS)
def test_grid_dataset_on_the_device_equals_the_host_dataset(tmp_path, kw):
    from gridnext_amd import imgprocess as IP
    annots = write_annots(tmp_path)
    dev, host = _both('SlideGridDataset', annots, 3, patch_size=8, window_size=12, **kw)
    for epoch in range(2):
        for i, srd in enumerate((SR1, SR2)):
            (g, l), (hg, hl) = dev[i], host[i]
            assert g.device == torch.device(DEV) and g.dtype == hg.dtype and tuple(g.shape) == (78, 64, 3, 8, 8)
            assert torch.equal(g.cpu(), hg) and torch.equal(l.cpu(), hl), (epoch, i)
            spots = IP._spot_table(srd, 47, 61).astype(np.int64)
            empty = torch.ones((78, 64), dtype=torch.bool)
            empty[spots[:, 2], spots[:, 3]] = False
            assert not bool(g.cpu()[empty].any()) and int(empty.sum()) == 78 * 64 - len(spots)       # cells without a spot


@pytest.mark.parametrize("kw", KWS, ids=IDS)
def test_patch_dataset_through_a_dataloader_equals_the_host_dataset(tmp_path, kw):
    dev, host = _both('SlidePatchDataset', write_annots(tmp_path), 4, patch_size=8, window_size=12, **kw)
    assert len(dev) == len(host) == 19
    seen = 0
    for (xs, ys), (hx, hy) in zip(DataLoader(dev, batch_size=5), DataLoader(host, batch_size=5)):
        assert xs.is_cuda and xs.dtype == hx.dtype and torch.equal(xs.cpu(), hx) and torch.equal(ys.cpu(), hy)
        seen += len(ys)
    assert seen == 19
    a, b = dev[7], host[7]                                                   # single items draw too
    assert torch.equal(a[0].cpu(), b[0]) and int(a[1]) == int(b[1])


def test_the_step_changes_the_bytes_and_nothing_else(tmp_path):
    """Saturation-only and hue-only steps, against the same list without the step under the same seed: the step is drawn
    last, so the codes and tables are the same and only the colours differ."""
    import gridnext_amd as ga
    from gridnext_amd import transforms as T
    annots = write_annots(tmp_path)
    args = ([SLIDE, SLIDE], [SR1, SR2], annots)
    plain = ga.SlideGridDataset(*args, patch_size=8, window_size=12, device=DEV, augment=T.Augment(_steps(False), seed=5))[0][0]
    for step in (T.SaturationHueJitter(saturation=0.5), T.SaturationHueJitter(hue=0.3)):
        aug = T.Augment(_steps(False) + [step], seed=5)
        dev = ga.SlideGridDataset(*args, patch_size=8, window_size=12, device=DEV, augment=aug)[0][0]
        host = ga.SlideGridDataset(*args, patch_size=8, window_size=12, device=None,
                                   augment=T.Augment(_steps(False) + [step], seed=5))[0][0]
        assert torch.equal(dev.cpu(), host) and not torch.equal(dev, plain)
        assert torch.equal(dev.flatten(2).any(2), plain.flatten(2).any(2))


def test_two_epochs_differ_and_reseeding_reproduces(tmp_path):
    import gridnext_amd as ga
    from gridnext_amd import transforms as T
    annots = write_annots(tmp_path)
    aug = T.Augment(_steps(), seed=8)
    grid = ga.SlideGridDataset([SLIDE, SLIDE], [SR1, SR2], annots, patch_size=8, window_size=12, device=DEV, augment=aug)
    pats = ga.SlidePatchDataset([SLIDE, SLIDE], [SR1, SR2], annots, patch_size=8, window_size=12, device=DEV, augment=aug)

    def epoch():
        return [grid[i][0].clone() for i in range(2)] + [xs.clone() for xs, _ in DataLoader(pats, batch_size=5)]

    first, second = epoch(), epoch()
    assert all(not torch.equal(a, b) for a, b in zip(first, second))
    aug.manual_seed(8)
    again = epoch()
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for t, _ in grid._src._resident.values():                                # the resident slides are only read
        from slide_fixture import decoded
        assert torch.equal(t.cpu(), torch.from_numpy(decoded()))


def test_the_entry_points_with_and_without_the_step(tmp_path, monkeypatch):
    """The entry points a slide dataset reaches, recorded at `_lib.call`: an Augment without the step makes the calls it made
    before the step existed (the old augmentation entry points only); with the step the one augmentation launch is
    csrc/augment.hip's, and nothing is added to it."""
    import gridnext_amd as ga
    from gridnext_amd import _lib
    from gridnext_amd import transforms as T
    annots = write_annots(tmp_path)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    args = ([SLIDE, SLIDE], [SR1, SR2], annots)
    idx = [17, 2, 9, 2, 0, 18]                                               # items of both slides: one gather per slide
    for raw in (True, False):
        for cast in (False, True):
            kw = dict(patch_size=8, window_size=12, device=DEV, raw_uint8=raw, remove_cast=cast)
            gather = 'gnx_wsi_patch_grid_u8_lut' if cast else 'gnx_wsi_patch_grid_u8'
            old = [gather, 'gnx_patch_grey_sum_u8', 'gnx_patch_augment_u8' if raw else 'gnx_patch_augment_u8_f32']
            new = [gather, 'gnx_patch_grey_sum_u8', 'gnx_patch_augment_hs_u8' if raw else 'gnx_patch_augment_hs_u8_f32']
            neutral = _steps(False) + [T.SaturationHueJitter()]                # an identity step: nothing of it is launched
            for steps, per_gather in ((_steps(False), old), (neutral, old), (_steps(), new)):
                aug = T.Augment(steps, seed=1)
                grid, pats = ga.SlideGridDataset(*args, **kw, augment=aug), ga.SlidePatchDataset(*args, **kw, augment=aug)
                grid[0], grid[1], pats.__getitems__(idx)                     # (the slides' colour-cast tables: once per slide)
                del names[:]
                grid[0]
                assert names == per_gather, (raw, cast, names)
                del names[:]
                pats.__getitems__(idx)
                assert names == per_gather * 2, (raw, cast, names)


P, C = 16, 3


def test_train_spotwise_from_the_augmented_device_dataset_equals_the_loop_fed_by_the_host_dataset(tmp_path):
    """Two epochs of train_spotwise: the augmented SlidePatchDataset on the device against the same loop, the same shuffling
    and the same Augment seed fed by the host dataset (device=None: CPU tensors, uploaded by the loop): equal histories and
    weights.  Both phases of both epochs draw, in the same order on both sides."""
    import gridnext_amd as ga
    from gridnext_amd import transforms as T
    annots = write_annots(tmp_path)
    runs = []
    for device in (None, DEV):
        data = ga.SlidePatchDataset([SLIDE, SLIDE], [SR1, SR2], annots, patch_size=P, window_size=12, device=device,
                                    augment=T.Augment(_steps(), seed=12))
        torch.manual_seed(4)
        f = ga.DenseNet(num_classes=C, growth_rate=8, block_config=(2, 2), num_init_features=16, bn_size=2, small_inputs=True)
        dl = {'train': DataLoader(data, batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(2)),
              'val': DataLoader(data, batch_size=8)}
        opt = torch.optim.Adam(f.parameters(), lr=1e-3)
        with contextlib.redirect_stdout(io.StringIO()):
            f, vh, th = ga.train_spotwise(f, dl, nn.CrossEntropyLoss(), opt, num_epochs=2)
        runs.append((th, vh, {k: v.clone() for k, v in f.state_dict().items()}))
    print("host", runs[0][:2], "device", runs[1][:2])
    assert len(runs[0][0]) == 2 and all(np.isfinite(v) for v in runs[0][0] + runs[0][1])
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
