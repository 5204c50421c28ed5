"""Training from resident slides: `cast_lut=` / `remove_cast=True` folded into the device gather, `patches_from_wsi`,
`SlideGridDataset` / `SlidePatchDataset` on a HIP device against their own host path (tests/test_slide_datasets_host.py pins that
to Pillow and to `PatchGridDataset`), and the training loops fed by them against the same loops fed the same tensors.
Fixture: the slide and the wsi_sr1 / wsi_sr2 trees under tests/golden/files/; the Loupe CSVs are written from their barcodes.
Every image comparison is torch.equal."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from slide_fixture import SLIDE, SR1, SR2, decoded, write_annots

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _perms(seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8)


@pytest.mark.parametrize("P,w", [(8, 12), (7, 9), (8, 8)])
def test_cast_lut_on_the_device_equals_the_host_path(P, w):
    from gridnext_amd import imgprocess as IP
    from gridnext_amd import transforms as T
    host = decoded()
    resident = torch.from_numpy(host).to(DEV)
    norm = T.Normalize(*NORM)
    for t in (_perms(P * w), IP.cast_tables(host)):
        for kw in (dict(raw_uint8=True), dict(), dict(preprocess_xform=norm)):
            host_kw = {k: v for k, v in kw.items() if k != 'raw_uint8'}
            want = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w, cast_lut=t, **host_kw)
            if 'raw_uint8' in kw:
                want = want.to(torch.uint8)
            for table in (t, torch.from_numpy(t), torch.from_numpy(t).to(DEV)):
                got = IP.grid_from_wsi_visium(resident, SR2, patch_size=P, window_size=w, device=DEV, cast_lut=table, **kw)
                assert got.dtype == want.dtype and got.device == torch.device(DEV) and torch.equal(got.cpu(), want), kw
            got = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w, device=DEV, cast_lut=t, **kw)   # own upload
            assert torch.equal(got.cpu(), want)
    assert torch.equal(resident.cpu(), torch.from_numpy(host))
    # t = cast_tables(slide): remove_cast=True, on a resident tensor and on an upload of the call's own
    t = IP.cast_tables(resident)
    assert np.array_equal(t, IP.cast_tables(host))
    for kw in (dict(raw_uint8=True), dict(), dict(preprocess_xform=norm)):
        a = IP.grid_from_wsi_visium(resident, SR2, patch_size=P, window_size=w, device=DEV, cast_lut=t, **kw)
        b = IP.grid_from_wsi_visium(resident, SR2, patch_size=P, window_size=w, device=DEV, remove_cast=True, **kw)
        c = IP.grid_from_wsi_visium(SLIDE, SR2, patch_size=P, window_size=w, device=DEV, remove_cast=True, **kw)
        assert torch.equal(a, b) and torch.equal(a, c), kw
    with pytest.raises(ValueError, match="remove_cast"):
        IP.grid_from_wsi_visium(resident, SR2, patch_size=P, window_size=w, device=DEV, cast_lut=t, remove_cast=True)
    with pytest.raises(ValueError, match="cast_lut"):
        IP.grid_from_wsi_visium(resident, SR2, patch_size=P, window_size=w, device=DEV, cast_lut=torch.from_numpy(t).to(DEV)[:2])


def test_remove_cast_on_a_resident_slide_reads_it_and_allocates_nothing_of_its_size():
    """A 1 200 x 1 300 slide (4.7 MB) under the fixture's spots at patch 8 (the grid: 0.96 MB): the peak of allocated device
    memory during the call grows by less than one slide.  (The copy the call used to cut from would be 4.7 MB on its own.)"""
    from gridnext_amd import imgprocess as IP
    import colorcast_ref as C
    host = C.tinted((1200, 1300), seed=8)
    resident = torch.from_numpy(host).to(DEV)
    want = IP.grid_from_wsi_visium(host, SR2, patch_size=8, window_size=12, remove_cast=True).to(torch.uint8)
    IP.grid_from_wsi_visium(resident, SR2, patch_size=8, window_size=12, device=DEV, raw_uint8=True)    # (tables, library: warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = IP.grid_from_wsi_visium(resident, SR2, patch_size=8, window_size=12, device=DEV, raw_uint8=True, remove_cast=True)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print("slide %d bytes, grid %d bytes, peak growth %d bytes" % (resident.numel(), got.numel(), growth))
    assert growth < resident.numel()
    assert torch.equal(got.cpu(), want)
    assert torch.equal(resident.cpu(), torch.from_numpy(host))


def test_patches_from_wsi_rows_are_the_grid_cells_and_out_fills_one_buffer_from_two_slides():
    from gridnext_amd import imgprocess as IP
    from gridnext_amd import transforms as T
    host = decoded()
    other = np.ascontiguousarray(host[::-1, :, ::-1])
    a, b = torch.from_numpy(host).to(DEV), torch.from_numpy(other).to(DEV)
    lut = _perms(3)
    spots = IP._spot_table(SR2, host.shape[0], host.shape[1])
    for P, w in ((8, 12), (7, 9), (8, 8)):
        for kw in (dict(raw_uint8=True), dict(), dict(preprocess_xform=T.Normalize(*NORM))):
            grid = IP.grid_from_wsi_visium(a, SR2, patch_size=P, window_size=w, device=DEV, cast_lut=lut, **kw)
            rows = IP.patches_from_wsi(a, spots[:, :2], patch_size=P, window_size=w, device=DEV, cast_lut=lut, **kw)
            assert tuple(rows.shape) == (len(spots), 3, P, P) and rows.dtype == grid.dtype
            assert torch.equal(rows, grid[torch.from_numpy(spots[:, 2]).long(), torch.from_numpy(spots[:, 3]).long()])
            host_kw = {k: v for k, v in kw.items() if k != 'raw_uint8'}
            want = IP.patches_from_wsi(host, spots[:, :2], patch_size=P, window_size=w, cast_lut=lut, **host_kw)
            assert torch.equal(rows.cpu().float() if 'raw_uint8' in kw else rows.cpu(), want)
            # one batch buffer, rows 1..5 from slide a and 5..9 from slide b
            rows_b = IP.patches_from_wsi(b, spots[3:7, :2], patch_size=P, window_size=w, device=DEV, **kw)
            buf = torch.full((10, 3, P, P), 9, device=DEV, dtype=rows.dtype)
            r = IP.patches_from_wsi(a, spots[:4, :2], patch_size=P, window_size=w, device=DEV, cast_lut=lut, out=buf[1:5], **kw)
            assert r.data_ptr() == buf[1:5].data_ptr()
            IP.patches_from_wsi(b, spots[3:7, :2], patch_size=P, window_size=w, device=DEV, out=buf[5:9], **kw)
            assert torch.equal(buf[1:5], rows[:4]) and torch.equal(buf[5:9], rows_b)
            assert bool((buf[0] == 9).all()) and bool((buf[9] == 9).all())
    assert torch.equal(a.cpu(), torch.from_numpy(host))
    with pytest.raises(ValueError, match="outside"):
        IP.patches_from_wsi(a, [(61, 3)], patch_size=8, device=DEV)
    with pytest.raises(ValueError, match="device=None"):
        IP.patches_from_wsi(a, [(30, 20)], patch_size=8, window_size=34, device=DEV)
    with pytest.raises(ValueError, match="out must be"):
        IP.patches_from_wsi(a, [(30, 20)], patch_size=8, device=DEV, raw_uint8=True, out=torch.zeros((1, 3, 8, 8), dtype=torch.uint8))


def _both(cls, annots, **kw):
    import gridnext_amd as ga
    make = getattr(ga, cls)
    args = ([SLIDE, SLIDE], [SR1, SR2], annots)
    return make(*args, device=DEV, **kw), make(*args, device=None, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(remove_cast=True), dict(raw_uint8=False),
                                dict(raw_uint8=False, remove_cast=True, img_transforms='norm')],
                         ids=['uint8', 'uint8_cast', 'float', 'float_cast_norm'])
def test_grid_dataset_on_the_device_equals_the_host_dataset(tmp_path, kw):
    from gridnext_amd import transforms as T
    kw = dict(kw)
    if kw.get('img_transforms') == 'norm':
        kw['img_transforms'] = T.Compose([T.ToTensor(), T.Normalize(*NORM)])
    dev, host = _both('SlideGridDataset', write_annots(tmp_path), patch_size=8, window_size=12, **kw)
    assert len(dev) == len(host) == 2 and list(dev.classes) == list(host.classes)
    for i in range(2):
        (g, l), (hg, hl) = dev[i], host[i]
        assert g.device == torch.device(DEV) and g.dtype == hg.dtype and tuple(g.shape) == (78, 64, 3, 8, 8)
        assert torch.equal(g.cpu(), hg) and torch.equal(l.cpu(), hl) and int((hl > 0).sum()) in (9, 10)


def test_residency_under_a_cap(tmp_path):
    """Two slides of 8 601 bytes each.  No cap: both stay.  A cap that fits one: the least recently used goes.  0: none
    stays.  Three passes over both items give the same bytes each time; the slides kept resident are never written."""
    import gridnext_amd as ga
    host = decoded()
    one = host.size
    want = [ga.SlideGridDataset([SLIDE], [srd], patch_size=8, window_size=12, remove_cast=True)[0][0] for srd in (SR1, SR2)]
    for cap, stays in ((None, [[0]] + [[0, 1]] * 5), (one + 10, [[0], [1]] * 3), (0, [[]] * 6)):
        ds = ga.SlideGridDataset([SLIDE, host], [SR1, SR2], patch_size=8, window_size=12, remove_cast=True, device=DEV,
                                 resident_bytes=cap)
        assert ds.resident() == []
        seen = []
        for _ in range(3):
            for i in (0, 1):
                assert torch.equal(ds[i][0].cpu(), want[i]), (cap, i)
                seen.append(ds.resident())
        assert seen == stays, cap
        for t, _ in ds._src._resident.values():
            assert torch.equal(t.cpu(), torch.from_numpy(host))
    assert torch.equal(ga.SlideGridDataset([SLIDE], [SR1], patch_size=8, device=DEV)[-1][0].cpu(),
                       ga.SlideGridDataset([SLIDE], [SR1], patch_size=8)[0][0])


def test_patch_dataset_items_are_the_labelled_cells(tmp_path):
    from gridnext_amd import imgprocess as IP
    annots = write_annots(tmp_path)
    for kw in (dict(remove_cast=True), dict(raw_uint8=False)):
        grids, _ = _both('SlideGridDataset', annots, patch_size=8, window_size=12, **kw)
        ds, host_ds = _both('SlidePatchDataset', annots, patch_size=8, window_size=12, **kw)
        want = []
        for i, srd in enumerate((SR1, SR2)):
            grid, labels = grids[i]
            for x, y, r, c in IP._spot_table(srd, 47, 61).tolist():
                if labels[r, c] > 0:
                    want.append((grid[r, c], int(labels[r, c]) - 1))
        assert len(ds) == len(host_ds) == len(want) == 19
        for k in range(len(ds)):
            patch, label = ds[k]
            assert patch.device == torch.device(DEV) and torch.equal(patch, want[k][0]) and int(label) == want[k][1]
            assert torch.equal(patch.cpu(), host_ds[k][0]) and int(host_ds[k][1]) == want[k][1]
        idx = [17, 2, 9, 2, 0, 18]
        batch = ds.__getitems__(idx)
        assert torch.equal(torch.stack([p for p, _ in batch]), torch.stack([ds[k][0] for k in idx]))
        assert [int(l) for _, l in batch] == [want[k][1] for k in idx]
        xs, ys = next(iter(DataLoader(ds, batch_size=7, shuffle=False)))
        assert xs.is_cuda and torch.equal(xs, torch.stack([w[0] for w in want[:7]])) and ys.tolist() == [w[1] for w in want[:7]]


def test_worker_refusal(tmp_path):
    import gridnext_amd as ga
    ds = ga.SlideGridDataset([SLIDE], [SR1], patch_size=8, device=DEV)
    real = torch.utils.data.get_worker_info
    torch.utils.data.get_worker_info = lambda: object()        # what a DataLoader worker process sees
    try:
        with pytest.raises(RuntimeError, match="num_workers=0"):
            ds[0]
        with pytest.raises(RuntimeError, match="num_workers=0"):
            ga.SlidePatchDataset([SLIDE], [SR1], patch_size=8, device=DEV)[0]
        assert tuple(ga.SlideGridDataset([SLIDE], [SR1], patch_size=8)[0][0].shape) == (78, 64, 3, 8, 8)    # the host path may
    finally:
        torch.utils.data.get_worker_info = real
    assert ds[0][0].is_cuda


# ------------------------------------------------------------------------------------------------ the loops
P, C = 16, 3


def _grid_model(seed=3):
    import gridnext_amd as ga
    torch.manual_seed(seed)
    f = ga.DenseNet(num_classes=C, growth_rate=8, block_config=(2, 2), num_init_features=16, bn_size=2, small_inputs=True)
    for p in f.parameters():
        p.requires_grad = False
    return ga.GridNetHexOddr(f, (3, P, P), (78, 64), C)


def _grid_loop(dataset, epochs, cached):
    import gridnext_amd as ga
    m = _grid_model()
    if cached:
        m.enable_f_cache()
    dl = {'train': DataLoader(dataset, batch_size=1, shuffle=True, generator=torch.Generator().manual_seed(1)),
          'val': DataLoader(dataset, batch_size=1)}
    opt = torch.optim.Adam(m.corrector.parameters(), lr=1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        m, vh, th = ga.train_gridwise(m, dl, nn.CrossEntropyLoss(), opt, num_epochs=epochs)
    counts = (m.f_cache.hits, m.f_cache.misses) if cached else None
    from gridnext_amd.utils import all_fgd_predictions
    preds = all_fgd_predictions(DataLoader(dataset, batch_size=1), m)
    return th, vh, {k: v.clone() for k, v in m.state_dict().items()}, counts, preds


def test_train_gridwise_from_resident_slides_equals_the_loop_fed_the_same_tensors(tmp_path):
    """One epoch fed by SlideGridDataset == the loop fed the same grids and labels from a TensorDataset: histories and weights.
    Three epochs with enable_f_cache(): 2 arrays x 2 phases x 3 epochs = 12 look-ups of 2 different byte contents - 2 misses in
    the first train phase, 10 hits (the gather is deterministic, the key is the array's bytes) - and the uncached results."""
    import gridnext_amd as ga
    annots = write_annots(tmp_path)
    ds = ga.SlideGridDataset([SLIDE, SLIDE], [SR1, SR2], annots, patch_size=P, window_size=12, device=DEV, remove_cast=True)
    items = [ds[i] for i in range(2)]
    tensors = TensorDataset(torch.stack([g for g, _ in items]), torch.stack([l for _, l in items]).to(DEV))
    th0, vh0, sd0, _, preds0 = _grid_loop(tensors, 1, False)
    th1, vh1, sd1, _, preds1 = _grid_loop(ds, 1, False)
    print("1 epoch: tensors", th0, vh0, "slides", th1, vh1)
    assert len(th0) == 1 and th0 == th1 and vh0 == vh1 and np.isfinite(th0[0]) and list(sd0) == list(sd1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    for a, b in zip(preds0, preds1):
        assert np.array_equal(a, b)
    assert len(preds0[0]) == 19
    th2, vh2, sd2, _, _ = _grid_loop(ds, 3, False)
    th3, vh3, sd3, counts, _ = _grid_loop(ds, 3, True)
    print("3 epochs: uncached", th2, vh2, "cached", th3, vh3, "(hits, misses)", counts)
    assert th2 == th3 and vh2 == vh3 and all(torch.equal(sd2[k], sd3[k]) for k in sd2)
    assert counts == (10, 2)


def test_train_spotwise_from_resident_slides_equals_the_same_batches_from_tensors(tmp_path):
    import gridnext_amd as ga
    annots = write_annots(tmp_path)
    ds = ga.SlidePatchDataset([SLIDE, SLIDE], [SR1, SR2], annots, patch_size=P, window_size=12, device=DEV)
    tensors = TensorDataset(torch.stack([ds[k][0] for k in range(len(ds))]),
                            torch.stack([ds[k][1] for k in range(len(ds))]).to(DEV))
    runs = []
    for data in (tensors, ds):
        torch.manual_seed(4)
        f = ga.DenseNet(num_classes=C, growth_rate=8, block_config=(2, 2), num_init_features=16, bn_size=2, small_inputs=True)
        dl = {'train': DataLoader(data, batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(2)),
              'val': DataLoader(data, batch_size=8)}
        opt = torch.optim.Adam(f.parameters(), lr=1e-3)
        with contextlib.redirect_stdout(io.StringIO()):
            f, vh, th = ga.train_spotwise(f, dl, nn.CrossEntropyLoss(), opt, num_epochs=2)
        runs.append((th, vh, {k: v.clone() for k, v in f.state_dict().items()}))
    print("tensors", runs[0][:2], "slides", runs[1][:2])
    assert len(runs[0][0]) == 2 and all(np.isfinite(v) for v in runs[0][0] + runs[0][1])
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
