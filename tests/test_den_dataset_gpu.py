"""DensityMapDataset end to end: dataset -> DataLoader (2 workers, batch 2) ->
DGTrainer('simple').train_step on MCNN (dataset downsample 4: the map arrives on the prediction's
grid) and on CSRNet (downsample 1: the trainer sum-pools the ground truth) at crop 64x64.  The loss
is finite and the parameters move; any other mode raises ValueError before a kernel is launched."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as R
from oracle import dg_oracle as O

pytestmark = pytest.mark.gpu

H, W = 96, 120


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("den_gpu"))
    os.makedirs(os.path.join(root, "train"))
    yy, xx = np.mgrid[0:H, 0:W]
    for n in range(4):
        rng = np.random.default_rng(n)
        pts = np.stack([rng.uniform(0, W - 1, 9), rng.uniform(0, H - 1, 9)], 1)
        d = np.zeros((H, W), dtype=np.float32)
        for x, y in pts:
            g = np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / 8.0)
            d += (g / g.sum()).astype(np.float32)
        stem = os.path.join(root, "train", f"f{n:03d}")
        Image.fromarray(R.test_image(H, W, n)).save(stem + (".jpg" if n % 2 else ".png"))
        np.save(stem + ".npy", pts)
        np.save(stem + "_dmap2.npy", d)
    return root


def _batch(root, downsample):
    from dgvcc_amd.datasets import DensityMapDataset, RawDenBatch
    from dgvcc_amd.utils.misc import seed_worker
    ds = DensityMapDataset(root, 64, downsample, "train", False, 1)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=2, collate_fn=ds.collate,
                                         worker_init_fn=seed_worker, generator=torch.Generator().manual_seed(0))
    raw = next(iter(loader))
    assert isinstance(raw, RawDenBatch) and raw.img_desc.shape == (2, 16) and raw.downsample == downsample
    return raw


def _step(dev, model, raw, mode, tmp_path):
    from dgvcc_amd.losses import MSELoss
    from dgvcc_amd.optim import AdamW
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    model.load_state_dict(O.seeded_state_dict(model.state_dict()))
    model = model.to(dev).set_precision("fp32").train()
    before = [p.detach().clone() for p in model.parameters()]
    opt = AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        tr = DGTrainer(2112, "t", dev, 1000, 10000, mode)
        loss = tr.train_step(model, MSELoss(), opt, raw, 0)
    finally:
        os.chdir(cwd)
    torch.cuda.synchronize()
    return loss, [not torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before)], model


@pytest.mark.parametrize("name,downsample", [("mcnn", 4), ("csrnet", 1)])
def test_train_step_from_the_dataset(dev, root, tmp_path, name, downsample):
    from dgvcc_amd.datasets import DeviceAugment
    from dgvcc_amd.models.baselines import MCNN, CSRNet
    random.seed(3)
    raw = _batch(root, downsample)
    imgs, imgs2, (points, dmaps, empty) = DeviceAugment(dev)(raw)
    assert imgs2 is imgs and imgs.shape == (2, 3, 64, 64) and empty.numel() == 0 and len(points) == 2
    assert dmaps.shape == (2, 1, 64 // downsample, 64 // downsample)
    assert torch.isfinite(imgs).all() and imgs.min() >= -1 and imgs.max() <= 1
    assert torch.isfinite(dmaps).all() and (dmaps >= 0).all() and dmaps.sum() > 0
    model = MCNN(load_weights=True) if name == "mcnn" else CSRNet()
    loss, moved, model = _step(dev, model, raw, "simple", tmp_path)
    assert np.isfinite(loss)
    assert all(moved), [n for (n, _), mv in zip(model.named_parameters(), moved) if not mv]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_other_modes_raise_before_any_launch(dev, root, tmp_path, monkeypatch):
    """Mode 'base' wants two views: ValueError naming the mode, before the batch is put on the device
    (no resize launch) and before the model runs."""
    import dgvcc_amd.datasets.augment as A
    from dgvcc_amd.models.baselines import MCNN
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    raw = _batch(root, 4)
    touched = []
    monkeypatch.setattr(A, "call", lambda name, *a: touched.append(name))
    monkeypatch.setattr(DGTrainer, "prepare_batch", lambda self, b: touched.append("prepare_batch"))
    monkeypatch.setattr(MCNN, "forward", lambda self, x: touched.append("forward"))
    with pytest.raises(ValueError, match="'base'"):
        _step(dev, MCNN(load_weights=True), raw, "base", tmp_path)
    assert touched == []
