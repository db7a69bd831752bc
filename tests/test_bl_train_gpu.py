"""Bayesian-loss training on the GPU: dg_bl_targets against the reference's fixture
(tests/golden/bl_targets.npz), the strided sum pool against torch float64, their composition with
the fused loss through DGTrainer.compute_count_loss against oracle/bl_oracle.py, and one
train_step per trainer mode on a RawDenClsBatch that carries `all_points`."""
import os
import tempfile

import numpy as np
import pytest
import torch

from bl_targets_ref import bl_targets as bl_targets_numpy
from oracle import dg_oracle as O
from oracle.bl_oracle import bl_loss

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIX = dict(np.load(os.path.join(GOLD, "bl_targets.npz")))
CASES = [str(c) for c in FIX["cases"]]


def run_targets(dev, name):
    from dgvcc_amd import kernels as K
    counts = FIX[name + "__counts"]
    _, _, h, w = (int(v) for v in FIX["crop"])
    pts = torch.from_numpy(FIX[name + "__points"].astype(np.float32)).reshape(-1, 2).contiguous().to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
    flips = torch.from_numpy(FIX[name + "__flips"].astype(np.float32)).to(dev)
    out = K.bl_targets(pts, offs, h, w, flips, want_all=True)
    return [t.cpu() for t in out]


# ---- dg_bl_targets ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_bl_targets_match_reference(dev, name):
    kept, targets, offs, d, ratio = run_targets(dev, name)
    want_d, want_ratio = FIX[name + "__d"], FIX[name + "__ratio"]
    want_offs = FIX[name + "__offsets"]
    m = int(want_offs[-1])
    d, ratio = d.double().numpy(), ratio.double().numpy()
    err_d = np.abs(d - want_d) / np.maximum(want_d, 1e-300)
    err_d[want_d == 0] = np.abs(d[want_d == 0])
    print(f"{name}: n {len(want_d)}, kept {m}, d rel err {err_d.max(initial=0):.2e}, "
          f"ratio abs err {np.abs(ratio - want_ratio).max(initial=0):.2e}")
    # the kept index set and the offsets: identical
    assert np.array_equal(ratio >= 0.3, want_ratio >= 0.3)
    assert np.array_equal(offs.numpy(), want_offs)
    # kept points in order, x mirrored where flagged: exact on the 1/8-pixel lattice
    assert np.array_equal(kept[:m].numpy(), FIX[name + "__kept"].astype(np.float32))
    assert err_d.max(initial=0) <= 1e-6
    assert np.abs(ratio - want_ratio).max(initial=0) <= 5e-6
    assert np.abs(targets[:m].double().numpy() - FIX[name + "__targets"]).max(initial=0) <= 5e-6
    # the targets are the kept points' ratios
    assert np.array_equal(targets[:m].numpy(), ratio[ratio >= 0.3].astype(np.float32))


@pytest.mark.parametrize("name", ["n1200", "batch"])
def test_bl_targets_are_deterministic(dev, name):
    a, b = run_targets(dev, name), run_targets(dev, name)
    m = int(a[2][-1])
    assert torch.equal(a[2], b[2])
    assert torch.equal(a[0][:m], b[0][:m]) and torch.equal(a[1][:m], b[1][:m])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


def test_bl_targets_read_flip_flags_from_the_parameter_records(dev):
    """The flip flags may be a strided column of the [B,16] augmentation records."""
    from dgvcc_amd import kernels as K
    from dgvcc_amd.datasets.augment import P
    counts = FIX["batch__counts"]
    pts = torch.from_numpy(FIX["batch__points"].astype(np.float32)).contiguous().to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
    params = torch.full((len(counts), 16), 7.0, device=dev)
    params[:, P["flip"]] = torch.from_numpy(FIX["batch__flips"].astype(np.float32)).to(dev)
    kept, targets, koffs = K.bl_targets(pts, offs, 64, 64, params[:, P["flip"]:P["flip"] + 1])
    m = int(FIX["batch__offsets"][-1])
    assert np.array_equal(koffs.cpu().numpy(), FIX["batch__offsets"])
    assert np.array_equal(kept[:m].cpu().numpy(), FIX["batch__kept"].astype(np.float32))


def test_bl_batch_costs_one_device_to_host_copy(dev):
    """The kernels' wrappers never wait for the device; building the loss's batch from a raw batch
    waits once, for the B + 1 offsets that split the kept points."""
    import warnings
    from dgvcc_amd import kernels as K
    from dgvcc_amd.datasets.augment import bl_batch, new_record
    from dgvcc_amd.losses.bl import sum_pool
    counts = FIX["batch__counts"]
    images = np.split(FIX["batch__points"].astype(np.float32), np.cumsum(counts)[:-1])
    pts = torch.from_numpy(FIX["batch__points"].astype(np.float32)).contiguous().to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
    params = torch.from_numpy(np.stack([new_record(flip=bool(f)) for f in FIX["batch__flips"]])).to(dev)
    pred = torch.rand(4, 1, 64, 64, device=dev, requires_grad=True)
    gy = torch.rand(4, 1, 8, 8, device=dev)
    all_points = tuple(torch.from_numpy(p) for p in images)
    st_sizes = torch.full((4,), 64.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any device-to-host copy or .item() raises
    try:
        K.bl_targets(pts, offs, 64, 64, params[:, 1:2])
        sum_pool(pred, 8, 1e-3).backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            kept, targets, st = bl_batch(all_points, st_sizes, params, 64, 64, dev)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()
             and "prototype" not in str(w.message)]
    assert len(syncs) == 1, syncs
    assert [len(p) for p in kept] == list(np.diff(FIX["batch__offsets"]))


# ---- sum pool --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,s", [((2, 24, 40), 1), ((2, 24, 40), 2), ((2, 24, 40), 8), ((1, 64, 64), 8)])
def test_sum_pool_matches_float64(dev, shape, s):
    from dgvcc_amd.losses.bl import sum_pool
    B, H, W = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 1, H, W, generator=g)
    scale = 1e-3
    scale32 = float(np.float32(scale))  # the kernel's scale argument is a float
    xd = x.to(dev).requires_grad_(True)
    y = sum_pool(xd, s, scale)
    assert y.shape == (B, 1, H // s, W // s)
    win = x.double().reshape(B, 1, H // s, s, W // s, s)
    want = scale32 * win.sum(dim=(3, 5))
    bound = 1e-6 * scale32 * win.abs().sum(dim=(3, 5))
    err = (y.detach().cpu().double() - want).abs()
    print(f"sum pool {shape} s={s}: worst err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    gy = torch.randn(B, 1, H // s, W // s, generator=g)
    y.backward(gy.to(dev))
    want_gx = (np.float32(scale32) * gy).repeat_interleave(s, dim=2).repeat_interleave(s, dim=3)
    assert torch.equal(xd.grad.cpu(), want_gx)  # a broadcast times scale: exact


def test_sum_pool_rejects_sizes_that_do_not_divide(dev):
    from dgvcc_amd.losses.bl import sum_pool
    with pytest.raises(ValueError):
        sum_pool(torch.zeros(1, 1, 30, 32, device=dev), 8)


# ---- composition: targets -> pool -> fused loss ------------------------------------------------
def lattice(rng, n, x0, x1, y0, y1):
    return np.stack([rng.integers(int(x0 * 8), int(x1 * 8), n) / 8.0,
                     rng.integers(int(y0 * 8), int(y1 * 8), n) / 8.0], 1)


def few_kept_image(seed=5):
    """Annotations of one 64 x 64 crop of which at most 9 are kept (so the trimmed sum keeps
    every row: ceil(0.9 * (L - 1)) = L - 1 for L - 1 <= 9) and several fall away, with every ratio
    clear of 0.3."""
    for s in range(seed, seed + 100):
        rng = np.random.default_rng(s)
        pts = np.concatenate([lattice(rng, 7, 4, 60, 4, 60), lattice(rng, 6, -40, -4, -40, 100),
                              lattice(rng, 4, 70, 200, 0, 64)])
        kept, targets, offs, d, ratio, keep = bl_targets_numpy([pts], 64.0, 64.0, [1])
        if 1 <= keep.sum() <= 9 and keep.sum() < len(pts) and np.abs(ratio - 0.3).min() > 1e-3:
            return pts
    raise AssertionError("no seed gives a usable image")


def trainer(dev, mode):
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    with tempfile.TemporaryDirectory() as td:
        cwd = os.getcwd()
        os.chdir(td)
        try:
            return DGTrainer(2112, "t", dev, 1000, 10000, mode)
        finally:
            os.chdir(cwd)


def test_count_loss_composition_matches_oracle(dev):
    from dgvcc_amd.datasets.augment import GtDatas, bl_batch, new_record
    from dgvcc_amd.losses.bl import BL
    log_para = 1000
    images = [few_kept_image(), np.zeros((0, 2))]
    flips = [1, 0]
    params = torch.from_numpy(np.stack([new_record(flip=bool(f)) for f in flips])).to(dev)
    st_sizes = torch.tensor([64.0, 64.0])
    bl = bl_batch(tuple(torch.from_numpy(p).float() for p in images), st_sizes, params, 64, 64, dev)
    kept, targets, offs, _, _, _ = bl_targets_numpy(images, 64.0, 64.0, flips)
    assert [len(p) for p in bl[0]] == list(np.diff(offs)) and 1 <= offs[1] <= 9 and offs[2] == offs[1]
    assert np.array_equal(bl[0][0].cpu().numpy(), kept.astype(np.float32))

    g = torch.Generator().manual_seed(11)
    pred = (log_para * torch.rand(2, 1, 64, 64, generator=g)).to(dev).requires_grad_(True)
    crit = BL(8.0, 64, 8, 1.0, True, dev)
    tr = trainer(dev, "simple")
    gt_datas = GtDatas(((), None, None), bl)
    loss = tr.compute_count_loss(crit, pred, gt_datas)
    loss.backward()

    dens = (pred.detach().cpu().double() / log_para).reshape(2, 1, 8, 8, 8, 8).sum(dim=(3, 5)).numpy()
    want, grad = bl_loss([kept, np.zeros((0, 2))], st_sizes.numpy(), [targets, np.zeros((0,))], dens,
                         64, 8, 8.0, 1.0, True)
    want_grad = torch.from_numpy(grad).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3) / log_para
    err_l = abs(loss.item() - want) / abs(want)
    err_g = (pred.grad.cpu().double() - want_grad).abs().max().item() / want_grad.abs().max().item()
    print(f"composition: loss {loss.item():.6f} vs {want:.6f} (rel {err_l:.2e}), grad err {err_g:.2e}")
    assert err_l <= 1e-4
    assert err_g <= 3e-4


def test_count_loss_rejects_a_prediction_off_the_grid(dev):
    from dgvcc_amd.datasets.augment import GtDatas
    from dgvcc_amd.losses.bl import BL
    tr = trainer(dev, "simple")
    bl = ((torch.zeros(0, 2, device=dev),), (torch.zeros(0, device=dev),), torch.tensor([64.0], device=dev))
    with pytest.raises(ValueError, match="64x64.*32x32"):
        tr.compute_count_loss(BL(8.0, 64, 8, 1.0, True, dev), torch.zeros(1, 1, 32, 32, device=dev),
                              GtDatas(((), None, None), bl))


def test_reference_layout_batches_take_the_old_branch(dev):
    """gt_datas without `.bl` is the reference's (points, targets, st_sizes) with a grid-sized map."""
    from dgvcc_amd.datasets.augment import DeviceAugment, RawDenClsBatch, new_record
    from dgvcc_amd.losses.bl import BL
    crit = BL(8.0, 64, 8, 1.0, True, dev)
    tr = trainer(dev, "simple")
    g = torch.Generator().manual_seed(2)
    pts = [torch.rand(5, 2, generator=g) * 64, torch.zeros(0, 2)]
    tg = [torch.rand(5, generator=g), torch.zeros(0)]
    st = torch.tensor([64.0, 64.0])
    dens = torch.rand(2, 1, 8, 8, generator=g).to(dev)
    got = tr.compute_count_loss(crit, dens, (pts, tg, st))
    want = crit([p.to(dev) for p in pts], st.to(dev), [t.to(dev) for t in tg], dens)
    assert got.item() == want.item()
    # and a raw batch without all_points still augments to the plain triple
    raw = RawDenClsBatch(torch.zeros(2, 64, 64, 3, dtype=torch.uint8), torch.from_numpy(np.stack([new_record()] * 2)),
                         (torch.zeros(0, 2), torch.zeros(0, 2)), torch.zeros(2, 1, 64, 64))
    gt_datas = DeviceAugment(dev)(raw)[2]
    assert type(gt_datas) is tuple and not hasattr(gt_datas, "bl")


# ---- plumbing: one train_step per mode ---------------------------------------------------------
def raw_batch(with_all_points):
    from dgvcc_amd.datasets.augment import RawDenClsBatch, new_record
    rng = np.random.default_rng(21)
    imgs = torch.from_numpy(rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8))
    params = torch.from_numpy(np.stack([new_record(flip=True), new_record(flip=False)]))
    all_points = [lattice(rng, 30, -20, 90, -20, 90), lattice(rng, 3, 10, 50, 10, 50)]
    points = []
    for p, flip in zip(all_points, (True, False)):
        q = p[(p[:, 0] >= 0) & (p[:, 0] <= 64) & (p[:, 1] >= 0) & (p[:, 1] <= 64)].copy()
        if flip:
            q[:, 0] = 64 - q[:, 0]
        points.append(torch.from_numpy(q).float())
    dmaps = torch.from_numpy(rng.random((2, 1, 64, 64)).astype(np.float32) * 1e-3)
    dmaps[1, :, :32] = 0  # some empty 16 x 16 blocks for the class map
    raw = RawDenClsBatch(imgs, params, tuple(points), dmaps)
    if with_all_points:
        raw.all_points = tuple(torch.from_numpy(p).float() for p in all_points)
        raw.st_sizes = torch.tensor([64.0, 80.0])
    return raw


def one_step(dev, model_name, mode, crit, raw, **kw):
    from dgvcc_amd.models import models as M
    model = getattr(M, model_name)(pretrained=False, **kw)
    sd0 = O.seeded_state_dict(model.state_dict())
    model.load_state_dict(sd0)
    model = model.to(dev).set_precision("fp32").train()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    tr = trainer(dev, mode)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.0)
    loss = tr.train_step(model, crit, opt, raw, 0)
    has_grad = {k for k, p in model.named_parameters() if p.grad is not None}
    moved = {k for k, p in model.named_parameters() if not torch.equal(p.detach(), before[k])}
    finite = all(torch.isfinite(p).all().item() for p in model.parameters())
    return loss, has_grad, moved, finite, [k for k, _ in model.named_parameters()]


@pytest.mark.parametrize("model_name,mode,kw", [("DGModel_base", "simple", dict(den_dropout=0.0)),
                                                ("DGModel_final", "final", dict(den_dropout=0.0, cls_dropout=0.0))])
def test_train_step_with_bl(dev, model_name, mode, kw):
    from dgvcc_amd.losses import MSELoss
    from dgvcc_amd.losses.bl import BL
    loss, has_grad, moved, finite, names = one_step(dev, model_name, mode, BL(8.0, 64, 8, 1.0, True, dev),
                                                    raw_batch(True), **kw)
    _, mse_grad, _, _, _ = one_step(dev, model_name, mode, MSELoss(), raw_batch(False), **kw)
    print(f"{mode}: BL step loss {loss:.6f}, {len(has_grad)} parameters with a gradient, {len(moved)} moved")
    assert np.isfinite(loss) and finite
    assert mse_grad and mse_grad <= has_grad, sorted(mse_grad - has_grad)
    # no weight decay: a parameter moves only through its gradient, down to the first convolution
    assert names[0] in moved and names[0] in has_grad, names[0]
    assert len(moved) >= len(has_grad) // 2, (len(moved), len(has_grad))
