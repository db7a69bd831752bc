"""BL's VGG19 counter (dgvcc_amd.models.baselines.BL_VGG) on the GPU: outputs and parameter gradients
against the fixtures made by running the reference (tests/golden/make_golden_blvgg.py), eval against
training forward, one DGTrainer 'simple' step per precision with the pooled-ground-truth MSE count
loss, one with the Bayesian loss on a reference-layout batch against oracle/bl_oracle.py, and the
device-batch branch of DGTrainer.compute_count_loss for a prediction that already is the loss's grid.

Fixture rules as tests/test_csrnet_gpu.py: the fixtures hold the reference's float64 run and the
error of its own fp32 run; outputs within max(3 x that error, 1e-4), gradients (normwise over the
stored entries, and over the per-parameter sums) within max(3 x that error, GRAD_FLOOR).  The output
is |z| with z negative at >= 99% of the pixels and no |z| below 0.025 (the fixture's `__zstat`), so a
plan without the abs misses the output bound by orders of magnitude and no sign can flip under fp32
error.
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dg_oracle as O
from oracle.bl_oracle import bl_loss

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"r16x48": (2, 16, 48),   # 1x3 features: the one-row align-corners upsampling (ratio 0 along H)
         "r48x80": (2, 48, 80)}   # 3x5 features, a 6x10 output: odd in both axes before the upsampling

# Gradient floor.  There is no BatchNorm, so tests/test_csrnet_gpu.py's reasoning carries over: the
# floor is the outputs' 1e-4, the room one flipped ReLU decision of a near-zero pre-activation needs
# in a gradient sum.  Measured on the MI355X against the float64 reference (the reference's own fp32
# run: 2.8e-7 / 6.4e-7 on outputs, 3.3e-7 / 6.3e-7 on gradients):
#   2x3x16x48 (1x3 features)  stored entries 2.5e-7, per-parameter sums 6.9e-7, output 8.9e-7
#   2x3x48x80 (3x5 features)  stored entries 1.9e-6, per-parameter sums 1.1e-6, output 2.8e-6
# ~50x under the floor, so it stays where CSRNet's is.
GRAD_FLOOR = 1e-4


def case_input(name):
    """As make_golden_blvgg.case_input: the top-left H x W corner of the seeded synthetic frames."""
    B, H, W = CASES[name]
    up = lambda v: -(-v // 16) * 16  # noqa: E731
    return O.synthetic_batch(B, up(H), up(W), seed=2112, with_dmap=False)[0][..., :H, :W].contiguous()


def _model(dev, precision="fp32"):
    from dgvcc_amd.models.baselines import BL_VGG
    m = BL_VGG()
    m.load_state_dict(O.seeded_state_dict(m.state_dict()))
    return m.to(dev).set_precision(precision).train()


def _stored(d, prefix, grads):
    a, b, sa, sb = [], [], [], []
    for k, g in grads.items():
        key = prefix + k.replace(".", "__")
        v = g.detach().double().cpu().reshape(-1)
        sa.append(v.sum().reshape(1))
        if key in d.files:
            r = torch.from_numpy(d[key]).double()
            a.append(v)
            b.append(r)
            sb.append(r.sum().reshape(1))
        else:
            a.append(v[torch.from_numpy(d[key + "@idx"])])
            b.append(torch.from_numpy(d[key + "@val"]).double())
            sb.append(torch.tensor([d[key + "@sum"][0]], dtype=torch.float64))
    return torch.cat(a), torch.cat(b), torch.cat(sa), torch.cat(sb)


@pytest.mark.parametrize("name", list(CASES))
def test_blvgg_matches_reference(dev, name):
    d = np.load(os.path.join(G, "blvgg.npz"))
    zmin, zneg = d[f"{name}__zstat"]
    assert zmin > 1e-2 and zneg >= 0.99  # what makes the abs checkable (see the module docstring)
    model = _model(dev)
    out = model(case_input(name).to(dev))
    ref = torch.from_numpy(d[f"{name}__out"])
    B, H, W = CASES[name]
    assert tuple(out.shape) == tuple(ref.shape) == (B, 1, H // 8, W // 8) and out.dtype == torch.float32
    assert bool((out >= 0).all())
    tol = max(3 * float(d[f"{name}__out__ref32_err"][0]), 1e-4)
    err = ((out.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"BL_VGG {name} out: err {err:.3e} tol {tol:.3e} (fp32 reference {d[f'{name}__out__ref32_err'][0]:.3e})")
    assert err < tol, (name, err, tol)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(99), dtype=torch.float64).float().to(dev)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert len(grads) == 38
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    a, b, sa, sb = _stored(d, f"{name}__grad__", grads)
    gtol = max(3 * float(d[f"{name}__grad_ref32_err"][0]), GRAD_FLOOR)
    e1, e2 = ((a - b).norm() / b.norm()).item(), ((sa - sb).norm() / sb.norm()).item()
    print(f"BL_VGG {name} grads: entries {e1:.3e} sums {e2:.3e} tol {gtol:.3e} "
          f"(fp32 reference {d[f'{name}__grad_ref32_err'][0]:.3e})")
    assert e1 < gtol and e2 < gtol, (name, e1, e2, gtol)


def test_blvgg_eval_matches_train_forward(dev):
    """No BatchNorm, no dropout: the eval forward (no tape) computes what the training forward does."""
    model = _model(dev)
    x = case_input("r48x80").to(dev)
    with torch.no_grad():
        a = model(x)
        b = model.eval()(x)
    assert torch.equal(a, b)


def _trainer(dev):
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    with tempfile.TemporaryDirectory() as td:
        cwd = os.getcwd()
        os.chdir(td)
        try:
            return DGTrainer(2112, "t", dev, 1000, 10000, "simple")
        finally:
            os.chdir(cwd)


def _train_step(dev, precision, batch, crit):
    from dgvcc_amd.optim import AdamW
    m = _model(dev, precision)
    with torch.no_grad():
        pred = m(batch[0].to(dev)).double()
    before = [p.detach().clone() for p in m.parameters()]
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    loss = _trainer(dev).train_step(m, crit, opt, batch, 0)
    torch.cuda.synchronize()
    moved = [not torch.equal(p.detach(), b) for p, b in zip(m.parameters(), before)]
    return m, pred, loss, moved


def test_blvgg_train_step_fp32(dev):
    """DGTrainer 'simple' + MSELoss + the fused AdamW at 2x3x32x32: the 4x4 prediction meets the
    32x32 ground truth sum-pooled by 8 (count-preserving)."""
    from dgvcc_amd.losses import MSELoss
    batch = O.synthetic_batch(2, 32, 32, seed=5)
    m, pred, loss, moved = _train_step(dev, "fp32", batch, MSELoss())
    gt = batch[2][1].double().to(dev)
    assert pred.shape == (2, 1, 4, 4) and gt.shape == (2, 1, 32, 32)
    want = ((pred - 64 * F.avg_pool2d(gt, 8) * 1000) ** 2).mean().item()
    assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)
    names = [n for n, _ in m.named_parameters()]
    assert all(moved), [n for n, mv in zip(names, moved) if not mv]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_blvgg_train_step_16bit(dev, precision):
    from dgvcc_amd.losses import MSELoss
    batch = O.synthetic_batch(2, 32, 32, seed=5)
    m, _, loss, _ = _train_step(dev, precision, batch, MSELoss())
    assert np.isfinite(loss)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_blvgg_train_step_bayesian_loss(dev):
    """The network the Bayesian loss was designed for, on the loss's own stride-8 grid: a
    reference-layout batch (points, targets, st_sizes), one image without points; the returned loss is
    oracle/bl_oracle.py's on the pre-step prediction, at test_bl_train_gpu.py's 1e-4."""
    from dgvcc_amd.losses.bl import BL
    imgs = O.synthetic_batch(2, 32, 32, seed=5)[0]
    rng = np.random.default_rng(8)
    pts = [rng.integers(8, 31 * 8, (6, 2)) / 8.0, np.zeros((0, 2))]  # the 1/8-pixel lattice, inside the crop
    tgs = [rng.uniform(0.3, 1.0, 6), np.zeros((0,))]
    st = np.array([32.0, 40.0])
    gt_datas = ([torch.from_numpy(p).float() for p in pts], [torch.from_numpy(t).float() for t in tgs],
                torch.from_numpy(st).float())
    crit = BL(sigma=8, c_size=32, stride=8, background_ratio=1, use_background=True, device=dev)
    m, pred, loss, moved = _train_step(dev, "fp32", (imgs, imgs, gt_datas), crit)
    assert pred.shape == (2, 1, 4, 4)
    want, _ = bl_loss([p.astype(np.float32).astype(np.float64) for p in pts], st,
                      [t.astype(np.float32).astype(np.float64) for t in tgs], pred.cpu().numpy(), 32, 8, 8.0, 1.0,
                      True)
    err = abs(loss - want) / abs(want)
    print(f"BL_VGG Bayesian-loss step: loss {loss:.6f} vs oracle {want:.6f} (rel {err:.2e})")
    assert err <= 1e-4, (loss, want)
    names = [n for n, _ in m.named_parameters()]
    assert all(moved), [n for n, mv in zip(names, moved) if not mv]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_device_batch_takes_a_grid_sized_prediction(dev):
    """compute_count_loss on a device batch (`gt_datas.bl`): a G x G prediction is the grid already, in
    log_para units; the value is the loss on pred / log_para, and its gradient flows back scaled."""
    from dgvcc_amd.datasets.augment import GtDatas
    from dgvcc_amd.losses.bl import BL
    log_para = 1000
    g = torch.Generator().manual_seed(4)
    pts = (torch.rand(5, 2, generator=g).mul(64).to(dev), torch.zeros(0, 2, device=dev))
    tgs = (torch.rand(5, generator=g).mul(0.7).add(0.3).to(dev), torch.zeros(0, device=dev))
    st = torch.tensor([64.0, 64.0], device=dev)
    crit = BL(8.0, 64, 8, 1.0, True, dev)
    tr = _trainer(dev)
    pred = (log_para * torch.rand(2, 1, 8, 8, generator=g)).to(dev).requires_grad_(True)
    got = tr.compute_count_loss(crit, pred, GtDatas(((), None, None), (pts, tgs, st)))
    got.backward()
    ref = pred.detach().clone().requires_grad_(True)
    want = crit(list(pts), st, list(tgs), ref / log_para)
    want.backward()
    err = abs(got.item() - want.item()) / abs(want.item())
    gerr = ((pred.grad - ref.grad).abs().max() / ref.grad.abs().max()).item()
    print(f"grid-sized device batch: loss {got.item():.6f} vs {want.item():.6f} (rel {err:.2e}), grad {gerr:.2e}")
    # pred * f32(1/1000) against pred / 1000: one rounding of the scale and one per element
    assert err <= 1e-6 and gerr <= 1e-6
    # any other shape still raises, naming both sizes
    with pytest.raises(ValueError, match="64x64.*32x32"):
        tr.compute_count_loss(crit, torch.zeros(2, 1, 32, 32, device=dev), GtDatas(((), None, None), (pts, tgs, st)))
    with pytest.raises(ValueError, match="64x64.*8x16"):
        tr.compute_count_loss(crit, torch.zeros(2, 1, 8, 16, device=dev), GtDatas(((), None, None), (pts, tgs, st)))
