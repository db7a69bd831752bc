"""MCNN (dgvcc_amd.models.baselines) on the GPU: outputs and parameter gradients against the
fixtures made by running the reference (tests/golden/make_golden_mcnn.py), eval against training
forward, and one DGTrainer 'simple' step per precision with the pooled-ground-truth MSE count loss.

Fixture rules as tests/test_csrnet_gpu.py: the fixtures hold the reference's float64 run and the
error of its own fp32 run; outputs within max(3 x that error, 1e-4), gradients (normwise over the
stored entries, and over the per-parameter sums) within max(3 x that error, GRAD_FLOOR).
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dg_oracle as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"r32x32": (2, 32, 32),   # the quarter-resolution 7x7 / 5x5 layers run on 8x8 maps
         "r36x44": (2, 36, 44)}   # a 9x11 output, odd in both axes

# Gradient floor: MCNN has no BatchNorm, so tests/test_csrnet_gpu.py's reasoning carries over: the fp32
# layers are exact-f32 MFMA sums of at most 32*49 = 1568 terms, and the floor is the outputs' 1e-4, the
# room one flipped ReLU decision of a near-zero pre-activation needs in a gradient sum.
GRAD_FLOOR = 1e-4


def case_input(name):
    """As make_golden_mcnn.case_input: the top-left H x W corner of the seeded synthetic frames."""
    B, H, W = CASES[name]
    up = lambda v: -(-v // 16) * 16  # noqa: E731
    return O.synthetic_batch(B, up(H), up(W), seed=2112, with_dmap=False)[0][..., :H, :W].contiguous()


def _model(dev, precision="fp32"):
    from dgvcc_amd.models.baselines import MCNN
    m = MCNN(load_weights=True)
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
def test_mcnn_matches_reference(dev, name):
    d = np.load(os.path.join(G, "mcnn.npz"))
    model = _model(dev)
    out = model(case_input(name).to(dev))
    ref = torch.from_numpy(d[f"{name}__out"])
    assert tuple(out.shape) == tuple(ref.shape) and out.dtype == torch.float32
    tol = max(3 * float(d[f"{name}__out__ref32_err"][0]), 1e-4)
    err = ((out.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"MCNN {name} out: err {err:.3e} tol {tol:.3e} (fp32 reference {d[f'{name}__out__ref32_err'][0]:.3e})")
    assert err < tol, (name, err, tol)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(99), dtype=torch.float64).float().to(dev)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert len(grads) == 26
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    a, b, sa, sb = _stored(d, f"{name}__grad__", grads)
    gtol = max(3 * float(d[f"{name}__grad_ref32_err"][0]), GRAD_FLOOR)
    e1, e2 = ((a - b).norm() / b.norm()).item(), ((sa - sb).norm() / sb.norm()).item()
    print(f"MCNN {name} grads: entries {e1:.3e} sums {e2:.3e} tol {gtol:.3e} "
          f"(fp32 reference {d[f'{name}__grad_ref32_err'][0]:.3e})")
    assert e1 < gtol and e2 < gtol, (name, e1, e2, gtol)


def test_mcnn_eval_matches_train_forward(dev):
    """No BatchNorm, no dropout: the eval forward (no tape) computes what the training forward does."""
    model = _model(dev)
    x = case_input("r36x44").to(dev)
    with torch.no_grad():
        a = model(x)
        b = model.eval()(x)
    assert torch.equal(a, b)


def _train_step(dev, precision, batch):
    from dgvcc_amd.losses import MSELoss
    from dgvcc_amd.optim import AdamW
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    m = _model(dev, precision)
    with torch.no_grad():
        pred = m(batch[0].to(dev)).double()
    before = [p.detach().clone() for p in m.parameters()]
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    with tempfile.TemporaryDirectory() as td:
        cwd = os.getcwd()
        os.chdir(td)
        try:
            tr = DGTrainer(2112, "t", dev, 1000, 10000, "simple")
            loss = tr.train_step(m, MSELoss(), opt, batch, 0)
        finally:
            os.chdir(cwd)
    torch.cuda.synchronize()
    moved = [not torch.equal(p.detach(), b) for p, b in zip(m.parameters(), before)]
    return m, pred, loss, moved


def test_mcnn_train_step_fp32(dev):
    """DGTrainer 'simple' + MSELoss + the fused AdamW at 2x3x32x32: the 8x8 prediction meets the
    32x32 ground truth sum-pooled by 4 (count-preserving)."""
    batch = O.synthetic_batch(2, 32, 32, seed=5)
    m, pred, loss, moved = _train_step(dev, "fp32", batch)
    gt = batch[2][1].double().to(dev)
    assert pred.shape == (2, 1, 8, 8) and gt.shape == (2, 1, 32, 32)
    want = ((pred - 16 * F.avg_pool2d(gt, 4) * 1000) ** 2).mean().item()
    assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)
    names = [n for n, _ in m.named_parameters()]
    assert all(moved), [n for n, mv in zip(names, moved) if not mv]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_mcnn_train_step_16bit(dev, precision):
    batch = O.synthetic_batch(2, 32, 32, seed=5)
    m, _, loss, _ = _train_step(dev, precision, batch)
    assert np.isfinite(loss)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
