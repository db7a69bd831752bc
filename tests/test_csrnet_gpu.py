"""CSRNet (dgvcc_amd.models.baselines) on the GPU: outputs and parameter gradients against the
fixtures made by running the reference (tests/golden/make_golden_csrnet.py), how often the layout
kernels launch, and one DGTrainer 'simple' step with the pooled-ground-truth MSE count loss.

Fixture rules as tests/test_models2.py: the fixtures hold the reference's float64 run and the
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
CASES = {"r64x64": (2, 64, 64),   # back end at 8x8: its six dilated layers stay in phase layout
         "r56x72": (2, 56, 72)}   # back end at 7x9, ragged: every dilated layer converts by itself

# Gradient floor.  tests/test_models2.py starts its BN-free DensityRegressorBase at 1e-2 because batch
# statistics over 32..512 pixels amplify near-zero ReLU flips of the fp32 forward.  CSRNet has no
# BatchNorm, and measured on the MI355X against the float64 reference (the reference's own fp32 run:
# 6.6e-7 / 6.4e-7):
#   2x3x64x64 (resident)   stored entries 1.9e-6, per-parameter sums 3.1e-6, output 4.1e-6
#   2x3x56x72 (per layer)  stored entries 2.1e-6, per-parameter sums 1.0e-6, output 3.4e-6
# so the floor is the outputs' 1e-4: ~30x the measured error, the room one flipped ReLU decision in
# a 64-channel layer at 8x8 needs (one of ~1e4 terms of a gradient sum).
GRAD_FLOOR = 1e-4


def case_input(name):
    """As make_golden_csrnet.case_input: the top-left H x W corner of the seeded synthetic frames."""
    B, H, W = CASES[name]
    up = lambda v: -(-v // 16) * 16  # noqa: E731
    return O.synthetic_batch(B, up(H), up(W), seed=2112, with_dmap=False)[0][..., :H, :W].contiguous()


def _model(dev, precision="fp32"):
    from dgvcc_amd.models.baselines import CSRNet
    m = CSRNet()
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


@pytest.fixture
def launch_counts(monkeypatch):
    from dgvcc_amd import kernels as K
    counts = {}
    real = K.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(K, "call", counting)
    return counts


@pytest.mark.parametrize("name", list(CASES))
def test_csrnet_matches_reference(dev, name, launch_counts):
    d = np.load(os.path.join(G, "csrnet.npz"))
    model = _model(dev)
    out = model(case_input(name).to(dev))
    ref = torch.from_numpy(d[f"{name}__out"])
    assert tuple(out.shape) == tuple(ref.shape) and out.dtype == torch.float32
    tol = max(3 * float(d[f"{name}__out__ref32_err"][0]), 1e-4)
    err = ((out.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"CSRNet {name} out: err {err:.3e} tol {tol:.3e} (fp32 reference {d[f'{name}__out__ref32_err'][0]:.3e})")
    assert err < tol, (name, err, tol)
    fwd = dict(launch_counts)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(99), dtype=torch.float64).float().to(dev)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    # 8x8: one conversion each way per pass; 7x9: one each way per dilated layer and pass
    n = 1 if name == "r64x64" else 6
    assert (fwd["dg_space_to_batch"], fwd["dg_batch_to_space"]) == (n, n)
    assert (launch_counts["dg_space_to_batch"], launch_counts["dg_batch_to_space"]) == (2 * n, 2 * n)
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
    a, b, sa, sb = _stored(d, f"{name}__grad__", grads)
    gtol = max(3 * float(d[f"{name}__grad_ref32_err"][0]), GRAD_FLOOR)
    e1, e2 = ((a - b).norm() / b.norm()).item(), ((sa - sb).norm() / sb.norm()).item()
    print(f"CSRNet {name} grads: entries {e1:.3e} sums {e2:.3e} tol {gtol:.3e} "
          f"(fp32 reference {d[f'{name}__grad_ref32_err'][0]:.3e})")
    assert e1 < gtol and e2 < gtol, (name, e1, e2, gtol)


def test_csrnet_eval_matches_train_forward(dev):
    """No BatchNorm, no dropout: the eval forward (no tape) computes what the training forward does."""
    model = _model(dev)
    x = case_input("r64x64").to(dev)
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


def test_csrnet_train_step_fp32(dev, monkeypatch):
    """DGTrainer 'simple' + MSELoss + the fused AdamW at 2x3x64x64: the 8x8 prediction meets the
    64x64 ground truth sum-pooled by 8 (count-preserving), under DGVCC_CHECK_AMAX's operand-maxima
    checks."""
    from dgvcc_amd import kernels as K
    monkeypatch.setattr(K, "_CHECK_AMAX", True)
    batch = O.synthetic_batch(2, 64, 64, seed=5)
    m, pred, loss, moved = _train_step(dev, "fp32", batch)
    gt = batch[2][1].double().to(dev)
    assert pred.shape == (2, 1, 8, 8) and gt.shape == (2, 1, 64, 64)
    want = ((pred - 64 * F.avg_pool2d(gt, 8) * 1000) ** 2).mean().item()
    assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)
    names = [n for n, _ in m.named_parameters()]
    assert all(moved), [n for n, mv in zip(names, moved) if not mv]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_csrnet_train_step_16bit(dev, precision):
    batch = O.synthetic_batch(2, 64, 64, seed=5)
    m, _, loss, _ = _train_step(dev, precision, batch)
    assert np.isfinite(loss)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
