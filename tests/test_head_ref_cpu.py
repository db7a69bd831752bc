"""The float64 restatements of tests/head_ref.py against float64 torch autograd and torch.optim.AdamW.  No GPU."""
import numpy as np
import pytest
import torch

import head_ref as HR

TOL = 1e-12


def _close(a, b, what="", tol=TOL):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), (what, err)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("use_bias", [False, True])
def test_head_against_autograd(act, use_bias):
    g = torch.Generator().manual_seed(11 + act)
    M, C = 37, 24
    x = torch.randn(M, C, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(1, generator=g, dtype=torch.float64).requires_grad_(True) if use_bias else None
    gy = torch.randn(M, generator=g, dtype=torch.float64)
    old = torch.randn(M, C, generator=g, dtype=torch.float64)
    s = x @ w + (b[0] if use_bias else 0.0)
    y = torch.relu(s) if act == 1 else torch.sigmoid(s) if act == 2 else s
    (y * gy).sum().backward()
    yr, sr, a = HR.head_fwd(x, w, b, act)
    _close(yr, y.detach(), "y")
    assert (a >= sr.abs() - 1e-12).all()
    r = HR.head_bwd(x, w, act, yr, gy, old)
    _close(r["gx"], x.grad + old, "gx")
    _close(r["gw"], w.grad, "gw")
    if use_bias:
        _close(r["gbias"], b.grad[0], "gbias")
    assert (r["gw_terms"] >= r["gw"].abs() - 1e-12).all() and r["gbias_terms"] >= r["gbias"].abs() - 1e-12
    _close(HR.head_bwd(x, w, act, yr, gy)["gx"], x.grad, "gx without accumulation")


@pytest.mark.parametrize("gt_scale,coef", [(1.0, 1.0), (1000.0, 0.37)])
def test_mse_against_autograd(gt_scale, coef):
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(257, generator=g, dtype=torch.float64).requires_grad_(True)
    gt = torch.rand(257, generator=g, dtype=torch.float64) * 1e-2
    loss = torch.nn.functional.mse_loss(pred, gt * gt_scale)
    (coef * loss).backward()
    r = HR.mse(pred, gt, gt_scale, coef)
    _close(r["loss"], loss.detach(), "loss")
    _close(r["dpred"], pred.grad, "dpred")


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adamw_against_torch(wd):
    """5 steps of torch.optim.AdamW in float64, the gradient exactly zero on some elements (from step 1 on: m =
    v = 0 there and the update is the decay alone)."""
    g = torch.Generator().manual_seed(7)
    n = 64
    p = torch.nn.Parameter(torch.randn(n, generator=g, dtype=torch.float64))
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pr, m, v = p.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        grad = torch.randn(n, generator=g, dtype=torch.float64)
        grad[::5] = 0.0
        p.grad = grad.clone()
        opt.step()
        r = HR.adamw(pr, grad, m, v, lr, b1, b2, eps, wd, step)
        pr, m, v = r["p"], r["m"], r["v"]
        _close(pr, p.detach(), f"p step {step}")
        st = opt.state[p]
        _close(m, st["exp_avg"], f"m step {step}")
        _close(v, st["exp_avg_sq"], f"v step {step}")
    _close(pr[::5], p.detach()[::5], "zero-gradient elements")
    assert torch.equal(m[::5], torch.zeros_like(m[::5])) and torch.equal(v[::5], torch.zeros_like(v[::5]))


def test_adamw_decay_factor_has_one_f32_value():
    """The hyper-parameters of the GPU cases: 1 - lr wd in f32 is the same value whether the product is rounded
    first or fused into the subtraction, so 'exactly p (1 - lr wd)' names one number."""
    lr = np.float32(1e-3)
    for wd in (0.0, 1e-4, 1e-2):
        wd = np.float32(wd)
        two = np.float32(np.float32(1.0) - np.float32(lr * wd))
        one = np.float32(1.0 - float(lr) * float(wd))
        assert two == one, (wd, two, one)


def test_tanh_against_autograd():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(100, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(100, generator=g, dtype=torch.float64)
    y = torch.tanh(x)
    (y * gy).sum().backward()
    _close(HR.tanh_fwd(x), y.detach(), "tanh")
    old = torch.randn(100, generator=g, dtype=torch.float64)
    gx, g0, _ = HR.tanh_bwd(y.detach(), gy, old)
    _close(gx, x.grad + old, "tanh bwd accumulate")
    _close(HR.tanh_bwd(y.detach(), gy)[0], x.grad, "tanh bwd")
