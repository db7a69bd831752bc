"""float64 restatements of the density head, the MSE loss, the AdamW step and tanh of head_loss.hip, written from
include/dgvcc.h and the kernels' comments.  Plain torch on the CPU: tests/test_head_ref_cpu.py checks them
against float64 autograd and torch.optim.AdamW, tests/test_head_kernels_gpu.py checks the kernels against them.
Every function takes the stored inputs and computes in float64; each also returns the sums of absolute terms
that the bounds need.
"""
import math

import torch


def _d(t):
    return None if t is None else t.detach().double().cpu()


# ---------------------------------------------------------------- head ---------
def head_fwd(x, w, bias, act):
    """y[p] = act(sum_c x[p, c] w[c] + bias), act 0 none, 1 ReLU, 2 sigmoid; x [M, C].  Returns (y, pre-activation
    s, sum |x w| + |bias| per pixel)."""
    x, w = _d(x), _d(w)
    s = x @ w
    a = x.abs() @ w.abs()
    if bias is not None:
        s = s + _d(bias)[0]
        a = a + _d(bias)[0].abs()
    y = s.clamp_min(0.0) if act == 1 else torch.sigmoid(s) if act == 2 else s
    return y, s, a


def head_gpre(gy, y, act):
    """Gradient of the pre-activation from the *stored* y: ReLU gy [y > 0], sigmoid gy y (1 - y)."""
    gy, y = _d(gy), _d(y)
    if act == 1:
        return torch.where(y > 0, gy, torch.zeros_like(gy))
    if act == 2:
        return gy * y * (1.0 - y)
    return gy


def head_bwd(x, w, act, y, gy, gx_old=None):
    """gx[p, c] = g'[p] w[c] (+ gx_old), gw[c] = sum_p g'[p] x[p, c], gbias = sum_p g'[p]; with the absolute
    terms of each."""
    x, w = _d(x), _d(w)
    g = head_gpre(gy, y, act)
    gw_terms = g.abs() @ x.abs()
    gx = g[:, None] * w[None, :]
    old = torch.zeros_like(gx) if gx_old is None else _d(gx_old)
    return dict(g=g, gx=gx + old, gx_prod=gx.abs(), gx_old=old.abs(), gw=g @ x, gw_terms=gw_terms,
                gbias=g.sum(), gbias_terms=g.abs().sum())


# ---------------------------------------------------------------- MSE ----------
def mse(pred, gt, gt_scale, grad_coef=1.0):
    """loss = mean (pred - gt gt_scale)^2, dpred = 2 grad_coef (pred - gt gt_scale) / n."""
    pred, gt = _d(pred).reshape(-1), _d(gt).reshape(-1)
    n = pred.numel()
    d = pred - gt * gt_scale
    return dict(loss=(d * d).sum() / n, dpred=2.0 * grad_coef * d / n, d=d, tgt=(gt * gt_scale).abs(), n=n)


# ---------------------------------------------------------------- AdamW --------
def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """One step of torch.optim.AdamW's single-tensor formula: p *= 1 - lr wd; m.lerp_(g, 1 - beta1);
    v = beta2 v + (1 - beta2) g^2; denom = sqrt(v) / sqrt(1 - beta2^step) + eps; p -= lr / (1 - beta1^step) m /
    denom.  Returns the new (p, m, v) and the intermediate terms."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    pd = p * (1.0 - lr * wd)
    m1 = m + (1.0 - beta1) * (g - m)
    v1 = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    step_size = lr / bc1
    upd = step_size * m1 / denom
    return dict(p=pd - upd, m=m1, v=v1, decayed=pd, upd=upd, denom=denom, step_size=step_size,
                m_terms=m.abs() + (1.0 - beta1) * (g.abs() + m.abs()), v_terms=beta2 * v.abs() + (1.0 - beta2) * g * g)


# ---------------------------------------------------------------- tanh ---------
def tanh_fwd(x):
    return torch.tanh(_d(x))


def tanh_bwd(y, gy, gx_old=None):
    """gx = gy (1 - y^2) (+ gx_old) from the stored y; also |gy| y^2, the product rounded before the
    subtraction."""
    y, gy = _d(y), _d(gy)
    g = gy * (1.0 - y * y)
    return (g if gx_old is None else g + _d(gx_old)), g, gy.abs() * y * y
