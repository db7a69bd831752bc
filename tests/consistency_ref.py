"""float64 restatements of the kernels between the decoder and the loss (memread.hip, resample.hip
dg_cat_combine, head_loss.hip dg_bce_loss), written from the formulas in the kernel headers and the
model code they cite.  Plain torch, no project imports: tests/test_consistency_ref_cpu.py checks the
backward functions against float64 autograd of the forward ones, tests/test_consistency_kernels_gpu.py
checks the kernels against these.

Rows are pixel rows [M, C] with the slot (channel) dimension last.  The backward functions take the
stored probabilities P as input, as the kernels do.  In the backward functions only, the logarithm of
a stored zero is read as log(TINY[T]), T the storage type: half its smallest positive subnormal.
"""
import math

import torch
import torch.nn.functional as F

TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134, torch.float32: 2.0 ** -150}


def _d(t):
    return None if t is None else t.double()


# ---------------------------------------------------------------- e-mask -----
def emask_dist(y1, y2, mu1, is1, mu2, is2):
    """|IN(y1) - IN(y2)| of y [N, HW, C] with per-(instance, channel) statistics [N, C]."""
    ia = (_d(y1) - _d(mu1)[:, None, :]) * _d(is1)[:, None, :]
    ib = (_d(y2) - _d(mu2)[:, None, :]) * _d(is2)[:, None, :]
    return (ia - ib).abs()


def emask_fwd(y1, y2, mu1, is1, mu2, is2, thr, drop1=None, drop2=None):
    """e = dist < thr; m_v = y_v * e * drop_v (models/models.py:147-184).  Returns (m1, m2, e)."""
    e = emask_dist(y1, y2, mu1, is1, mu2, is2) < thr
    d1 = 1.0 if drop1 is None else _d(drop1)[:, None, :]
    d2 = 1.0 if drop2 is None else _d(drop2)[:, None, :]
    return _d(y1) * e * d1, _d(y2) * e * d2, e


def emask_bwd(gm1, gm2, e, drop1=None, drop2=None):
    """g_y_v = g_m_v * e * drop_v (e is a constant of the backward)."""
    d1 = 1.0 if drop1 is None else _d(drop1)[:, None, :]
    d2 = 1.0 if drop2 is None else _d(drop2)[:, None, :]
    return _d(gm1) * e * d1, _d(gm2) * e * d2


# ---------------------------------------------------------------- softmax ----
def softmax_fwd(L):
    return F.softmax(_d(L), -1)


def softmax_bwd(P, G):
    """gL = P (G - <P, G>)."""
    P, G = _d(P), _d(G)
    return P * (G - (P * G).sum(-1, keepdim=True))


def pair_loss(P1, P2):
    """loss_con = mean((P1 - P2)^2) (models/models.py:286-296) of the stored probabilities."""
    return ((_d(P1) - _d(P2)) ** 2).mean()


def pair_bwd(P1, P2, G1, G2, coef):
    """gL_v = P_v (g_v' - <P_v, g_v'>), g_1' = G1 + k (P1 - P2), g_2' = G2 - k (P1 - P2),
    k = 2 coef / (M C); G_v None = 0, coef None = 0."""
    P1, P2 = _d(P1), _d(P2)
    M, C = P1.shape
    k = 0.0 if coef is None else 2.0 * float(coef) / (M * C)
    g1 = (0.0 if G1 is None else _d(G1)) + k * (P1 - P2)
    g2 = (0.0 if G2 is None else _d(G2)) - k * (P1 - P2)
    return softmax_bwd(P1, g1), softmax_bwd(P2, g2)


# ---------------------------------------------------------------- KL-JSD -----
def jsd_loss(L1, L2):
    """loss_kl of models2.DensityRegressorM.forward_train (models/models2.py:339-346) from the logits:
    0.5/HW (kl_div(log p1, pm, batchmean) + kl_div(log p2, pm, batchmean)), pm = (p1 + p2)/2
    = sum pm (2 log pm - log p1 - log p2) / (2 M)."""
    la, lb = F.log_softmax(_d(L1), -1), F.log_softmax(_d(L2), -1)
    pm = 0.5 * (la.exp() + lb.exp())
    return (2.0 * torch.xlogy(pm, pm) - pm * (la + lb)).sum() / (2.0 * L1.shape[0])


def _log_stored(P, tiny):
    return torch.log(P.clamp_min(tiny))


def jsd_loss_terms_bwd(P1, P2, k, tiny):
    """k (p_v (A - <p_v, A> + 1) - pm), A = log pm - (log p1 + log p2)/2: the logit gradient of
    k * sum pm (2 log pm - log p1 - log p2) through both softmaxes (sum_j p_j = 1)."""
    pm = 0.5 * (P1 + P2)
    A = torch.where(pm > 0, _log_stored(pm, tiny) - 0.5 * (_log_stored(P1, tiny) + _log_stored(P2, tiny)),
                    torch.zeros_like(pm))
    t1 = (P1 * A).sum(-1, keepdim=True)
    t2 = (P2 * A).sum(-1, keepdim=True)
    return k * (P1 * (A - t1 + 1.0) - pm), k * (P2 * (A - t2 + 1.0) - pm)


def jsd_bwd(P1, P2, G1, G2, coef, tiny=TINY[torch.float32]):
    """Readout softmax backward of G_v (None = 0) plus coef * d loss_kl / d logits (coef None = 0)."""
    P1, P2 = _d(P1), _d(P2)
    M = P1.shape[0]
    k = 0.0 if coef is None else float(coef) / (2.0 * M)
    a1, a2 = jsd_loss_terms_bwd(P1, P2, k, tiny)
    g1 = softmax_bwd(P1, torch.zeros_like(P1) if G1 is None else G1) + a1
    g2 = softmax_bwd(P2, torch.zeros_like(P2) if G2 is None else G2) + a2
    return g1, g2


# ---------------------------------------------------------------- fused head -
def act_fwd(s, act):
    return F.relu(s) if act == 1 else torch.sigmoid(s) if act == 2 else s


def act_gpre(gy, y, act):
    """act'(pre) gy from the saved output y."""
    if act == 1:
        return torch.where(y > 0, gy, torch.zeros_like(gy))
    if act == 2:
        return gy * y * (1.0 - y)
    return gy


def head_vec(mem, w):
    """v = mem^T w: den_head's 1x1 weights pulled through the readout y_new = mem P."""
    return _d(w) @ _d(mem)


def head_fwd(P, v, bias, act):
    """d = act(w . (mem P) + b) = act(v . P + b) on the stored probabilities."""
    return act_fwd(_d(P) @ _d(v) + (0.0 if bias is None else float(bias)), act)


def head_bwd(Ps, v, act, yhs, gyhs, loss, coef, tiny=TINY[torch.float32]):
    """Backward of the fused head for the views in Ps (1 or 2).  Returns (gLs, u, gb):
    gL_v = P_v (gP_v - <P_v, gP_v>) + loss term, gP_v = gpre_v v (+- k (P1 - P2) for loss 1),
    u = sum_px sum_v gpre_v P_v, gb = sum gpre.  gyh None = 0; coef None = no loss term."""
    Ps = [_d(P) for P in Ps]
    v = _d(v)
    M, C = Ps[0].shape
    q = [torch.zeros(M, dtype=torch.float64) if g is None else act_gpre(_d(g), _d(y), act)
         for g, y in zip(gyhs, yhs)]
    gP = [qi[:, None] * v[None, :] for qi in q]
    if loss == 1 and coef is not None:
        k = 2.0 * float(coef) / (M * C)
        gP[0] = gP[0] + k * (Ps[0] - Ps[1])
        gP[1] = gP[1] - k * (Ps[0] - Ps[1])
    gL = [softmax_bwd(P, g) for P, g in zip(Ps, gP)]
    if loss == 2 and coef is not None:
        a1, a2 = jsd_loss_terms_bwd(Ps[0], Ps[1], float(coef) / (2.0 * M), tiny)
        gL = [gL[0] + a1, gL[1] + a2]
    u = sum(qi @ P for qi, P in zip(q, Ps))
    return gL, u, sum(qi.sum() for qi in q)


def head_grads(mem, w, u):
    """dmem_readout = w u^T, gw = mem u."""
    return torch.outer(_d(w), u), _d(mem) @ u


# ---------------------------------------------------------------- class maps -
def cls_combine(c1, c2, cgt, s, thr):
    """models/models.py:196-207, 323-327: nearest x s of the thresholded maps [N, h, w].
    Two views: (clamp(up(cgt) + |up(c1 >= thr) - up(c2 >= thr)|, 0, 1), the |.| term);
    one view (c2 None): (cgt given ? up(cgt) : up(c1 >= thr), None)."""
    up = lambda t: t.repeat_interleave(s, 1).repeat_interleave(s, 2)
    b1 = (c1 >= thr).to(c1.dtype)
    if c2 is None:
        return up(cgt if cgt is not None else b1), None
    e = (b1 - (c2 >= thr).to(c1.dtype)).abs()
    g = cgt if cgt is not None else torch.zeros_like(e)
    return up((g + e).clamp(0, 1)), up(e)


# ---------------------------------------------------------------- cat-combine
def cat_combine(z1, z2, z3, bias):
    """z1 + up2(z2) + up4(z3) + bias on NHWC float64 maps (models/models.py:84, 89-90)."""
    nchw = lambda t: _d(t).permute(0, 3, 1, 2)
    up = lambda t, s: F.interpolate(nchw(t), scale_factor=s, mode="bilinear", align_corners=False)
    z = nchw(z1) + up(z2, 2) + up(z3, 4)
    if bias is not None:
        z = z + _d(bias)[None, :, None, None]
    return z.permute(0, 2, 3, 1)


# ---------------------------------------------------------------- BCE --------
def bce(pred, target, grad_coef=1.0):
    """F.binary_cross_entropy mean and grad_coef * its gradient, with ATen's clamps: log >= -100,
    denominator (1 - p) p >= 1e-12 (ATen's constant is a float: the float32 nearest 1e-12)."""
    p, t = _d(pred), _d(target)
    lp = torch.log(p).clamp_min(-100.0)
    l1p = torch.log(1.0 - p).clamp_min(-100.0)
    loss = -(t * lp + (1.0 - t) * l1p).mean()
    grad = grad_coef * (p - t) / ((1.0 - p) * p).clamp_min(torch.tensor(1e-12, dtype=torch.float32).item()) / p.numel()
    return loss, grad


# ---------------------------------------------------------------- inputs -----
def jsd_inputs(kind, M, C, seed):
    """The KL-JSD logit pairs of the tests (float32 CPU tensors [M, C]).
    ordinary:  2 randn; view 2 = view 1 + 0.3 randn.
    separated: ordinary, then on four random slots per row -48, -30, -20 and -12 are added to view 2's
               logit on even rows and to view 1's on odd rows.
    underflow: 2.5 randn; view 2 = view 1 + 0.3 randn (f16 storage rounds p < 3e-8 to 0)."""
    g = torch.Generator().manual_seed(seed)
    scale = 2.5 if kind == "underflow" else 2.0
    l1 = torch.randn(M, C, generator=g) * scale
    l2 = l1 + 0.3 * torch.randn(M, C, generator=g)
    if kind == "separated":
        drops = torch.tensor([-48.0, -30.0, -20.0, -12.0])
        for r in range(M):
            slots = torch.randperm(C, generator=g)[:4]
            (l2 if r % 2 == 0 else l1)[r, slots] += drops
    return l1, l2


# (C, storage type, seed) of the e-mask layouts at N = 3, HW = 35
EMASK_CASES = [(512, torch.float32, 21), (512, torch.bfloat16, 22), (24, torch.float32, 23),
               (24, torch.bfloat16, 24), (8, torch.float16, 25)]


def emask_inputs(N, HW, C, dtype, seed, p_drop=0.3):
    """Inputs of the e-mask tests: y_v [N, HW, C] of the storage type, f32 statistics [N, C] made on the
    host (mean, 1/std of the stored values), drop vectors of zeros and 1/(1 - p), and thr (a float32
    value) midway between the two middle order statistics of |IN(y1) - IN(y2)|: near the median, so that
    both decisions are common, and not on an element."""
    g = torch.Generator().manual_seed(seed)
    y1 = torch.randn(N, HW, C, generator=g).to(dtype)
    y2 = (y1.float() + 0.4 * torch.randn(N, HW, C, generator=g)).to(dtype)
    mu1, mu2 = y1.float().mean(1), y2.float().mean(1)
    is1, is2 = 1.0 / y1.float().std(1), 1.0 / y2.float().std(1)
    drop1 = (torch.rand(N, C, generator=g) >= p_drop).float() / (1.0 - p_drop)
    drop2 = (torch.rand(N, C, generator=g) >= p_drop).float() / (1.0 - p_drop)
    srt = emask_dist(y1, y2, mu1, is1, mu2, is2).flatten().sort().values
    mid = 0.5 * (srt[srt.numel() // 2 - 1].item() + srt[srt.numel() // 2].item())
    thr = torch.tensor(mid, dtype=torch.float32).item()
    return y1, y2, mu1, is1, mu2, is2, drop1, drop2, thr


def jsd_term_f32_old(x):
    """float32 emulation of the forward term before the range fix: log1p(e^2 / (4 (1 + e))),
    e = expm1(x), x = log p1 - log p2."""
    e = torch.expm1(x.float())
    return torch.log1p(e * e / (4.0 * (1.0 + e)))


def jsd_term_f32_new(x):
    """float32 emulation of the forward term: the form above for |x| <= 1 (no cancellation), else the
    symmetric |x| + 2 log1p(exp(-|x|)) - 2 ln 2 (finite for every finite x)."""
    x = x.float()
    ax = x.abs()
    far = ax + 2.0 * torch.log1p(torch.exp(-ax)) - torch.tensor(2.0 * math.log(2.0), dtype=torch.float32)
    return torch.where(ax > 1.0, far, jsd_term_f32_old(x))


def jsd_term_f64(x):
    """2 log pm - log p1 - log p2 as a function of x = log p1 - log p2."""
    x = x.double()
    return 2.0 * torch.logaddexp(x, torch.zeros_like(x)) - x - 2.0 * math.log(2.0)
