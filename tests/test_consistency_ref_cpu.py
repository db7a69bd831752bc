"""The float64 restatements of tests/consistency_ref.py, checked without a GPU:
* every backward restatement against torch float64 autograd of the forward restatement (1e-10 relative,
  inputs with no stored zeros, unrounded float64 P for the pair / KL-JSD backwards);
* the conditions the GPU tests' inputs are chosen for (share of mask decisions excluded near the
  threshold, no f32 underflow in the "separated" KL-JSD inputs, one-sided f16 zeros in the "underflow"
  inputs);
* a float32 emulation of the KL-JSD forward term: the form log1p(e^2 / (4 (1 + e))), e = expm1(x), is inf
  on the "separated" inputs (expm1f(x) == -1 for x <~ -17.33, e*e overflows for x >~ 44.3); the ranged form
  (that one for |x| <= 1, |x| + 2 log1p(exp(-|x|)) - 2 ln 2 beyond) is within 1e-6 of float64.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import consistency_ref as R


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_emask_bwd_matches_autograd():
    g = _gen(1)
    N, HW, C = 3, 35, 24
    y1 = torch.randn(N, HW, C, generator=g, dtype=torch.float64).requires_grad_(True)
    y2 = (y1.detach() + 0.4 * torch.randn(N, HW, C, generator=g, dtype=torch.float64)).requires_grad_(True)
    mu1, mu2 = y1.detach().mean(1), y2.detach().mean(1)
    is1, is2 = 1 / y1.detach().std(1), 1 / y2.detach().std(1)
    drop1 = (torch.rand(N, C, generator=g) > 0.3).double() / 0.7
    drop2 = (torch.rand(N, C, generator=g) > 0.3).double() / 0.7
    m1, m2, e = R.emask_fwd(y1, y2, mu1, is1, mu2, is2, 0.4, drop1, drop2)
    assert 0.2 < e.double().mean().item() < 0.8
    gm1, gm2 = torch.randn(N, HW, C, generator=g).double(), torch.randn(N, HW, C, generator=g).double()
    ((m1 * gm1).sum() + (m2 * gm2).sum()).backward()
    r1, r2 = R.emask_bwd(gm1, gm2, e, drop1, drop2)
    assert _rel(r1, y1.grad) < 1e-10 and _rel(r2, y2.grad) < 1e-10


def test_softmax_bwd_matches_autograd():
    g = _gen(2)
    L = (2 * torch.randn(7, 512, generator=g)).double().requires_grad_(True)
    G = torch.randn(7, 512, generator=g).double()
    P = R.softmax_fwd(L)
    (P * G).sum().backward()
    assert _rel(R.softmax_bwd(P.detach(), G), L.grad) < 1e-10


@pytest.mark.parametrize("use", ["both", "g1", "g2", "nocoef"])
def test_pair_bwd_matches_autograd(use):
    g = _gen(3)
    M, C, coef = 7, 512, 50.0 * 7 * 512
    L1 = (2 * torch.randn(M, C, generator=g)).double().requires_grad_(True)
    L2 = (L1.detach() + 0.3 * torch.randn(M, C, generator=g).double()).requires_grad_(True)
    G1 = torch.randn(M, C, generator=g).double() if use != "g2" else None
    G2 = torch.randn(M, C, generator=g).double() if use != "g1" else None
    cf = None if use == "nocoef" else coef
    P1, P2 = R.softmax_fwd(L1), R.softmax_fwd(L2)
    tot = (cf or 0.0) * R.pair_loss(P1, P2)
    tot = tot + (0 if G1 is None else (P1 * G1).sum()) + (0 if G2 is None else (P2 * G2).sum())
    tot.backward()
    assert abs(R.pair_loss(P1, P2).item() - F.mse_loss(P1, P2).item()) <= 1e-12 * F.mse_loss(P1, P2).item()
    r1, r2 = R.pair_bwd(P1.detach(), P2.detach(), G1, G2, cf)
    assert _rel(r1, L1.grad) < 1e-10 and _rel(r2, L2.grad) < 1e-10


def _kl_reference(L1, L2, HW):
    """models2.py:339-346 as the model writes it: logits [B, C, HW], slot dim 1."""
    M, C = L1.shape
    a = L1.view(M // HW, HW, C).permute(0, 2, 1)
    b = L2.view(M // HW, HW, C).permute(0, 2, 1)
    pm = (F.softmax(a, 1) + F.softmax(b, 1)) / 2
    return 0.5 / HW * (F.kl_div(F.log_softmax(a, 1), pm, reduction="batchmean")
                       + F.kl_div(F.log_softmax(b, 1), pm, reduction="batchmean"))


@pytest.mark.parametrize("use", ["both", "g1", "g2", "nocoef"])
def test_jsd_bwd_matches_autograd(use):
    g = _gen(4)
    M, C, coef = 14, 512, 3.0 * 14
    L1 = (2 * torch.randn(M, C, generator=g)).double().requires_grad_(True)
    L2 = (L1.detach() + 0.3 * torch.randn(M, C, generator=g).double()).requires_grad_(True)
    G1 = torch.randn(M, C, generator=g).double() if use != "g2" else None
    G2 = torch.randn(M, C, generator=g).double() if use != "g1" else None
    cf = None if use == "nocoef" else coef
    loss = R.jsd_loss(L1, L2)
    ref = _kl_reference(L1, L2, 7)
    assert abs(loss.item() - ref.item()) <= 1e-12 * ref.item()
    P1, P2 = R.softmax_fwd(L1), R.softmax_fwd(L2)
    tot = (cf or 0.0) * ref
    tot = tot + (0 if G1 is None else (P1 * G1).sum()) + (0 if G2 is None else (P2 * G2).sum())
    tot.backward()
    r1, r2 = R.jsd_bwd(P1.detach(), P2.detach(), G1, G2, cf)
    assert _rel(r1, L1.grad) < 1e-10 and _rel(r2, L2.grad) < 1e-10


@pytest.mark.parametrize("nv,loss,act,bias", [(1, 0, 1, True), (2, 0, 0, False), (2, 1, 2, True), (2, 2, 1, True)])
def test_head_bwd_matches_autograd(nv, loss, act, bias):
    """d = act(w . (mem P) + b) with the readout materialised, against the v = mem^T w restatement."""
    g = _gen(5 + loss)
    M, C, k, coef = 14, 512, 24, 40.0
    Ls = [(2 * torch.randn(M, C, generator=g)).double().requires_grad_(True)]
    if nv == 2:
        Ls.append((Ls[0].detach() + 0.3 * torch.randn(M, C, generator=g).double()).requires_grad_(True))
    mem = torch.randn(k, C, generator=g).double().requires_grad_(True)
    w = (0.05 * torch.randn(k, generator=g)).double().requires_grad_(True)
    b = torch.tensor([0.02], dtype=torch.float64, requires_grad=True)
    gy = [torch.randn(M, generator=g).double() for _ in range(nv)]
    Ps = [R.softmax_fwd(L) for L in Ls]
    ds = [R.act_fwd((mem @ P.t()).t() @ w + (b if bias else 0.0), act) for P in Ps]
    tot = sum((d * q).sum() for d, q in zip(ds, gy))
    if loss == 1:
        tot = tot + coef * F.mse_loss(Ps[0], Ps[1])
    if loss == 2:
        tot = tot + coef * _kl_reference(Ls[0], Ls[1], 7)
    tot.backward()
    v = R.head_vec(mem.detach(), w.detach())
    yh = [R.head_fwd(P.detach(), v, b.item() if bias else None, act) for P in Ps]
    for a, d in zip(yh, ds):
        assert _rel(a, d.detach()) < 1e-12
    if act == 1:
        assert 0.2 < (yh[0] > 0).double().mean().item() < 0.8
    gL, u, gb = R.head_bwd([P.detach() for P in Ps], v, act, yh, gy, loss, coef if loss else None)
    for r, L in zip(gL, Ls):
        assert _rel(r, L.grad) < 1e-10
    dmem, gw = R.head_grads(mem.detach(), w.detach(), u)
    assert _rel(dmem, mem.grad) < 1e-10 and _rel(gw, w.grad) < 1e-10
    if bias:
        assert abs(gb.item() - b.grad.item()) <= 1e-10 * abs(b.grad.item())


def test_cls_combine_matches_interpolate():
    g = _gen(8)
    c1, c2 = torch.rand(2, 3, 5, generator=g), torch.rand(2, 3, 5, generator=g)
    cgt = (torch.rand(2, 3, 5, generator=g) > 0.5).float()
    up = lambda t: F.interpolate(t[:, None], scale_factor=4, mode="nearest")[:, 0]
    b1, b2 = (c1 >= 0.5).float(), (c2 >= 0.5).float()
    res, err = R.cls_combine(c1, c2, cgt, 4, 0.5)
    assert torch.equal(err, (up(b1) - up(b2)).abs())
    assert torch.equal(res, (up(cgt) + (up(b1) - up(b2)).abs()).clamp(0, 1))
    assert torch.equal(R.cls_combine(c1, None, None, 4, 0.5)[0], up(b1))
    assert torch.equal(R.cls_combine(c1, None, cgt, 4, 0.5)[0], up(cgt))


def test_cat_combine_is_conv_of_concatenation():
    """conv1x1(cat[y1, up2(y2), up4(y3)]) = z1 + up2(z2) + up4(z3) + bias, zk = conv1x1(yk; W slice k)."""
    g = _gen(9)
    N, H, W, C = 2, 8, 12, 6
    ys = [torch.randn(N, 5, H // s, W // s, generator=g).double() for s in (1, 2, 4)]
    wt = torch.randn(C, 15, 1, 1, generator=g).double()
    bias = torch.randn(C, generator=g).double()
    up = lambda t, s: t if s == 1 else F.interpolate(t, scale_factor=s, mode="bilinear", align_corners=False)
    want = F.conv2d(torch.cat([up(y, s) for y, s in zip(ys, (1, 2, 4))], 1), wt, bias)
    zs = [F.conv2d(y, wt[:, 5 * i:5 * i + 5]).permute(0, 2, 3, 1) for i, y in enumerate(ys)]
    assert _rel(R.cat_combine(zs[0], zs[1], zs[2], bias), want.permute(0, 2, 3, 1)) < 1e-12


def test_bce_matches_aten():
    g = _gen(10)
    p = torch.rand(257, generator=g)
    t = torch.rand(257, generator=g)
    p[:6] = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    t[:6] = torch.tensor([0.0, 1.0, 0.3, 0.0, 1.0, 0.3])
    pd = p.double().requires_grad_(True)
    want = F.binary_cross_entropy(pd, t.double())
    (2.5 * want).backward()
    loss, grad = R.bce(p, t, 2.5)
    assert abs(loss.item() - want.item()) <= 1e-12 * want.item()
    assert _rel(grad, pd.grad) < 1e-10
    assert torch.isfinite(grad).all()


# ------------------------------------------------------------------ conditions of the GPU inputs --
def test_emask_threshold_band_is_thin():
    """The GPU test excludes mask decisions with | |ia - ib| - thr | <= 1e-5 thr (the compiler may
    contract the subtraction): for its inputs that is <= 0.1 % of the elements, and both decisions are
    common."""
    for C, dt, seed in R.EMASK_CASES:
        y1, y2, mu1, is1, mu2, is2, _, _, thr = R.emask_inputs(3, 35, C, dt, seed)
        dist = R.emask_dist(y1, y2, mu1, is1, mu2, is2)
        assert ((dist - thr).abs() <= 1e-5 * thr).double().mean().item() <= 1e-3
        assert 0.4 < (dist < thr).double().mean().item() < 0.6


def test_separated_inputs_have_no_f32_underflow():
    l1, l2 = R.jsd_inputs("separated", 37, 512, 31)
    p1, p2 = R.softmax_fwd(l1), R.softmax_fwd(l2)
    assert min(p1.min().item(), p2.min().item()) >= 1e-30
    x = F.log_softmax(l1.double(), -1) - F.log_softmax(l2.double(), -1)
    assert x.min().item() < -40 and x.max().item() > 40  # both views are the low one on some rows
    for dt in (torch.bfloat16, torch.float16):  # the 16-bit forwards act on the rounded logits
        q1, q2 = R.softmax_fwd(l1.to(dt)), R.softmax_fwd(l2.to(dt))
        assert min(q1.min().item(), q2.min().item()) >= 1e-30


def test_underflow_inputs_have_one_sided_f16_zeros():
    l1, l2 = R.jsd_inputs("underflow", 192, 1024, 32)
    h = torch.float16
    p1, p2 = R.softmax_fwd(l1.to(h)).to(h), R.softmax_fwd(l2.to(h)).to(h)
    one_sided = (p1 == 0) != (p2 == 0)
    assert one_sided.sum().item() >= 1
    g1, g2 = R.jsd_bwd(p1, p2, None, None, 3.0 * 192, R.TINY[h])
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()


def test_jsd_forward_term_range_f32_emulation():
    l1, l2 = R.jsd_inputs("separated", 37, 512, 31)
    la, lb = F.log_softmax(l1.double(), -1), F.log_softmax(l2.double(), -1)
    pm = 0.5 * (la.exp() + lb.exp())
    want = R.jsd_loss(l1, l2)
    assert abs((pm * R.jsd_term_f64(la - lb)).sum().item() / 74 - want.item()) <= 1e-12 * want.item()
    x32 = (la - lb).float()
    old = (pm.float() * R.jsd_term_f32_old(x32)).sum(-1)
    assert torch.isinf(old[0::2]).all() and torch.isinf(old[1::2]).all()  # x < -17.33 rows and x > 44.3 rows
    new = (pm.float() * R.jsd_term_f32_new(x32)).double().sum() / 74
    assert abs(new.item() - want.item()) <= 1e-6 * want.item()
    # the accuracy loss of the old form sets in before it overflows
    t = torch.tensor([-16.0])
    assert abs(R.jsd_term_f32_old(t).item() - R.jsd_term_f64(t).item()) > 0.03
    assert abs(R.jsd_term_f32_new(t).item() - R.jsd_term_f64(t).item()) < 1e-5
    # and on ordinary inputs the two forms agree (|x| stays small; only the last bits may move)
    o1, o2 = R.jsd_inputs("ordinary", 37, 512, 33)
    xo = (F.log_softmax(o1.double(), -1) - F.log_softmax(o2.double(), -1)).float()
    assert xo.abs().max().item() < 2.5
    assert _rel(R.jsd_term_f32_new(xo).double(), R.jsd_term_f64(xo)) < 1e-6
    assert math.isfinite(new.item())
