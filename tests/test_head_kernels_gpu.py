"""Kernel-level tests of the density head (dg_head_fwd / dg_head_bwd), the MSE loss, the AdamW step and tanh of
head_loss.hip against the float64 restatements of tests/head_ref.py (checked against torch autograd and
torch.optim.AdamW in tests/test_head_ref_cpu.py): per element and per channel, never against a whole-tensor
maximum.  The references take the stored inputs (and, for the backwards, the kernel's stored y).

Bounds (derived; e = 2^-24, S = 512 e, u_T the storage type's ulp as in tests/test_bn_kernels_gpu.py).
  head y: (L + 8) e sum|x w| + 4 e |ref|, L = ceil(C / (TPP V)) V the FMAs of one lane (TPP = 32, 16 or 8 lanes
    per pixel, V = 4 or 8 channels per load), 8 for the shuffle tree of at most 5 steps and the bias.  Sigmoid:
    the dot product's bound / 4 (the largest slope) + 4 SIGMOID_ULPS 2^-23 |ref|.  No accuracy table of expf is
    installed with the toolchain, so 1 / (1 + expf(-s)) was measured through the kernel itself on exact
    pre-activations (one-hot x, w = 1): worst relative error SIGMOID_ULPS = 0.980 x 2^-23 over 4001 points of [-30, 30];
    four times that is allowed, the sample being small.
  head gx: per element, ReLU / none: 2 e (|g' w| + |old|) (g' exact); sigmoid: 5 e |g' w| + 2 e |old| (g' = gy y
    (1 - y) takes three roundings of its own, which the count of 2 leaves out).  16-bit: + u_T |ref| once.
  head gw, gbias: per channel S sum|g' x| + e |ref|.  Longest f32 chain: ceil(ppb / rows) + rows (ppb <= 65 pixels
    per block at these M; rows = 256 / (C / V) <= 128) and, for gbias, 256 thread sums: below 512.  Across
    blocks the sum is double.
  MSE loss: ((L + 12) e sum d^2 + 2 e sum |d| |gt gt_scale|) / n + e |ref|: L = ceil(n / (nblk 256)) FMAs per
    thread, 6 tree steps, 4 wave sums, then double; d = pred - gt gt_scale carries the rounding of the product
    (gt_scale = 1: exact, the term drops) and of the difference.  dpred: 3 e |ref| (k = 2 coef / n, the
    difference, the product) + e |k| |gt gt_scale| when gt_scale != 1.
  AdamW: m: 2 e (|m| + (1 - b1)(|g| + |m|)) (difference, FMA).  v: 4 e (b2 |v| + (1 - b2) g^2) + 2^-126 (two
    products, FMA; results below the smallest normal may be flushed).  p: 4 e |p (1 - lr wd)| + step_size / denom
    B(m) + 10 e |update| + e |ref|: the decay factor and product; the update step_size m / denom with denom =
    sqrt(v) / sqrt(bc2) + eps good to 7 e (v's 4 e halved by the root, root, quotient, bc2's root, sum), the
    quotient, step_size and the product; the final difference.  Where g = 0 and m = v = 0 the result is p (1 - lr
    wd) in f32 exactly and m, v stay 0.
  tanh forward: 4 TANHF_ULPS 2^-23 |ref|.  No accuracy table of tanhf is installed with the toolchain: the worst
    error of dg_tanh_fwd against float64 over this module's inputs (262149 points: N(0, 2) and 0, +-1e-8, +-20,
    +-100) was measured at TANHF_ULPS = 1.179 x 2^-23 |ref|; four times that is allowed.
  tanh backward: 3 e |ref| + e |gy| y^2 (y y is rounded before it is taken from 1 unless the compiler fuses
    the two; exact where y = +-1 or 0), + e |old + ref| when accumulating.
"""
import math

import numpy as np
import pytest
import torch

import bn_ref as R
import head_ref as HR
from test_bn_kernels_gpu import (E, S, SENT, U, _end_run_on_device_fault, act_of, neighbours_intact,  # noqa: F401
                                 stored, sum_bound, within)

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
IDS = R.IDS
ULP = 2.0 ** -23
# measured on an MI355X (ROCm 7) through the kernels, see the module docstring
SIGMOID_ULPS = 0.980
TANHF_ULPS = 1.179


def _k():
    from dgvcc_amd import kernels as K
    return K


def ulps(out, ref):
    """Worst |out - ref| / (2^-23 |ref|) over the elements with ref != 0."""
    out, ref = out.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    nz = ref != 0
    return ((out - ref).abs()[nz] / (ULP * ref.abs()[nz])).max().item() if nz.any() else 0.0


# ------------------------------------------------------------------------------ head --------------
HEAD = [(F32, C) for C in (8, 64, 96, 256, 512, 1024)] + [(dt, C) for dt in (BF16, F16) for C in (8, 64, 96, 256, 2048)]


def lane_chain(dt, C):
    V = R.VEC[dt]
    tpp = 32 if C // V >= 32 else 16 if C // V >= 16 else 8
    return -(-C // (tpp * V)) * V


def head_inputs(dt, C, M, seed=0):
    g = torch.Generator().manual_seed(seed or 17 + C + M)
    x = torch.randn(1, M, 1, C, generator=g).to(dt)
    w = torch.randn(C, generator=g) / C ** 0.5
    return x, w, torch.randn(1, generator=g), torch.randn(M, generator=g)


def y_bound_head(dt, C, act, ref, a):
    dot = (lane_chain(dt, C) + 8) * E * a
    if act == 2:
        return dot / 4 + 4 * SIGMOID_ULPS * ULP * ref.abs()
    return dot + 4 * E * ref.abs()


def gx_bound(dt, act, r, accumulate):
    b = (5 if act == 2 else 2) * E * r["gx_prod"] + 2 * E * r["gx_old"]
    return stored(b, r["gx"], dt)


def run_head(dev, dt, C, M, act, sliced=False, use_gx=True, accumulate=False, use_gbias=True, fwd_only=False):
    K = _k()
    x, w, bias, gy = head_inputs(dt, C, M)
    bias = bias if act == 2 else None
    xA = act_of(x, dev, sliced)
    wd, bd = w.to(dev), None if bias is None else bias.to(dev)
    y = K.head_fwd(xA, wd, bd, act)
    torch.cuda.synchronize()
    x2 = x.reshape(M, C)
    yr, _, a = HR.head_fwd(x2, w, bias, act)
    what = f"{IDS[dt]} C {C} M {M} act {act}"
    within(y.reshape(-1), yr, y_bound_head(dt, C, act, yr, a), what + " y")
    if fwd_only:
        return
    old = None
    gxA = None
    if use_gx:
        if accumulate:
            old = torch.randn(1, M, 1, C, generator=torch.Generator().manual_seed(5)).to(dt)
            gxA = act_of(old, dev, sliced)
        else:
            gxA = act_of(x, dev, sliced, fill=SENT)
    gw = torch.full((C,), SENT, dtype=F32, device=dev)
    gb = torch.full((1,), SENT, dtype=F32, device=dev)
    K.head_bwd(xA, wd, act, y, gy.to(dev), gxA, gw, gb if use_gbias else None, accumulate)
    torch.cuda.synchronize()
    r = HR.head_bwd(x2, w, act, y.reshape(-1), gy, None if old is None else old.reshape(M, C))
    if use_gx:
        within(gxA.view().reshape(M, C), r["gx"], gx_bound(dt, act, r, accumulate), what + " gx")
        neighbours_intact(gxA, what + " gx")
    within(gw, r["gw"], sum_bound(r["gw_terms"], r["gw"]), what + " gw")
    if use_gbias:
        within(gb.reshape(()), r["gbias"], sum_bound(r["gbias_terms"], r["gbias"]), what + " gbias")
    else:
        assert gb.item() == SENT


@pytest.mark.parametrize("dt,C", HEAD, ids=lambda v: IDS.get(v, str(v)))
def test_head(dev, dt, C):
    """Forward and backward at every TPP instantiation, idle lanes (C / V < 8), C / V not dividing 256 (C = 96),
    one row per block (f32 C = 1024, 16-bit C = 2048), and M = 65537 (1024 blocks of 65 pixels) where C <= 256."""
    for M in (1, 63, 126, 65537):
        if M > 1000 and C > 256:
            continue
        for act in (0, 1, 2):
            run_head(dev, dt, C, M, act)


def test_head_fwd_grid_stride(dev):
    """M = 131080 at TPP = 32: the forward's blocks walk more than one group of pixels."""
    run_head(dev, BF16, 256, 131080, 1, fwd_only=True)


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: IDS[d])
@pytest.mark.parametrize("variant", ["slices", "nogx", "accumulate", "nogbias"])
def test_head_variants(dev, dt, variant):
    """C = 256, M = 126: x and gx as channel slices of wider sentinel buffers (ldx, ldgx > C), gx = NULL,
    accumulate_gx onto a non-zero gx, gbias = NULL."""
    for act in (1, 2):
        run_head(dev, dt, 256, 126, act, sliced=variant == "slices", use_gx=variant != "nogx",
                 accumulate=variant == "accumulate", use_gbias=variant != "nogbias")


def test_head_rejected_shapes(dev):
    """f32 C = 2048 (C / V > 256: the backward), f32 C = 6, bf16 C = 12, ld no multiple of the vector width:
    DGError and nothing written."""
    K = _k()
    p, s = K.ptr, K.stream()
    for dt, C, ld, fwd_too in ((F32, 2048, 2048, False), (F32, 6, 8, True), (BF16, 12, 16, True), (F32, 64, 66, True),
                               (BF16, 64, 68, True)):
        M = 8
        x = torch.zeros(M * ld, dtype=dt, device=dev)
        gx = torch.full_like(x, SENT)
        w = torch.ones(C, device=dev)
        y, gy = torch.full((M,), SENT, device=dev), torch.ones(M, device=dev)
        gw, gb = torch.full((C,), SENT, device=dev), torch.full((1,), SENT, device=dev)
        work = torch.full((1024 * (C + 1),), SENT, device=dev)
        code = K.dtype_code(dt)
        if fwd_too:
            with pytest.raises(K.DGError):
                K.call("dg_head_fwd", code, p(x), ld, M, C, p(w), None, 1, p(y), s)
        with pytest.raises(K.DGError):
            K.call("dg_head_bwd", code, p(x), ld, M, C, p(w), 0, p(gy), p(gy), p(gx), ld, 0, p(gw), p(gb), p(work), s)
        torch.cuda.synchronize()
        for t in ((y,) if fwd_too else ()) + (gx, gw, gb, work):
            assert torch.equal(t, torch.full_like(t, SENT)), (dt, C, ld, "output written")


def test_sigmoid_accuracy(dev):
    """1 / (1 + expf(-s)) on exact pre-activations (one-hot x, w = 1, no bias) over [-30, 30]: within four times
    the measured SIGMOID_ULPS; prints the figure measured now."""
    K = _k()
    sv = torch.linspace(-30, 30, 4001)
    x = torch.zeros(1, sv.numel(), 1, 8)
    x[0, :, 0, 0] = sv
    w = torch.zeros(8)
    w[0] = 1.0
    y = K.head_fwd(K.Act(x.to(dev)), w.to(dev), None, 2)
    torch.cuda.synchronize()
    ref = torch.sigmoid(sv.double())
    print(f"  sigmoid: worst error {ulps(y, ref):.3f} x 2^-23 |ref|")
    within(y.reshape(-1), ref, 4 * SIGMOID_ULPS * ULP * ref, "sigmoid")


# ------------------------------------------------------------------------------ MSE ---------------
@pytest.mark.parametrize("gt_scale,coef", [(1.0, 1.0), (1000.0, 1.0), (1.0, 0.37), (1000.0, 0.37)])
@pytest.mark.parametrize("n", [1, 255, 257, 262145, 4194307])
def test_mse(dev, n, gt_scale, coef):
    """dg_mse_loss: one thread, a partial block, two blocks, the 1024-block cap (chains of 2 and 17 per thread);
    with the gradient (per element) and with dpred = NULL (the same loss bits)."""
    K = _k()
    g = torch.Generator().manual_seed(n % 1000 + int(gt_scale))
    pred = torch.randn(n, generator=g)
    gt = torch.rand(n, generator=g) * 3.0 / gt_scale
    loss, dpred = K.mse_loss(pred.to(dev), gt.to(dev), gt_scale, True, coef)
    loss2, none = K.mse_loss(pred.to(dev), gt.to(dev), gt_scale, False, coef)
    torch.cuda.synchronize()
    assert none is None and torch.equal(loss, loss2), "loss with and without dpred"
    coef32 = float(np.float32(coef))
    r = HR.mse(pred, gt, gt_scale, coef32)
    nblk = max(1, min(1024, -(-n // 256)))
    L = -(-n // (nblk * 256))
    prod = 0.0 if gt_scale == 1.0 else 1.0
    d = r["d"]
    bl = ((L + 12) * E * (d * d).sum() + prod * 2 * E * (d.abs() * r["tgt"]).sum()) / n + E * r["loss"].abs()
    within(loss, r["loss"], bl, f"n {n} loss")
    k = 2.0 * coef32 / n
    within(dpred, r["dpred"], 3 * E * r["dpred"].abs() + prod * E * k * r["tgt"], f"n {n} dpred")


# ------------------------------------------------------------------------------ AdamW -------------
def f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize("step,wd", [(1, 0.0), (2, 1e-4), (1000, 1e-2)])
@pytest.mark.parametrize("n", [1, 257, 4194309])
def test_adamw(dev, n, step, wd):
    """dg_adamw_step per element (p, m and v): one element, two blocks, the grid-stride loop (n > 16384 x 256);
    gradients with exact zeros, |g| = 1e-20 and 1e18; step 1 from m = v = 0, later steps from random moments
    with m = v = 0 kept on every second zero-gradient element."""
    K = _k()
    g = torch.Generator().manual_seed(n % 1000 + step)
    lr, b1, b2, eps, wd = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.01
    gr[::7] = 0.0
    for i, v in ((1, 1e-20), (2, -1e-20), (3, 1e18), (4, -1e18)):
        if i < n:
            gr[i] = v
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4
        m[::14], v[::14] = 0.0, 0.0
    pd, md, vd = p.to(dev), m.to(dev), v.to(dev)
    K.adamw_step(pd, gr.to(dev), md, vd, lr, b1, b2, eps, wd, step)
    torch.cuda.synchronize()
    r = HR.adamw(p, gr, m, v, lr, b1, b2, eps, wd, step)
    what = f"n {n} step {step}"
    bm = 2 * E * r["m_terms"]
    within(md, r["m"], bm, what + " m")
    within(vd, r["v"], 4 * E * r["v_terms"] + 2.0 ** -126, what + " v")
    bp = 4 * E * r["decayed"].abs() + r["step_size"] / r["denom"] * bm + 10 * E * r["upd"].abs() + E * r["p"].abs()
    within(pd, r["p"], bp, what + " p")
    still = (gr == 0) & (m == 0) & (v == 0)
    assert still.any()
    c32 = torch.tensor(np.float32(1.0 - lr * wd))
    assert torch.equal(pd.cpu()[still], (p * c32)[still]), what + ": decay alone where g = m = v = 0"
    assert not md.cpu()[still].any() and not vd.cpu()[still].any()


# ------------------------------------------------------------------------------ tanh --------------
def tanh_inputs(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 2.0
    sp = torch.tensor([0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0])
    if n >= sp.numel():
        x[:sp.numel()] = sp
    return x, torch.randn(n, generator=g), torch.randn(n, generator=g)


@pytest.mark.parametrize("n", [1, 255, 257, 262149])
def test_tanh(dev, n):
    """dg_tanh_fwd against float64 within four times the measured accuracy of tanhf (printed again here);
    dg_tanh_bwd, with and without accumulate, as exact arithmetic on the stored y."""
    K = _k()
    x, gy, old = tanh_inputs(n)
    xd, gyd = x.to(dev), gy.to(dev)
    y = torch.full((n,), SENT, device=dev)
    K.call("dg_tanh_fwd", K.ptr(xd), n, K.ptr(y), K.stream())
    gx, gxa = torch.full((n,), SENT, device=dev), old.to(dev)
    K.call("dg_tanh_bwd", K.ptr(y), K.ptr(gyd), n, K.ptr(gx), 0, K.stream())
    K.call("dg_tanh_bwd", K.ptr(y), K.ptr(gyd), n, K.ptr(gxa), 1, K.stream())
    torch.cuda.synchronize()
    ref = HR.tanh_fwd(x)
    print(f"  tanhf n {n}: worst error {ulps(y, ref):.3f} x 2^-23 |ref|")
    within(y, ref, 4 * TANHF_ULPS * ULP * ref.abs(), f"n {n} tanh")
    acc, g0, sq = HR.tanh_bwd(y, gy, old)
    within(gx, g0, 3 * E * g0.abs() + E * sq, f"n {n} tanh bwd")
    within(gxa, acc, 3 * E * g0.abs() + E * sq + E * acc.abs(), f"n {n} tanh bwd accumulate")
    assert math.isfinite(gx.sum().item())
