"""SwitchWhiten2d sw_type 3 (BW + IW + LN) and 5 (BW + IW + BN + IN + LN), tied mixing weights and
affine=False on the GPU, against the float64 restatement tests/sw_ref.py (itself pinned to the
reference operator by tests/golden/sw_types.npz): the kernels through dgvcc_amd.kernels, the new
entry points at sw_type 2 against dg_sw_fwd / dg_sw_bwd bit for bit, the split phases in one
process, the module's standalone forward() under autograd, and one SW-counter train step.

Bounds are those of test_trunk_kernels_gpu.py::test_switch_whiten (relerr = max |a - b| / max |b|):
f32  y 1e-4, dx and every parameter gradient 1e-3, running statistics 1e-4;
16-bit  y 3e-2, dx and every parameter gradient 5e-2, running statistics 1e-2."""
import functools

import pytest
import torch

import sw_ref as R
from test_kernels_gpu import relerr, to_nchw, to_nhwc

pytestmark = pytest.mark.gpu

PARAMS = R.PARAMS
SHAPES = [
    (2, 16, 1, 3),   # one group, one pixel row: LN inside the group, HW below a 4-pixel MFMA step
    (3, 64, 9, 7),   # LN across four groups, ragged pixel tail
    (2, 256, 6, 5),  # sixteen groups (C at the kernels' limit)
    (1, 32, 4, 4),   # N = 1: BW = IW
]
# (sw_type, act, tie, affine): both types with both act values and each tie / affine combination
VARIANTS = [(3, 0, False, True), (3, 1, True, True), (3, 0, True, False), (3, 1, False, False),
            (5, 1, False, True), (5, 0, True, True), (5, 1, True, False), (5, 0, False, False)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _k():
    from dgvcc_amd import kernels as K
    return K


def _bounds(dtype):
    f32 = dtype == torch.float32
    return dict(y=1e-4 if f32 else 3e-2, dx=1e-3 if f32 else 5e-2, grad=1e-3 if f32 else 5e-2,
                run=1e-4 if f32 else 1e-2)


@functools.lru_cache(maxsize=None)
def _case(shape, sw_type, act, tie, affine, dtype):
    """Seeded inputs (rounded to dtype) and the float64 reference results, computed once."""
    gen = torch.Generator().manual_seed(7 + sw_type)
    params = R.make_params(shape[1], sw_type, tie, affine, gen)
    x, gy = R.make_input(shape, gen)
    if dtype != torch.float32:
        x, gy = x.to(dtype).float(), gy.to(dtype).float()
    ref = R.run(x, gy, params, sw_type, act)
    ref["y_eval"] = R.run_eval(x, params, sw_type, act)
    return x, gy, params, ref


def _run_kernels(K, dev, dtype, x, gy, params, sw_type, act, tie):
    """Training forward + backward and an eval forward through dgvcc_amd.kernels."""
    N, C, H, W = x.shape
    pd = {k: v.to(dev) for k, v in params.items()}
    par = [pd.get(k) for k in PARAMS]
    xd = K.Act(to_nhwc(x).to(dev, dtype))
    ye = K.Act(K.nhwc(N, H, W, C, dtype, dev))
    K.sw_fwd(xd, *par, pd["running_mean"].clone(), pd["running_cov"].clone(), False, act, ye, sw_type=sw_type,
             tie=tie)
    y = K.Act(K.nhwc(N, H, W, C, dtype, dev))
    save = K.sw_fwd(xd, *par, pd["running_mean"], pd["running_cov"], True, act, y, sw_type=sw_type, tie=tie)
    dx = K.Act(K.nhwc(N, H, W, C, dtype, dev))
    d = {k: torch.empty(params[k].shape, device=dev) for k in PARAMS if k in params}
    K.sw_bwd(K.Act(to_nhwc(gy).to(dev, dtype)), y if act else None, xd, save, par[0], par[1], par[2], act, dx,
             d.get("weight"), d.get("bias"), d["sw_mean_weight"], d.get("sw_var_weight"), sw_type=sw_type, tie=tie)
    torch.cuda.synchronize()
    out = {"y": to_nchw(y.buf.float()), "gx": to_nchw(dx.buf.float()), "y_eval": to_nchw(ye.buf.float()),
           "post__running_mean": pd["running_mean"], "post__running_cov": pd["running_cov"]}
    out.update({"grad__" + k: v for k, v in d.items()})
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "t{}_act{}_tie{}_aff{}".format(*map(int, v)))
def test_sw_types_kernels(dev, dtype, shape, variant):
    sw_type, act, tie, affine = variant
    K = _k()
    x, gy, params, ref = _case(shape, sw_type, act, tie, affine, dtype)
    out = _run_kernels(K, dev, dtype, x, gy, params, sw_type, act, tie)
    assert set(out) == set(ref)
    b = _bounds(dtype)
    errs = {k: relerr(out[k], ref[k].reshape(out[k].shape)) for k in sorted(ref)}
    print(errs)
    assert errs["y"] < b["y"] and errs["y_eval"] < b["y"], errs
    assert errs["gx"] < b["dx"], errs
    for k in errs:
        if k.startswith("grad__"):
            assert errs[k] < b["grad"], (k, errs)
    assert errs["post__running_mean"] < b["run"] and errs["post__running_cov"] < b["run"], errs


def _raw_fwd_bwd(K, dev, dtype, x, gy, pd, act, new, sw_type=2, tie=0):
    """dg_sw_fwd + dg_sw_bwd, or (new) dg_swx_fwd + dg_swx_bwd, called directly."""
    N, C, H, W = x.shape
    HW = H * W
    ex = (sw_type, tie) if new else ()
    pre = "dg_swx_" if new else "dg_sw_"
    rm, rc = pd["running_mean"].clone(), pd["running_cov"].clone()
    xd = K.Act(to_nhwc(x).to(dev, dtype))
    gd = K.Act(to_nhwc(gy).to(dev, dtype))
    y = K.Act(K.nhwc(N, H, W, C, dtype, dev))
    dx = K.Act(K.nhwc(N, H, W, C, dtype, dev))
    nsave = K.query("dg_swx_save_size", N, C, sw_type) if new else K.query("dg_sw_save_size", N, C)
    save = torch.zeros(nsave // 4, device=dev)
    work = torch.empty(K.query("dg_sw_workspace", N, HW, C) // 4 + 1, device=dev)
    mw, vw, gam, bet = (pd[k] for k in PARAMS)
    K.call(pre + "fwd", xd.dt, xd.ptr, xd.ld, N, HW, C, *ex, 5, 1e-5, 0.9, K.ptr(mw), K.ptr(vw), K.ptr(gam),
           K.ptr(bet), K.ptr(rm), K.ptr(rc), 1, act, K.ptr(save), y.ptr, y.ld, K.ptr(work), K.stream())
    d = {k: torch.empty_like(pd[k]) for k in PARAMS}
    K.call(pre + "bwd", xd.dt, gd.ptr, gd.ld, y.ptr, y.ld, xd.ptr, xd.ld, N, HW, C, *ex, 5, 1e-5, K.ptr(mw),
           K.ptr(vw), K.ptr(gam), act, K.ptr(save), dx.ptr, dx.ld, 0, K.ptr(d["weight"]), K.ptr(d["bias"]),
           K.ptr(d["sw_mean_weight"]), K.ptr(d["sw_var_weight"]), K.ptr(work), K.stream())
    torch.cuda.synchronize()
    return dict(y=y.buf, dx=dx.buf, rm=rm, rc=rc, save=save, **d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 64, 9, 7), (2, 256, 6, 5)], ids=lambda s: "x".join(map(str, s)))
def test_type2_entry_points_bit_identical(dev, dtype, shape):
    """sw_type 2, untied, affine through dg_swx_*: outputs, gradients, running statistics (and the saved
    statistics) torch.equal to dg_sw_fwd / dg_sw_bwd on the same inputs."""
    K = _k()
    gen = torch.Generator().manual_seed(21)
    params = R.make_params(shape[1], 2, False, True, gen)
    x, gy = R.make_input(shape, gen)
    pd = {k: v.to(dev) for k, v in params.items()}
    old = _raw_fwd_bwd(K, dev, dtype, x, gy, pd, 1, new=False)
    new = _raw_fwd_bwd(K, dev, dtype, x, gy, pd, 1, new=True)
    for k in old:
        assert torch.equal(old[k], new[k]), k
    assert old["y"].float().abs().max() > 0 and old["dx"].float().abs().max() > 0


@pytest.mark.parametrize("variant", [(3, False, True), (5, True, False), (5, False, True)],
                         ids=lambda v: "t{}_tie{}_aff{}".format(*map(int, v)))
def test_split_phases_equal_full_batch(dev, variant):
    """stats on two halves of a batch of 4, the [G][272] moments summed on the host, finish(count = 4)
    on each half: the full-batch forward within 2e-6 (f32; the project's bound for a changed summation
    order).  The backward's bmoments, summed the same way, and dx, dgamma / dbeta and the mixing-weight
    gradients (sums over the halves) against the full-batch backward."""
    sw_type, tie, affine = variant
    K = _k()
    N, C, H, W = 4, 64, 7, 5
    HW = H * W
    gen = torch.Generator().manual_seed(31)
    params = R.make_params(C, sw_type, tie, affine, gen)
    x, gy = R.make_input((N, C, H, W), gen)
    pd = {k: v.to(dev) for k, v in params.items()}
    mw, vw, gam, bet = (K.ptr(pd.get(k)) for k in PARAMS)
    nmom = K.query("dg_sw_moments_size", C) // 8

    def phases(xs, gs, count, mom_sum=None, bm_sum=None):
        """One rank's part: returns its moments / bmoments, and the results when the sums are given."""
        n = xs.shape[0]
        xd, gd = K.Act(to_nhwc(xs).to(dev)), K.Act(to_nhwc(gs).to(dev))
        y, dx = K.Act(K.nhwc(n, H, W, C, torch.float32, dev)), K.Act(K.nhwc(n, H, W, C, torch.float32, dev))
        save = torch.empty(K.query("dg_swx_save_size", n, C, sw_type) // 4, device=dev)
        work = torch.empty(K.query("dg_sw_workspace", n, HW, C) // 4 + 1, device=dev)
        mom = torch.empty(nmom, dtype=torch.float64, device=dev)
        bm = torch.empty(nmom, dtype=torch.float64, device=dev)
        rm, rc = pd["running_mean"].clone(), pd["running_cov"].clone()
        d = {k: torch.empty_like(pd[k]) for k in PARAMS if k in pd}
        K.call("dg_swx_fwd_stats", xd.dt, xd.ptr, xd.ld, n, HW, C, sw_type, K.ptr(save), K.ptr(mom), K.ptr(work),
               K.stream())
        if mom_sum is None:
            return mom, None, None
        K.call("dg_swx_fwd_finish", xd.dt, xd.ptr, xd.ld, n, HW, C, sw_type, int(tie), 5, 1e-5, 0.9, mw, vw, gam,
               bet, K.ptr(rm), K.ptr(rc), 1, 1, count, K.ptr(mom_sum), K.ptr(save), y.ptr, y.ld, K.stream())
        K.call("dg_swx_bwd_stats", xd.dt, gd.ptr, gd.ld, y.ptr, y.ld, xd.ptr, xd.ld, n, HW, C, sw_type, int(tie), 5,
               1e-5, mw, vw, gam, 1, K.ptr(save), K.ptr(bm), K.ptr(d.get("weight")), K.ptr(d.get("bias")),
               K.ptr(work), K.stream())
        if bm_sum is None:
            return mom, bm, None
        K.call("dg_swx_bwd_finish", xd.dt, gd.ptr, gd.ld, y.ptr, y.ld, xd.ptr, xd.ld, n, HW, C, sw_type, int(tie), 1,
               mw, vw, K.ptr(save), count, K.ptr(bm_sum), dx.ptr, dx.ld, 0, K.ptr(d["sw_mean_weight"]),
               K.ptr(d.get("sw_var_weight")), K.ptr(work), K.stream())
        torch.cuda.synchronize()
        return mom, bm, dict(y=y.buf, dx=dx.buf, rm=rm, rc=rc, **d)

    halves = [(x[:2], gy[:2]), (x[2:], gy[2:])]
    mom_sum = sum(phases(xs, gs, N)[0] for xs, gs in halves)
    bm_sum = sum(phases(xs, gs, N, mom_sum)[1] for xs, gs in halves)
    parts = [phases(xs, gs, N, mom_sum, bm_sum)[2] for xs, gs in halves]
    mom_full = phases(x, gy, N)[0]
    bm_full = phases(x, gy, N, mom_full)[1]
    full = phases(x, gy, N, mom_full, bm_full)[2]

    tol = 2e-6
    assert relerr(mom_sum, mom_full) < tol
    assert relerr(torch.cat([p["y"] for p in parts]), full["y"]) < tol
    for p in parts:  # every rank holds the batch's running statistics
        assert relerr(p["rm"], full["rm"]) < tol and relerr(p["rc"], full["rc"]) < tol
    assert relerr(bm_sum, bm_full) < tol
    assert relerr(torch.cat([p["dx"] for p in parts]), full["dx"]) < tol
    for k in PARAMS:
        if k in pd:
            assert relerr(parts[0][k] + parts[1][k], full[k]) < tol, k
    # and the full batch through the phases is the one-call forward / backward of dgvcc_amd.kernels
    ref = R.run(x, gy, params, sw_type, act=1)
    assert relerr(to_nchw(full["y"]), ref["y"]) < 1e-4 and relerr(to_nchw(full["dx"]), ref["gx"]) < 1e-3


def _flat_dot(gs, us):
    return sum((g.double().cpu() * u.double()).sum().item() for g, u in zip(gs, us))


def _check_directions(g32, g64, dirs, what):
    for us in dirs:
        d32, d64 = _flat_dot(g32, us), _flat_dot(g64, us)
        print(what, "directional derivative f32 / f64 / rel:", d32, d64, abs(d32 - d64) / abs(d64))
        assert abs(d32 - d64) < 1e-3 * abs(d64), (what, d32, d64)


@pytest.mark.parametrize("variant", [(5, False, True), (5, True, False), (3, False, True)],
                         ids=lambda v: "t{}_tie{}_aff{}".format(*map(int, v)))
def test_module_forward_autograd(dev, variant):
    """SwitchWhiten2d(32, sw_type=...).forward on an NCHW tensor: output, input gradient, parameter
    gradients and running statistics against sw_ref.  Directional derivatives: for seeded directions u
    over (x, parameters), the f32 <grad, u> within 1e-3 (the f32 gradient bound) of the float64 <grad, u>
    itself, |d32 - d64| < 1e-3 |d64|: a bound on the derivative along u, which errors that pass the
    per-tensor max-norm checks can still miss.  The same in eval mode (running statistics as constants:
    no batch adjoint), and a parameter written in place between forward and backward is refused."""
    from dgvcc_amd.models.trunks import SwitchWhiten2d
    sw_type, tie, affine = variant
    shape = (2, 32, 5, 7)
    gen = torch.Generator().manual_seed(41)
    params = R.make_params(32, sw_type, tie, affine, gen)
    x, gy = R.make_input(shape, gen)
    ref = R.run(x, gy, params, sw_type)
    m = SwitchWhiten2d(32, sw_type=sw_type, tie_weight=tie, affine=affine, momentum=0.9)
    m.load_state_dict(params)
    m = m.to(dev).train()
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.is_cuda
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    assert relerr(y.detach(), ref["y"]) < 1e-4
    assert relerr(xd.grad, ref["gx"]) < 1e-3
    names = [k for k in PARAMS if k in params]
    for k in names:
        g = getattr(m, k).grad
        assert g is not None and g.dtype == torch.float32 and g.shape == params[k].shape
        assert relerr(g, ref["grad__" + k]) < 1e-3, k
    assert relerr(m.running_mean, ref["post__running_mean"]) < 1e-4
    assert relerr(m.running_cov, ref["post__running_cov"]) < 1e-4
    g32 = [xd.grad] + [getattr(m, k).grad for k in names]
    g64 = [ref["gx"]] + [ref["grad__" + k] for k in names]
    dirs = [[torch.randn(g.shape, generator=gen) for g in g64] for _ in range(4)]
    _check_directions(g32, g64, dirs, "train")
    # eval mode: the running statistics just updated, no update
    m.eval()
    rm0 = m.running_mean.clone()
    with torch.no_grad():
        ye = m(x.to(dev))
    pe = dict(params, running_mean=ref["post__running_mean"], running_cov=ref["post__running_cov"])
    assert relerr(ye, R.run_eval(x, pe, sw_type)) < 1e-4 and torch.equal(m.running_mean, rm0)
    # eval-mode gradients: the reference operator differentiates through eval (frozen statistics)
    refe = R.run(x, gy, pe, sw_type, training=False)
    m.zero_grad()
    xe = x.to(dev).requires_grad_(True)
    m(xe).backward(gy.to(dev))
    torch.cuda.synchronize()
    assert relerr(xe.grad, refe["gx"]) < 1e-3
    for k in names:
        assert relerr(getattr(m, k).grad, refe["grad__" + k]) < 1e-3, k
    _check_directions([xe.grad] + [getattr(m, k).grad for k in names],
                      [refe["gx"]] + [refe["grad__" + k] for k in names], dirs, "eval")
    assert torch.equal(m.running_mean, rm0)
    # a parameter written in place after the forward: autograd's version check, not a stale gradient
    yv = m(x.to(dev))
    with torch.no_grad():
        m.sw_mean_weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        yv.backward(gy.to(dev))
    with torch.no_grad():
        m.sw_mean_weight.sub_(1.0)
    # 16-bit input: same shape and dtype back
    yb = m(x.to(dev, torch.bfloat16))
    assert yb.dtype == torch.bfloat16 and yb.shape == x.shape
    assert relerr(yb.float(), R.run_eval(x.to(torch.bfloat16).float(), pe, sw_type)) < 3e-2


def test_sw_counter_type5_train_step(dev):
    """One SW-counter train step at 2 x 3 x 64 x 64 with sw_cfg = {'sw_type': 5}: finite losses, a gradient
    on every parameter, and all ten mixing-weight entries of every SW layer move."""
    from oracle import dg_oracle as O
    from dgvcc_amd import main
    from dgvcc_amd.losses import mse_loss
    from dgvcc_amd.models.trunks import SwitchWhiten2d
    model = main.get_model("sw", {"pretrained": False, "sw_cfg": {"sw_type": 5}})
    model.load_state_dict(O.seeded_state_dict(model.state_dict()))
    model = model.to(dev).set_precision("fp32").train()
    img, _, (_, dmaps, _) = O.synthetic_batch(2, 64, 64, seed=2112)
    layers = [m for m in model.modules() if isinstance(m, SwitchWhiten2d)]
    assert len(layers) == 7 and all(m.sw_type == 5 for m in layers)
    before = [torch.cat([m.sw_mean_weight, m.sw_var_weight]).detach().clone() for m in layers]
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss = mse_loss(model(img.to(dev)), dmaps.to(dev), 1000.0)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
    opt.step()
    for m, b in zip(layers, before):
        now = torch.cat([m.sw_mean_weight, m.sw_var_weight]).detach()
        assert now.numel() == 10 and (now != b).all().item(), (now - b)
    with torch.no_grad():
        loss2 = mse_loss(model(img.to(dev)), dmaps.to(dev), 1000.0)
    assert torch.isfinite(loss2).item()
