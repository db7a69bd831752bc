"""The float64 restatements of tests/bn_ref.py against float64 autograd of F.batch_norm(training=True) -> ReLU ->
channel dropout -> F.max_pool2d(2) (dropout before the pool, as the kernels store y), the SyncBatchNorm
restatements against the whole-batch ones on a batch split into two unequal parts, and the conditions the
input makers promise for every case of tests/test_bn_kernels_gpu.py, so that a failure there cannot be
blamed on its inputs.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

TOL = 1e-10


def _close(a, b, what=""):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), (what, err)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _small(act, p, pooled, seed=5):
    N, H, W, C = 3, 6, 10, 8
    return R.make_case(N, H, W, C, torch.float32, seed, act, p, pooled)


def _autograd(i, act, drop, pooled, normalise=True, momentum=0.1):
    """(y, yp, dz, dgamma, dbeta, running_mean, running_var) of the torch graph in float64, for the
    upstream gradients g (of y) and gp (of yp)."""
    z = _nchw(i["z"].double()).clone().requires_grad_(True)
    gam, bet = i["gamma"].double().requires_grad_(True), i["beta"].double().requires_grad_(True)
    rm, rv = i["rm0"].double().clone(), i["rv0"].double().clone()
    t = F.batch_norm(z, rm, rv, gam, bet, True, momentum, i["eps"]) if normalise else z
    y = F.relu(t) if act else t
    if drop is not None:
        y = y * drop.double()[:, :, None, None]
    loss = (y * _nchw(i["g"].double())).sum()
    yp = None
    if pooled:
        yp = F.max_pool2d(y, 2)
        loss = loss + (yp * _nchw(i["gp"].double())).sum()
    loss.backward()
    return (_nhwc(y.detach()), None if yp is None else _nhwc(yp.detach()), _nhwc(z.grad),
            gam.grad if normalise else None, bet.grad if normalise else None, rm, rv)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("p", [None, 0.3])
def test_stats_apply_bwd_against_autograd(act, p):
    i = _small(act, p, False)
    st = R.stats(i["z"], i["gamma"], i["beta"], i["eps"])
    y, _, dz, dgam, dbet, rm, rv = _autograd(i, act, i["drop"], False)
    _close(R.running(i["rm0"], st["mean"], 0.1), rm, "running_mean")
    _close(R.running(i["rv0"], st["unbiased"], 0.1), rv, "running_var")
    _close(R.apply(i["z"], st["scale"], st["shift"], act, i["drop"], i["HW"]), y, "y")
    b = R.bwd(i["g"], i["z"], i["gamma"], st["mean"], st["invstd"], st["scale"], st["shift"], act, i["drop"],
              i["HW"])
    _close(b["dz"], dz, "dz")
    _close(b["dgamma"], dgam, "dgamma")
    _close(b["dbeta"], dbet, "dbeta")
    _close(b["dbias"], dz.reshape(-1, dz.shape[-1]).sum(0), "dbias = sum dz")


def test_stats_single_pixel():
    """M = 1: variance 0 and the running update takes the biased value (no division by M - 1)."""
    z = torch.tensor([[[[0.5, -2.0, 3.0, 0.0]]]])
    st = R.stats(z, None, None, 1e-5)
    assert torch.equal(st["var"], torch.zeros(4, dtype=torch.float64)) and torch.equal(st["unbiased"], st["var"])
    _close(st["invstd"], torch.full((4,), 1e-5, dtype=torch.float64).rsqrt())
    _close(st["shift"], -z.double().reshape(4) * st["scale"])


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("p", [None, 0.3])
def test_unnormalised_against_autograd(act, p):
    i = _small(act, p, False, seed=6)
    y, _, dz, _, _, _, _ = _autograd(i, act, i["drop"], False, normalise=False)
    _close(R.apply(i["z"], None, None, act, i["drop"], i["HW"]), y, "y")
    b = R.bwd(i["g"], i["z"], None, None, None, None, None, act, i["drop"], i["HW"])
    _close(b["dz"], dz, "dz")
    s = dz.reshape(-1, dz.shape[-1]).sum(0)
    _close(b["dbeta"], s, "dbeta")
    _close(b["dbias"], s, "dbias")
    assert not b["dgamma"].any()


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("p", [None, 0.3])
@pytest.mark.parametrize("direct", [False, True])
def test_pooled_against_autograd(act, p, direct):
    """The pooled forms, planted ties included: ATen's max_pool2d also takes the first maximum."""
    i = _small(act, p, True, seed=7)
    if not direct:
        i = dict(i, g=torch.zeros_like(i["g"]))
    st = R.stats(i["z"], i["gamma"], i["beta"], i["eps"])
    y, yp, dz, dgam, dbet, _, _ = _autograd(i, act, i["drop"], True)
    yr = R.apply(i["z"], st["scale"], st["shift"], act, i["drop"], i["HW"])
    bad, tied = R.pool_gaps(i["z"], R.apply(i["z"], st["scale"], st["shift"], act), torch.float32)
    assert bad == 0 and tied >= 0.25
    _close(R.pool_fwd(yr), yp, "yp")
    b = R.pool_bwd(i["gp"], i["g"] if direct else None, yr, i["z"], i["gamma"], st["mean"], st["invstd"],
                   st["scale"], st["shift"], act, i["drop"])
    _close(b["dz"], dz, "dz")
    _close(b["dgamma"], dgam, "dgamma")
    _close(b["dbeta"], dbet, "dbeta")


def test_first_max_rule():
    w = torch.tensor([[1.0, 3.0, 3.0, 2.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]]).t().reshape(1, 1, 1, 4, 3)
    assert R.first_max(w).flatten().tolist() == [1, 0, 2]
    t = torch.arange(2 * 4 * 6 * 3, dtype=torch.float64).reshape(2, 4, 6, 3)
    assert torch.equal(R.unwindows(R.windows(t)), t)
    assert R.windows(t)[0, 0, 0, :, 0].tolist() == [0.0, 3.0, 18.0, 21.0]


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("p", [None, 0.3])
def test_sync_equals_whole_batch(act, p):
    """Two 'ranks' holding 1 and 2 images of one batch: the merged rows give the whole batch's statistics, and
    the phases of the backward its dz; dgamma / dbeta / dbias of the parts add up to the whole batch's."""
    i = _small(act, p, False, seed=8)
    z, g, HW = i["z"], i["g"], i["HW"]
    st = R.stats(z, i["gamma"], i["beta"], i["eps"])
    parts = [slice(0, 1), slice(1, 3)]
    rows = torch.stack([R.row(z[s]) for s in parts])
    ss = R.stats_from_rows(rows, i["gamma"], i["beta"], i["eps"])
    for k in ("mean", "var", "invstd", "scale", "shift", "unbiased"):
        _close(ss[k], st[k], k)
    assert ss["M"] == st["M"]
    # a zero row (syncbn.split_row's second row) changes nothing
    zero = torch.zeros_like(rows[0])
    _close(R.merge(torch.stack([rows[0], zero, rows[1], zero])), R.merge(rows), "zero rows")
    whole = R.bwd(g, z, i["gamma"], st["mean"], st["invstd"], st["scale"], st["shift"], act, i["drop"], HW)
    drops = [None if i["drop"] is None else i["drop"][s] for s in parts]
    args = (st["mean"], st["invstd"], st["scale"], st["shift"], act)
    loc = [R.sums4(g[s], z[s], *args, d, HW)[0] for s, d in zip(parts, drops)]
    glob = loc[0] + loc[1]
    assert float(glob[3, 0] + glob[3, 1]) == st["M"]
    dzs, tot = [], dict(dgamma=0.0, dbeta=0.0, dbias=0.0)
    for s, d, l in zip(parts, drops, loc):
        Ml = z[s].numel() // z.shape[-1]
        f = R.finalize_sync(l, glob, Ml, None, i["gamma"], st["invstd"])
        f2 = R.finalize_sync(l, glob, Ml, st["M"], i["gamma"], st["invstd"])
        for k in ("k1", "k2", "k3"):
            _close(f[k], whole[k], k)
            assert torch.equal(f[k], f2[k])
        dzs.append(R.apply_coef(g[s], z[s], *args, f["k1"], f["k2"], f["k3"], d, HW)[0])
        for k in tot:
            tot[k] = tot[k] + f[k]
    _close(torch.cat(dzs), whole["dz"], "dz")
    for k in tot:
        _close(tot[k], whole[k], k)


# ------------------------------------------------------------------ the input conditions ------
ALL_PLAIN = R.plain_cases() + [c for dt in R.DTYPES for c in (R.slice_case(dt), R.nonorm_case(dt),
                                                               R.m3137_case(dt), R.sync_case(dt))]
ALL_POOLED = R.pooled_cases() + [R.sync_pool_case(dt) for dt in (R.F32, R.BF16)]


@pytest.mark.parametrize("case", ALL_PLAIN + ALL_POOLED, ids=lambda c: c.name)
def test_input_conditions(case):
    i = R.inputs(case)
    z = i["z"]
    assert z.dtype == case.dt and i["g"].dtype == case.dt and torch.isfinite(z.float()).all()
    st = R.stats(z, i["gamma"], i["beta"], i["eps"])
    if case.act == 1:  # every element: the sign of the pre-activation is beyond any f32 evaluation's reach
        assert R.relu_margin(z, st["scale"], st["shift"]) >= 1e-3
    # shift = beta - mean scale does not cancel (its relative bound means something)
    assert (st["shift"].abs() >= 0.99 * (i["beta"].double().abs() + (st["mean"] * st["scale"]).abs())).all()
    if case.p is not None:
        assert R.drop_ok(i["drop"], case.p)
    if case.pooled:
        bad, tied = R.pool_gaps(z, R.apply(z, st["scale"], st["shift"], case.act), case.dt)
        assert bad == 0, "window values neither equal nor > 4 ulp apart"
        assert tied >= 0.25, "planted ties lost"
        if case.p is not None:  # also with the dropout zeros in place
            assert R.pool_gaps(z, R.apply(z, st["scale"], st["shift"], case.act, i["drop"], i["HW"]), case.dt)[0] == 0


def test_nonorm_margin():
    """The unnormalised ReLU mask is z > 0: no stored z is zero."""
    for dt in R.DTYPES:
        assert (R.inputs(R.nonorm_case(dt))["z"].float() != 0).all()


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.IDS[d])
@pytest.mark.parametrize("delta", [0, 8, 64])
def test_stress_inputs(dt, delta):
    mean0, std0 = ((4096.0, 1.0) if dt == R.F32 else (16.0, 0.25)) if delta == 0 else (0.0, 1.0 if dt == R.F32 else 0.25)
    z, d = R.make_stress(3137, 64, dt, 40 + delta, mean0, std0, delta)
    x = z.double().reshape(-1, 64)
    if delta == 0:
        assert (d <= 1.0).all() and (x.mean(0).abs() >= 50 * x.std(0)).all()
    else:
        # delta deviations of the other pixels; d, the conditioning the bound uses, counts the outlier
        # in the deviation as well and is smaller
        assert (((x[0] - x[1:].mean(0)).abs() / x[1:].std(0) - delta).abs() <= 0.1 * delta).all()
        assert (d <= 1.1 * delta).all() and (d >= 0.5 * delta).all()
