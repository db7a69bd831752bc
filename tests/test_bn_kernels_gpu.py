"""Kernel-level tests of the BatchNorm passes of norm.hip (statistics, apply, backward, the forms fused with
the 2x2 max pool, the SyncBatchNorm phase entries) against the float64 restatements of tests/bn_ref.py, per
element and per channel in max norm: never against a whole-tensor maximum, never an L2 norm.  The references
take the stored inputs and, where a kernel takes statistics rows, the kernel's own stored f32 rows, so each
kernel is judged as the function it implements; tests/test_bn_ref_cpu.py asserts the input conditions (ReLU
margin, window gaps and planted ties, dropout masks) on the reference alone.

Bounds (derived, not measured; e = 2^-24, S = 512 e).
  sums (dgamma, dbeta, dbias, the sum rows, a row's M2): S sum|terms| of the channel + e |ref|.  No f32 chain
    of these passes is longer than 256 LDS rows + 65 pixels (un-pooled) or 128 window values + 256 LDS rows
    (pooled) at the shapes below; the rest is double.
  coefficients: k1 one product (e |k1|); k2 = k1 sum g'xhat / M and k3 = k1 sum g' / M the sum bound scaled by
    |k1| / M, + 2 e |k| (k1's rounding and their own).
  f32 elements: tol max over the channel's pixels of the sum of the absolute terms (y: |z scale| + |shift|,
    with or without drop, tol 2e-5; dz: |k1 g'| + |k2 xhat| + |k3|, tol 1e-4: the older tests' tolerances), dz plus
    the coefficient bounds, |xhat| B(k2) + B(k3).
  16-bit elements: on top, one ulp of the storage type, u_T |ref| (u = 2^-8 bf16, 2^-11 f16; + 2^-24 f16).
  mean, invstd, scale, shift, running statistics: 1e-5 |ref| per channel.
  stress variance: 1e-5 (1 + delta^2) var per channel, delta the measured distance of the first pixel (the
    kernels' shift) from the channel mean in deviations: the conditioning of a sum shifted by that pixel.
  amax words: equal to max |stored output| exactly.
"""
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
E = 2.0 ** -24
S = 512 * E
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
MOM = 0.1
SENT = -7777.0


def _k():
    from dgvcc_amd import kernels as K
    return K


def _sb():
    from dgvcc_amd import syncbn
    return syncbn


@pytest.fixture(autouse=True)
def _end_run_on_device_fault():
    """A device fault ends the run: nothing more is launched on a faulted device."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device fault: {e}", returncode=3)


# ------------------------------------------------------------------------------ comparisons ------
def within(out, ref, bound, what):
    """|out - ref| <= bound per element (bound broadcast over the pixels)."""
    out, ref = out.detach().double().cpu(), ref.double()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), (what, "non-finite output")
    err = (out - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    print(f"  {what}: max err {err.max().item():.3e}, worst err / bound {ratio.max().item():.3f}")
    over = err > bound
    assert not over.any(), (what, "elements over the bound: %d, worst err / bound %.3f at %s" % (
        int(over.sum()), ratio.max().item(), tuple(torch.nonzero(ratio == ratio.max())[0].tolist())))


def stored(bound, ref, dt):
    """The bound of a value stored once in dt from an f32 value with bound `bound`."""
    if dt == F32:
        return bound
    return bound + U[dt] * ref.abs() + (2.0 ** -24 if dt == F16 else 0.0)


def chanmax(t):
    return t.reshape(-1, t.shape[-1]).max(0).values


def rel(out, ref, tol, what):
    within(out, ref, tol * ref.double().abs(), what)


def sum_bound(abs_sum, ref):
    return S * abs_sum + E * ref.abs()


def check_amax(a, what):
    """f32: the tensor word and every channel word equal max |stored output| exactly."""
    if a.buf.dtype != F32:
        return
    K = _k()
    assert a.amax is not None and a.amax.numel() == K.amax_words(a.C), what
    v = a.view().float().abs().reshape(-1, a.C).max(0).values
    assert torch.equal(a.amax[1:1 + a.C], v), (what, "channel words")
    assert a.amax[0].item() == v.max().item(), (what, "tensor word")


def act_of(t, dev, sliced=False, fill=None):
    """t [N, H, W, C] on the device as an Act; sliced: channels [V, V + C) of a buffer C + 2 V wide whose
    other channels hold SENT.  fill: the value of an output buffer instead of t's."""
    K = _k()
    N, H, W, C = t.shape
    V = R.VEC[t.dtype]
    if not sliced:
        return K.Act(t.to(dev) if fill is None else torch.full((N, H, W, C), fill, dtype=t.dtype, device=dev))
    buf = torch.full((N, H, W, C + 2 * V), SENT, dtype=t.dtype, device=dev)
    buf[..., V:V + C] = t.to(dev) if fill is None else fill
    return K.Act(buf, off=V, C=C)


def neighbours_intact(a, what):
    if a.buf.shape[3] == a.C:
        return
    rest = torch.cat([a.buf[..., :a.off], a.buf[..., a.off + a.C:]], -1)
    assert torch.equal(rest, torch.full_like(rest, SENT)), (what, "neighbouring channels written")


def dz_bound(b, dt, tol=1e-4, extra_sum_round=0.0):
    """Per-element bound of dz for the reference b (bn_ref.bwd): tol chanmax(terms) + |xhat| B(k2) + B(k3)."""
    M, a, s, k1 = b["M"], b["abs_sums"], b["sums"], b["k1"].abs()
    bk2 = k1 / M * (sum_bound(a[1], s[1]) + extra_sum_round * s[1].abs()) + 2 * E * b["k2"].abs()
    bk3 = k1 / M * (sum_bound(a[0], s[0]) + extra_sum_round * s[0].abs()) + 2 * E * b["k3"].abs()
    if not (b["k2"].any() or b["k3"].any()):  # no normalisation: dz = g'
        bk2, bk3 = 0.0 * bk2, 0.0 * bk3
    bound = tol * chanmax(b["terms"]) + b["xhat"].abs().reshape(b["dz"].shape) * bk2 + bk3
    return stored(bound, b["dz"], dt), bk2, bk3


def check_bwd(b, dt, dz, dgam, dbet, dbias, coef=None, what="bwd"):
    a, s = b["abs_sums"], b["sums"]
    bound, bk2, bk3 = dz_bound(b, dt)
    within(dz, b["dz"], bound, what + " dz")
    within(dgam, b["dgamma"], sum_bound(a[1], s[1]) if b["dgamma"].any() else 0.0, what + " dgamma")
    within(dbet, b["dbeta"], sum_bound(a[0], s[0]), what + " dbeta")
    if b["k2"].any():
        within(dbias, b["dbias"], S * b["k2"].abs() * a[2] + E * b["dbias"].abs(), what + " dbias")
    else:
        within(dbias, b["dbias"], sum_bound(a[0], s[0]), what + " dbias")
    if coef is not None:
        within(coef[0], b["k1"], E * b["k1"].abs(), what + " k1")
        within(coef[1], b["k2"], bk2, what + " k2")
        within(coef[2], b["k3"], bk3, what + " k3")


def y_bound(z, scale, shift, ref, dt):
    zs, sf = R.pre(z, scale, shift)
    return stored(2e-5 * chanmax(zs.abs() + sf.abs()), ref, dt)


def check_stats(sd, st, rm, rv, i, what="stats"):
    for k, row in zip(("mean", "invstd", "scale", "shift"), sd):
        rel(row, st[k], 1e-5, f"{what} {k}")
    rel(rm, R.running(i["rm0"], st["mean"], MOM), 1e-5, what + " running_mean")
    rel(rv, R.running(i["rv0"], st["unbiased"], MOM), 1e-5, what + " running_var")


def fwd_train(K, dev, zA, i):
    rm, rv = i["rm0"].to(dev), i["rv0"].to(dev)
    stats = K.bn_fwd_train(zA, i["gamma"].to(dev), i["beta"].to(dev), rm, rv, MOM, i["eps"])
    return stats, rm, rv


def _f32(C, dev):
    return torch.full((C,), SENT, dtype=F32, device=dev)


# ------------------------------------------------------------------------------ un-pooled passes --
def run_plain(dev, case, sliced=False):
    K, sb = _k(), _sb()
    i = R.inputs(case)
    z, g, drop, HW, act, dt, C = i["z"], i["g"], i["drop"], i["HW"], case.act, case.dt, case.C
    gam, dropd = i["gamma"].to(dev), None if drop is None else drop.to(dev)
    zA, gA = act_of(z, dev, sliced), act_of(g, dev, sliced)
    stats, rm, rv = fwd_train(K, dev, zA, i)
    yA, dzA, dz2A = (act_of(z, dev, sliced, fill=SENT) for _ in range(3))
    K.bn_apply(zA, stats, act, yA, dropd)
    dgam, dbet, dbias = _f32(C, dev), _f32(C, dev), _f32(C, dev)
    K.bn_bwd(gA, zA, gam, stats, act, dzA, dgam, dbet, dbias, dropd)
    dgam2, dbet2, dbias2 = _f32(C, dev), _f32(C, dev), _f32(C, dev)
    coef = K.bn_bwd_coef(gA, zA, gam, stats, act, dgam2, dbet2, dbias2, dropd)
    sb.bwd_apply(gA, zA, stats, act, coef, dz2A, dropd)
    torch.cuda.synchronize()
    sd = stats.cpu()
    check_stats(sd, R.stats(z, i["gamma"], i["beta"], i["eps"]), rm, rv, i)
    yr = R.apply(z, sd[2], sd[3], act, drop, HW)
    within(yA.view(), yr, y_bound(z, sd[2], sd[3], yr, dt), "y")
    if drop is not None:
        assert not yA.view()[(R.drop_rows(drop, HW) == 0).reshape(z.shape)].any(), "dropped y not zero"
    check_bwd(R.bwd(g, z, i["gamma"], sd[0], sd[1], sd[2], sd[3], act, drop, HW), dt, dzA.view(), dgam, dbet, dbias,
              coef.cpu())
    for a, what in ((yA, "y"), (dzA, "dz"), (dz2A, "dz (coef)")):
        check_amax(a, what)
        neighbours_intact(a, what)
    # coefficients, then their application = the one-call backward, bit for bit
    assert torch.equal(dz2A.buf, dzA.buf), "bn_bwd_coef + bn_bwd_apply_coef != bn_bwd"
    assert torch.equal(dgam2, dgam) and torch.equal(dbet2, dbet) and torch.equal(dbias2, dbias)


PLAIN = R.plain_cases()


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: c.name)
def test_bn_plain(dev, case):
    run_plain(dev, case)


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.IDS[d])
def test_bn_channel_slice(dev, dt):
    """z, y, g, dz as channels [V, V + C) of separate buffers C + 2 V wide (ld > C), with dropout."""
    run_plain(dev, R.slice_case(dt), sliced=True)


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.IDS[d])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("use_drop", [False, True], ids=["nodrop", "drop"])
def test_bn_bwd_unnormalised(dev, dt, act, use_drop):
    """stats = None: dz = act'(z) g drop, dbeta = dbias = sum dz, dgamma = 0 (the !invstd arm of bn_bwd_finalize)."""
    K = _k()
    case = R.nonorm_case(dt)
    i = R.inputs(case)
    z, g, HW, C = i["z"], i["g"], i["HW"], case.C
    drop = i["drop"] if use_drop else None
    zA, gA, dzA = act_of(z, dev), act_of(g, dev), act_of(z, dev, fill=SENT)
    dgam, dbet, dbias = _f32(C, dev), _f32(C, dev), _f32(C, dev)
    K.bn_bwd(gA, zA, None, None, act, dzA, dgam, dbet, dbias, None if drop is None else drop.to(dev))
    torch.cuda.synchronize()
    check_bwd(R.bwd(g, z, None, None, None, None, None, act, drop, HW), dt, dzA.view(), dgam, dbet, dbias)
    check_amax(dzA, "dz")


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.IDS[d])
def test_bn_unroll_bit_identical(dev, dt, monkeypatch):
    """DGVCC_EW_UNROLL = 2 and 4 (read per launch) give bn_apply and bn_bwd bit for bit (M = 3137, C = 64).  The
    f32 entries take their 256-thread kernels only without an amax buffer, so the entries are called directly;
    the wrappers' f32 form (1024 threads, amax) must agree as well."""
    K = _k()
    case = R.m3137_case(dt)
    i = R.inputs(case)
    M, C, act = case.N * case.H * case.W, case.C, case.act
    zA, gA = act_of(i["z"], dev), act_of(i["g"], dev)
    gam = i["gamma"].to(dev)
    stats, _, _ = fwd_train(K, dev, zA, i)
    work = torch.empty(K.query("dg_bn_workspace", M, C) // 4 + 1, device=dev)

    def run():
        y, dz = torch.full_like(zA.buf, SENT), torch.full_like(zA.buf, SENT)
        rows = [_f32(C, dev) for _ in range(3)]
        K.call("dg_bn_apply", zA.dt, zA.ptr, zA.ld, M, C, K.ptr(stats[2]), K.ptr(stats[3]), act, None, M,
               K.ptr(y), C, None, K.stream())
        K.call("dg_bn_bwd", zA.dt, gA.ptr, gA.ld, zA.ptr, zA.ld, M, C, K.ptr(gam), K.ptr(stats[0]), K.ptr(stats[1]),
               K.ptr(stats[2]), K.ptr(stats[3]), act, None, M, K.ptr(dz), C, K.ptr(rows[0]), K.ptr(rows[1]),
               K.ptr(rows[2]), K.ptr(work), None, K.stream())
        torch.cuda.synchronize()
        return [y, dz] + rows

    base = run()
    for u in ("2", "4"):
        monkeypatch.setenv("DGVCC_EW_UNROLL", u)
        for a, b, what in zip(run(), base, ("y", "dz", "dgamma", "dbeta", "dbias")):
            assert torch.equal(a, b), (what, "DGVCC_EW_UNROLL=" + u)
    monkeypatch.delenv("DGVCC_EW_UNROLL")
    yA, dzA = act_of(i["z"], dev, fill=SENT), act_of(i["z"], dev, fill=SENT)
    K.bn_apply(zA, stats, act, yA)
    K.bn_bwd(gA, zA, gam, stats, act, dzA, _f32(C, dev), _f32(C, dev), _f32(C, dev))
    torch.cuda.synchronize()
    assert torch.equal(yA.buf, base[0]) and torch.equal(dzA.buf, base[1]), "wrapper form"


# ------------------------------------------------------------------------------ pooled passes -----
def run_pooled(dev, case, use_drop, use_gd, with_y):
    K = _k()
    i = R.inputs(case)
    z, HW, act, dt, C = i["z"], i["HW"], case.act, case.dt, case.C
    drop = i["drop"] if use_drop else None
    gd = i["g"] if use_gd else None
    gam, dropd = i["gamma"].to(dev), None if drop is None else drop.to(dev)
    N, H, W, _ = z.shape
    zA = act_of(z, dev)
    stats, _, _ = fwd_train(K, dev, zA, i)
    yA = act_of(z, dev, fill=SENT)
    ypA = K.Act(torch.full((N, H // 2, W // 2, C), SENT, dtype=dt, device=dev))
    K.bn_apply_pool(zA, stats, act, yA, ypA, dropd)
    if not with_y:  # the forward without y: the same yp and amax words
        yp2 = K.Act(torch.full_like(ypA.buf, SENT))
        K.bn_apply_pool(zA, stats, act, None, yp2, dropd)
    dzA = act_of(z, dev, fill=SENT)
    dgam, dbet, dbias = _f32(C, dev), _f32(C, dev), _f32(C, dev)
    K.bn_bwd_pool(act_of(i["gp"], dev), None if gd is None else act_of(gd, dev), zA, gam, stats, act, dzA, dgam,
                  dbet, dbias, dropd)
    torch.cuda.synchronize()
    sd = stats.cpu()
    yr = R.apply(z, sd[2], sd[3], act, drop, HW)
    within(yA.view(), yr, y_bound(z, sd[2], sd[3], yr, dt), "y")
    ys = yA.buf.cpu()  # the stored y: the first-max rule and the backward's routing are judged on it
    assert torch.equal(ypA.buf.cpu().double(), R.pool_fwd(ys)), "yp is not the first max of the stored y"
    check_amax(yA, "y")
    if dt == F32:
        assert ypA.amax is yA.amax
    if not with_y:
        assert torch.equal(yp2.buf, ypA.buf), "yp without y"
        if dt == F32:
            assert torch.equal(yp2.amax, yA.amax), "amax without y"
    b = R.pool_bwd(i["gp"], gd, ys, z, i["gamma"], sd[0], sd[1], sd[2], sd[3], act, drop)
    check_bwd(b, dt, dzA.view(), dgam, dbet, dbias, what="pool bwd")
    check_amax(dzA, "dz")


@pytest.mark.parametrize("case", R.pooled_cases(), ids=lambda c: c.name)
def test_bn_pooled(dev, case):
    big = case.C == 1024
    for use_drop, use_gd, with_y in [(True, True, True)] if big else [(True, True, True), (False, False, False),
                                                                      (True, False, False), (False, True, True)]:
        print(f" drop {use_drop} gd {use_gd} y {with_y}")
        run_pooled(dev, case, use_drop, use_gd, with_y)


# ------------------------------------------------------------------------------ rejected shapes ---
def test_bn_rejected_shapes(dev):
    """C / V not dividing 256, f32 C = 2048, ld no multiple of V, odd H or W of the pooled entries:
    DG_ERR_UNSUPPORTED (-2) and nothing written."""
    K = _k()
    st = K.lib_call_status

    def bufs(dt, M, ld):
        z = torch.zeros(M * ld, dtype=dt, device=dev)
        return z, torch.zeros_like(z), torch.full_like(z, SENT), torch.full_like(z, SENT)

    rows = torch.full((8, 2048), SENT, dtype=F32, device=dev)
    ones = torch.ones(4, 2048, dtype=F32, device=dev)
    work = torch.empty(1 << 20, dtype=F32, device=dev)
    s = K.stream()
    p = K.ptr
    for dt, C, ld in ((F32, 12, 12), (BF16, 24, 24), (F16, 24, 24), (F32, 2048, 2048), (F32, 64, 66), (BF16, 64, 68),
                      (F16, 64, 68)):
        code, M = K.dtype_code(dt), 8
        z, g, y, dz = bufs(dt, M, ld)
        r = [st("dg_bn_fwd_train", code, p(z), ld, M, C, p(ones[0]), p(ones[1]), None, None, 0.1, 1e-5, p(rows[0]),
                p(rows[1]), p(rows[2]), p(rows[3]), p(work), s),
             st("dg_bn_stats_row", code, p(z), ld, M, C, p(rows[0]), p(work), s),
             st("dg_bn_apply", code, p(z), ld, M, C, p(ones[0]), p(ones[1]), 1, None, M, p(y), ld, None, s),
             st("dg_bn_bwd", code, p(g), ld, p(z), ld, M, C, p(ones[0]), p(ones[0]), p(ones[1]), p(ones[2]),
                p(ones[3]), 1, None, M, p(dz), ld, p(rows[4]), p(rows[5]), p(rows[6]), p(work), None, s),
             st("dg_bn_bwd_sums", code, p(g), ld, p(z), ld, M, C, p(ones[0]), p(ones[1]), p(ones[2]), p(ones[3]), 1,
                None, M, p(rows[7]), p(work), s),
             st("dg_bn_bwd_apply_coef", code, p(g), ld, p(z), ld, M, C, p(ones[0]), p(ones[1]), p(ones[2]),
                p(ones[3]), 1, None, M, p(ones), p(dz), ld, None, s)]
        torch.cuda.synchronize()
        assert r == [-2] * 6, (dt, C, ld, r)
        for t in (y, dz, rows):
            assert torch.equal(t, torch.full_like(t, SENT)), (dt, C, ld, "output written")
    for dt in R.DTYPES:
        for H, W in ((3, 4), (4, 3)):
            code, C, N = K.dtype_code(dt), 64, 1
            z, g, y, dz = bufs(dt, N * H * W, C)
            r = [st("dg_bn_apply_pool", code, p(z), C, N, H, W, C, p(ones[0]), p(ones[1]), 1, None, p(y), C, p(dz), C,
                    None, s),
                 st("dg_bn_bwd_pool", code, p(g), C, None, 0, p(z), C, N, H, W, C, p(ones[0]), p(ones[0]), p(ones[1]),
                    p(ones[2]), p(ones[3]), 1, None, p(dz), C, p(rows[4]), p(rows[5]), p(rows[6]), p(work), None, s),
                 st("dg_bn_bwd_pool_sums", code, p(g), C, None, 0, p(z), C, N, H, W, C, p(ones[0]), p(ones[1]),
                    p(ones[2]), p(ones[3]), 1, None, p(rows[7]), p(work), s),
                 st("dg_bn_bwd_pool_apply_coef", code, p(g), C, None, 0, p(z), C, N, H, W, C, p(ones[0]), p(ones[1]),
                    p(ones[2]), p(ones[3]), 1, None, p(ones), p(dz), C, None, s)]
            torch.cuda.synchronize()
            assert r == [-2] * 4, (dt, H, W, r)
            for t in (y, dz, rows):
                assert torch.equal(t, torch.full_like(t, SENT)), (dt, H, W, "output written")


# ------------------------------------------------------------------------------ statistics stress -
def _stress(dt, delta):
    mean0, std0 = ((4096.0, 1.0) if dt == F32 else (16.0, 0.25)) if delta == 0 else (0.0, 1.0 if dt == F32 else 0.25)
    return R.make_stress(3137, 64, dt, 40 + delta, mean0, std0, delta)


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.IDS[d])
@pytest.mark.parametrize("delta", [0, 8, 64])
def test_bn_stats_stress(dev, dt, delta):
    """(a) delta = 0: |mean| >> std (4096 / 1 in f32, 16 / 0.25 in 16 bits), first pixel within a deviation of
    the mean; (b) first pixel 8 and 64 deviations out, mean 0.  The variance of dg_bn_fwd_train (read from the
    running variance: momentum 1 on a zero row stores the unbiased value itself) and of dg_bn_stats_row (M2 / M)
    within 1e-5 (1 + d^2) var, d the measured distance of the first pixel from the mean in deviations."""
    K, sb = _k(), _sb()
    z, d = _stress(dt, delta)
    M, C = 3137, 64
    zA = act_of(z, dev)
    rm, rv = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    stats = K.bn_fwd_train(zA, None, None, rm, rv, 1.0, 1e-5)
    row = sb.row_from_z(zA)
    torch.cuda.synchronize()
    st = R.stats(z, None, None, 1e-5)
    bound = 1e-5 * (1.0 + d * d) * st["var"]
    for what, var in (("fwd_train", rv.double().cpu() * (M - 1) / M), ("stats_row", row[2].double().cpu() / M)):
        print(f"  stress {R.IDS[dt]} delta {delta} {what}: max |var - ref| / var "
              f"{((var - st['var']).abs() / st['var']).max().item():.3e}")
        within(var, st["var"], bound, what + " var")
    if delta == 0:  # (b) has mean 0: no relative bound
        rel(stats[0], st["mean"], 1e-5, "mean")
        rel(row[1], st["mean"], 1e-5, "row mean")
    assert torch.equal(row[0].cpu(), torch.full((C,), float(M)))
    within(1.0 / stats[1].double().cpu() ** 2 - 1e-5, st["var"], bound + 3 * E * (st["var"] + 1e-5), "invstd^-2 - eps")


@pytest.mark.parametrize("dt", [BF16, F16], ids=lambda d: R.IDS[d])
def test_bn_bwd_large_mean(dev, dt):
    """The (a) input through bn_bwd in 16 bits, whose partial sums centre once per thread
    (sum g' z - mu sum g'): dgamma (and the rest) still meet the ordinary bounds."""
    K = _k()
    z, _ = _stress(dt, 0)
    M, C = 3137, 64
    g = torch.Generator().manual_seed(9)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    gy = (0.3 + torch.randn(1, M, 1, C, generator=g)).to(dt)
    zA, gA, dzA = act_of(z, dev), act_of(gy, dev), act_of(z, dev, fill=SENT)
    stats = K.bn_fwd_train(zA, gam.to(dev), bet.to(dev), None, None, MOM, 1e-5)
    dgam, dbet, dbias = _f32(C, dev), _f32(C, dev), _f32(C, dev)
    K.bn_bwd(gA, zA, gam.to(dev), stats, 0, dzA, dgam, dbet, dbias)
    torch.cuda.synchronize()
    sd = stats.cpu()
    check_bwd(R.bwd(gy, z, gam, sd[0], sd[1], sd[2], sd[3], 0), dt, dzA.view(), dgam, dbet, dbias)


# ------------------------------------------------------------------------------ SyncBatchNorm -----
def _finalize_sync(K, loc, glob, Ml, Mg, gam, invstd, dev):
    C = loc.shape[1]
    out = [_f32(C, dev) for _ in range(3)]
    coef = torch.full((3, C), SENT, dtype=F32, device=dev)
    K.call("dg_bn_bwd_finalize_sync", K.ptr(loc), K.ptr(glob), Ml, Mg, C, K.ptr(gam), K.ptr(invstd), K.ptr(out[0]),
           K.ptr(out[1]), K.ptr(out[2]), K.ptr(coef), K.stream())
    return out, coef


def _sync_backward(dev, dt, i, stats, whole, parts, pooled, use_g):
    """The phases of the synchronised backward over `parts` (slices of the batch dimension or of the pixel
    rows) of one batch; whole: the float64 whole-batch backward with the kernels' statistics."""
    K, sb = _k(), _sb()
    z, act, C = i["z"], i["act"], i["z"].shape[-1]
    sd = stats.cpu()
    gam = i["gamma"].to(dev)
    cut = (lambda t, s: t[s]) if pooled else (lambda t, s: t[:, s])
    zs = [act_of(cut(z, s).contiguous(), dev) for s in parts]
    gs = [act_of(cut(i["g"], s).contiguous(), dev) if use_g else None for s in parts]
    gps = [act_of(i["gp"][s].contiguous(), dev) if pooled else None for s in parts]
    loc = [sb.bwd_sums(g, zA, stats, act, g_pool=gp) for g, zA, gp in zip(gs, zs, gps)]
    glob = loc[0] + loc[1]  # the all-reduce: an f32 add
    Mg = sum(zA.M for zA in zs)
    dzs = []
    for s, zA, g, gp, l in zip(parts, zs, gs, gps, loc):
        (dgam, dbet, dbias), coef = _finalize_sync(K, l, glob, zA.M, -1, gam, stats[1], dev)
        (dgam2, dbet2, dbias2), coef2 = _finalize_sync(K, l, glob, zA.M, Mg, gam, stats[1], dev)
        dzA = act_of(cut(z, s).contiguous(), dev, fill=SENT)
        sb.bwd_apply(g, zA, stats, act, coef, dzA, g_pool=gp)
        torch.cuda.synchronize()
        assert torch.equal(coef, coef2) and torch.equal(dbias, dbias2), "count from row 3 != explicit count"
        check_amax(dzA, "dz")
        dzs.append(dzA.buf.cpu())
        # this part's sums against float64 (the kernels' statistics)
        zp, HW = cut(z, s), i["HW"]
        gl = R.pool_route(i["gp"][s], i["g"][s] if use_g else None, cut(whole["y"], s)) if pooled else cut(i["g"], s)
        r4, a = R.sums4(gl, zp, sd[0], sd[1], sd[2], sd[3], act, None, HW)
        lc = l.double().cpu()
        for k, what in enumerate(("sum g'", "sum g' xhat", "sum xhat")):
            within(lc[k], r4[k], sum_bound(a[k], r4[k]), "local " + what)
        assert torch.equal(lc[3], r4[3]), "count row"
        # finalize_sync as the function of its stored sums
        f = R.finalize_sync(l, glob, zA.M, None, i["gamma"], sd[1])
        within(coef[0], f["k1"], E * f["k1"].abs(), "k1")
        within(coef[1], f["k2"], 2 * E * f["k2"].abs(), "k2")
        within(coef[2], f["k3"], 2 * E * f["k3"].abs(), "k3")
        assert torch.equal(dgam, l[1]) and torch.equal(dbet, l[0])
        within(dbias, f["dbias"], S * f["terms"] + E * f["dbias"].abs(), "dbias (stored sums)")
        # dgamma / dbeta / dbias against this part's float64 sums and the whole batch's coefficients
        within(dgam, r4[1], sum_bound(a[1], r4[1]), "local dgamma")
        within(dbet, r4[0], sum_bound(a[0], r4[0]), "local dbeta")
        wa, ws, k1 = whole["abs_sums"], whole["sums"], whole["k1"].abs()
        bk2 = k1 / Mg * (sum_bound(wa[1], ws[1]) + E * ws[1].abs()) + 2 * E * whole["k2"].abs()
        bk3 = k1 / Mg * (sum_bound(wa[0], ws[0]) + E * ws[0].abs()) + 2 * E * whole["k3"].abs()
        f64 = R.finalize_sync(r4, whole["sums4"], zA.M, None, i["gamma"], sd[1])
        within(dbias, f64["dbias"], S * f64["terms"] + k1 * sum_bound(a[0], r4[0]) + whole["k2"].abs() *
               sum_bound(a[2], r4[2]) + r4[2].abs() * bk2 + zA.M * bk3 + E * f64["dbias"].abs(), "local dbias")
    dz = torch.cat(dzs, 0 if pooled else 1)
    bound, _, _ = dz_bound(whole, dt, extra_sum_round=E)  # the global sums are rounded twice: per part, and added
    within(dz, whole["dz"], bound, "dz of the parts")


@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: R.IDS[d])
def test_syncbn_one_device(dev, dt):
    """Two 'ranks' = the first 65 and the last 3072 pixel rows of one 3137-pixel batch on one device."""
    K, sb = _k(), _sb()
    case = R.sync_case(dt)
    i = R.inputs(case)
    z, C = i["z"], case.C
    parts = [slice(0, 65), slice(65, 3137)]
    rows = []
    for s in parts:
        zA = act_of(z[:, s].contiguous(), dev)
        row = sb.row_from_z(zA)
        rows.append(sb.split_row(row, zA.M))
        r = R.row(z[:, s])
        rc = row.double().cpu()
        assert torch.equal(rc[0], r[0])
        rel(rc[1], r[1], 1e-5, "row mean")
        within(rc[2], r[2], sum_bound(r[2], r[2]), "row M2")
    rows = torch.cat(rows)
    rm, rv = i["rm0"].to(dev), i["rv0"].to(dev)
    stats = K.bn_part_finalize(rows, rows.shape[0], C, i["gamma"].to(dev), i["beta"].to(dev), rm, rv, MOM, i["eps"])
    torch.cuda.synchronize()
    check_stats(stats.cpu(), R.stats(z, i["gamma"], i["beta"], i["eps"]), rm, rv, i, "merged")
    sd = stats.cpu()
    whole = R.bwd(i["g"], z, i["gamma"], sd[0], sd[1], sd[2], sd[3], case.act)
    whole["sums4"] = R.sums4(i["g"], z, sd[0], sd[1], sd[2], sd[3], case.act)[0]
    _sync_backward(dev, dt, i, stats, whole, parts, False, True)


@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: R.IDS[d])
@pytest.mark.parametrize("use_g", [False, True], ids=["gpool", "gpool+g"])
def test_syncbn_pooled_one_device(dev, dt, use_g):
    """The synchronised backward through the pooled entries: 'ranks' of 1 and 2 images of 14x22."""
    K = _k()
    case = R.sync_pool_case(dt)
    i = R.inputs(case)
    z = i["z"]
    N, H, W, C = z.shape
    zA = act_of(z, dev)
    stats, _, _ = fwd_train(K, dev, zA, i)
    yA = act_of(z, dev, fill=SENT)
    K.bn_apply_pool(zA, stats, case.act, yA, K.Act(torch.empty((N, H // 2, W // 2, C), dtype=dt, device=dev)))
    torch.cuda.synchronize()
    sd, ys = stats.cpu(), yA.buf.cpu()
    gd = i["g"] if use_g else None
    whole = R.pool_bwd(i["gp"], gd, ys, z, i["gamma"], sd[0], sd[1], sd[2], sd[3], case.act)
    whole["y"] = ys
    whole["sums4"] = R.sums4(R.pool_route(i["gp"], gd, ys), z, sd[0], sd[1], sd[2], sd[3], case.act)[0]
    _sync_backward(dev, dt, i, stats, whole, [slice(0, 1), slice(1, 3)], True, use_g)
