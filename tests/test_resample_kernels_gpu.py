"""Kernel-level tests of resample.hip (the 2x2 max pool, the general k x k max pool and its argmax-recording
twin, the bilinear / nearest upsample with its C = 1 and x2 / x4 specialisations) against the float64
restatements of tests/resample_ref.py, per element: never against a whole-tensor maximum.  The references
take the stored inputs; tests/test_resample_ref_cpu.py pins them to ATen and asserts what the input makers
promise.  Channel c of every input is scaled by 2^((c mod 7) - 3), so small channels sit beside large ones.

Bounds (derived, not measured; e = 2^-24, u = 2^-8 bf16 / 2^-11 f16; resample_ref holds the functions).
  pool forward, nearest forward: bit-equal (NaN equal to NaN, -0 apart from +0); recorded indices equal.
  2x2 pool backward: bit-equal; with accumulate, the once-rounded f32 sum operand + gradient stored in T.
  general / idx pool backward: n e sum |terms| (n <= 4 windows + the accumulate operand), + u |ref| for
    16-bit storage (+ 2^-24 f16); the two forms bit-equal to each other.
  bilinear forward: 8 e sum |w x| (six roundings on a path: tap weight, two products and an add per row,
    the row product, the final add), then the storage term.
  bilinear backward: (n + 4) e sum |w g| (the weight product, an fma chain of n taps, the gy + gy2 add, the
    accumulate add, whose operand counts among the terms), then the storage term.  The separable C = 1
    backward has shorter chains than n and falls under the same bound.

Section d runs modes 0 / 1 / 2 x scales {1, 2, 3, 4, 8, 16} x (H, W) in {(1, 1), (1, 5), (5, 1), (2, 2), (6, 5)}
and 33 x 17 at scale 3 mode 1, at C = V and C = 1, less what resample_ref.up_shapes drops because it selects
the same kernel with the same branch outcomes as a shape that stays:
  nearest at scales 3 and 8      one rule (o // scale, never clamped) at every scale; 1, 2, 4 and 16 stay
  scale 8 at (1, 5), (5, 1), (2, 2)   the generic kernels at a power-of-two scale, as 16 at the same shapes
                                  and 8 at (1, 1) and (6, 5), which stay
  scale 1 at (1, 5), (5, 1)      the identity at every shape; (1, 1), (2, 2), (6, 5) stay
"""
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
SENT = -7777.0
dtypes = pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.IDS[d])


def _k():
    from dgvcc_amd import kernels as K
    return K


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
    """|out - ref| <= bound per element."""
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


def same(out, ref, what):
    """Bit-equal as values of the storage type: NaN equal to NaN, -0 apart from +0."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    no, nr = torch.isnan(out), torch.isnan(ref)
    bad = (no != nr) | (torch.where(no, torch.zeros_like(out), out).view(torch.int64)
                        != torch.where(nr, torch.zeros_like(ref), ref).view(torch.int64))
    print(f"  {what}: {int(bad.sum())} of {bad.numel()} elements differ")
    assert not bad.any(), (what, "first difference at %s" % (tuple(torch.nonzero(bad)[0].tolist()),))


def act_of(t, dev, sliced=False, fill=None):
    """t [N, H, W, C] on the device as an Act; sliced: channels [V, V + C) of a buffer whose width is C rounded
    up to V, + 2 V (off and ld multiples of V), every other channel SENT.  fill: an output buffer of t's
    extent holding that value instead of t."""
    K = _k()
    N, H, W, C = t.shape
    V = R.VEC[t.dtype]
    if not sliced:
        return K.Act(t.to(dev).contiguous() if fill is None else torch.full((N, H, W, C), fill, dtype=t.dtype, device=dev))
    buf = torch.full((N, H, W, -(-C // V) * V + 2 * V), SENT, dtype=t.dtype, device=dev)
    buf[..., V:V + C] = t.to(dev) if fill is None else fill
    return K.Act(buf, off=V, C=C)


def out_like(shape, dt, dev, sliced, fill=SENT):
    return act_of(torch.empty(shape, dtype=dt), dev, sliced, fill=fill)


def neighbours_intact(a, what):
    if a.buf.shape[3] == a.C:
        return
    rest = torch.cat([a.buf[..., :a.off], a.buf[..., a.off + a.C:]], -1)
    assert torch.equal(rest, torch.full_like(rest, SENT)), (what, "neighbouring channels written")


# ------------------------------------------------------------------------------ runners ----------
def run_pool(dev, dt, x, gy, acc, k, st, pad, sliced, forms=("gen", "idx")):
    """Forward and backward (without and with the accumulate operand) of the named pool forms against the
    reference; returns {form: (y, gx, gx_acc)} as device tensors."""
    K = _k()
    N, H, W, C = x.shape
    y_ref, arg = R.pool(x, k, st, pad)
    P, Q = y_ref.shape[1:3]
    b0 = R.pool_bwd(arg, gy, k, st, pad, H, W)
    b1 = R.pool_bwd(arg, gy, k, st, pad, H, W, acc=acc) if acc is not None else None
    xA, gyA = act_of(x, dev, sliced), act_of(gy, dev, sliced)
    outs = {}
    for form in forms:
        yA = out_like((N, P, Q, C), dt, dev, sliced)
        gxA = out_like((N, H, W, C), dt, dev, sliced)
        gxaA = act_of(acc, dev, sliced) if acc is not None else None
        if form == "two":
            K.maxpool_fwd(xA, yA)
            K.maxpool_bwd(xA, gyA, gxA)
            if acc is not None:
                K.maxpool_bwd(xA, gyA, gxaA, accumulate=True)
        elif form == "gen":
            K.maxpool_k_fwd(xA, k, st, pad, yA)
            K.maxpool_k_bwd(xA, gyA, k, st, pad, gxA)
            if acc is not None:
                K.maxpool_k_bwd(xA, gyA, k, st, pad, gxaA, accumulate=True)
        else:
            idx = K.maxpool_k_fwd_idx(xA, k, st, pad, yA)
            K.maxpool_k_bwd_idx(idx, gyA, k, st, pad, gxA)
            if acc is not None:
                K.maxpool_k_bwd_idx(idx, gyA, k, st, pad, gxaA, accumulate=True)
            torch.cuda.synchronize()
            assert idx.dtype == torch.uint8 and torch.equal(idx.cpu().long(), arg), (form, "recorded argmax")
        torch.cuda.synchronize()
        what = f"{form} k{k}s{st}p{pad} {H}x{W} {R.IDS[dt]}"
        same(yA.view(), y_ref, what + " y")
        if form == "two":
            same(gxA.view(), b0["gx"], what + " gx")
        else:
            within(gxA.view(), b0["gx"], R.pool_bwd_bound(b0, dt), what + " gx")
        if acc is not None:
            if form == "two":   # one window per pixel: the f32 sum of two stored values, rounded once, stored
                once = (acc.float() + b0["gx"].float()).to(dt)
                same(gxaA.view(), once, what + " gx (accumulate)")
            else:
                within(gxaA.view(), b1["gx"], R.pool_bwd_bound(b1, dt), what + " gx (accumulate)")
        for a, w in ((yA, "y"), (gxA, "gx"), (gxaA, "gx (accumulate)")):
            if a is not None:
                neighbours_intact(a, what + " " + w)
        outs[form] = (yA.view(), gxA.view(), gxaA.view() if gxaA is not None else None)
    if "gen" in outs and "idx" in outs:   # the same sums in the same order
        for a, b in zip(outs["gen"], outs["idx"]):
            if a is not None:
                same(a, b, "gen against idx")
    return outs


def run_up(dev, dt, x, gy, s, mode, sliced, gy2=None, acc=None, what=""):
    """upsample_fwd of x and upsample_bwd of gy (+ gy2, + the accumulate operand) against the reference."""
    K = _k()
    N, H, W, C = x.shape
    what = f"{what} x{s} mode {mode} {H}x{W} C {C} {R.IDS[dt]}"
    f = R.up_fwd(x, s, mode)
    b = R.up_bwd(gy, s, mode, gy2=gy2, acc=acc)
    yA = out_like((N, H * s, W * s, C), dt, dev, sliced)
    K.upsample_fwd(act_of(x, dev, sliced), s, mode, yA)
    gxA = act_of(acc, dev, sliced) if acc is not None else out_like((N, H, W, C), dt, dev, sliced)
    K.upsample_bwd(act_of(gy, dev, sliced), s, mode, gxA, gy2=None if gy2 is None else act_of(gy2, dev, sliced),
                   accumulate=acc is not None)
    torch.cuda.synchronize()
    if mode == 2:
        same(yA.view(), f["y"], what + " y")
    else:
        within(yA.view(), f["y"], R.up_fwd_bound(f, dt), what + " y")
    within(gxA.view(), b["gx"], R.up_bwd_bound(b, dt), what + " gx")
    neighbours_intact(yA, what + " y")
    neighbours_intact(gxA, what + " gx")
    return yA.view(), gxA.view()


def up_inputs(N, H, W, C, s, dt, seed, gy2=False, acc=False):
    x, gy = R.values((N, H, W, C), dt, seed), R.values((N, H * s, W * s, C), dt, seed + 1)
    return (x, gy, R.values((N, H * s, W * s, C), dt, seed + 2) if gy2 else None,
            R.values((N, H, W, C), dt, seed + 3) if acc else None)


# ------------------------------------------------------------------------------ a. slices --------
@dtypes
@pytest.mark.parametrize("nv", [1, 3])
def test_slices_pool(dev, dt, nv):
    """Every pool entry point on channels [V, V + C) of wider buffers, C = V and 3 V: values, and the guard
    channels of every written buffer bit-unchanged."""
    C = nv * R.VEC[dt]
    x = R.tied((2, 12, 10, C), dt, 21)
    gy, acc = R.values((2, 6, 5, C), dt, 22), R.values((2, 12, 10, C), dt, 23)
    run_pool(dev, dt, x, gy, acc, 2, 2, 0, True, forms=("two", "gen", "idx"))
    x = R.tied((2, 11, 9, C), dt, 24)
    gy, acc = R.values((2, 6, 5, C), dt, 25), R.values((2, 11, 9, C), dt, 26)
    run_pool(dev, dt, x, gy, acc, 3, 2, 1, True)


UP_KERNELS = ((0, 2), (0, 4), (1, 2), (0, 3), (2, 4))   # bl<2>, bl<4>, generic (three modes)


@dtypes
@pytest.mark.parametrize("mode,s", UP_KERNELS)
@pytest.mark.parametrize("C", ["V", "3V", 1, 3, 12])
def test_slices_upsample(dev, dt, mode, s, C):
    """upsample_fwd / upsample_bwd on channel slices: the vector kernels at C = V and 3 V, the scalar ones at
    C = 1, 3 and 12 (12 is a vector case at f32), the C = 1 backward kernel on strided maps."""
    C = {"V": R.VEC[dt], "3V": 3 * R.VEC[dt]}.get(C, C)
    x, gy, _, _ = up_inputs(2, 6, 5, C, s, dt, 31)
    run_up(dev, dt, x, gy, s, mode, True, what="sliced")


# ------------------------------------------------------------------------------ b. accumulate ----
@dtypes
def test_pool_accumulate(dev, dt):
    """accumulate=True on maxpool_bwd, maxpool_k_bwd and maxpool_k_bwd_idx, dense, on values that are no small
    integers (two channel vectors; the overlapping k3/s1/p1 windows give up to nine terms and the operand)."""
    C = 2 * R.VEC[dt]
    for k, st, pad, H, W, forms in ((2, 2, 0, 12, 10, ("two", "gen", "idx")), (3, 2, 1, 11, 9, ("gen", "idx")),
                                    (3, 1, 1, 7, 6, ("gen", "idx"))):
        x = R.values((2, H, W, C), dt, 45)
        P, Q = R.pool_out(H, k, st, pad), R.pool_out(W, k, st, pad)
        run_pool(dev, dt, x, R.values((2, P, Q, C), dt, 46), R.values((2, H, W, C), dt, 47), k, st, pad, False, forms=forms)


@dtypes
@pytest.mark.parametrize("mode,s", UP_KERNELS)
@pytest.mark.parametrize("second", [False, True], ids=["gy", "gy+gy2"])
@pytest.mark.parametrize("C", ["V", 3])
def test_upsample_accumulate(dev, dt, mode, s, second, C):
    """accumulate=True, with and without gy2: bl<2>, bl<4>, the generic vector kernel in its three modes, and the
    scalar kernel (C = 3).  (The pool kernels' accumulate runs in every pool test of this file.)"""
    C = R.VEC[dt] if C == "V" else C
    x, gy, gy2, acc = up_inputs(2, 6, 5, C, s, dt, 41, gy2=second, acc=True)
    run_up(dev, dt, x, gy, s, mode, False, gy2=gy2, acc=acc, what="accumulate")
    if second:   # gy2 without accumulate
        run_up(dev, dt, x, gy, s, mode, False, gy2=gy2, what="gy2")


# ------------------------------------------------------------------------------ c. pool rules ----
@dtypes
@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "k%ds%dp%d_%dx%d" % c)
def test_pool_rules(dev, dt, case):
    """First max in scan order, NaN propagates, -inf padding: the planted windows (all equal, a tie at each
    position, +-0, one and two NaNs, all -inf, +inf) through the general pool and its idx twin, without and
    with accumulate; k2/s2/p0 also through the 2x2 kernels, which must agree with it bit for bit; k3/s3/p0
    on 7 x 8 leaves the last row and column in no window (gradient 0, or the accumulate operand)."""
    k, st, pad, H, W = case
    x, gy, acc, _ = R.pool_case(k, st, pad, H, W, dt)
    two = (k, st, pad) == (2, 2, 0)
    outs = run_pool(dev, dt, x, gy, acc, k, st, pad, False, forms=("two", "gen", "idx") if two else ("gen", "idx"))
    if two:
        for a, b in zip(outs["two"], outs["gen"]):
            same(a, b, "2x2 kernels against the general pool at k2/s2/p0")
    if (k, st, pad) == (3, 3, 0):
        y, gx, gxa = outs["gen"]
        assert not gx[:, 6].any() and not gx[:, :, 6:].any()
        accd = acc.to(gx.device)
        assert torch.equal(gxa[:, 6], accd[:, 6]) and torch.equal(gxa[:, :, 6:], accd[:, :, 6:])


# ------------------------------------------------------------------------------ d. shapes --------
@dtypes
@pytest.mark.parametrize("mode,s,H,W", R.up_shapes())
def test_upsample_shapes(dev, dt, mode, s, H, W):
    """Border and degenerate shapes (one row, one column, one pixel), every scale and mode, at C = V and at
    C = 1 (dense: the C = 1 forward kernel where the output width is a multiple of 4, the separable backward)."""
    for C in (R.VEC[dt], 1):
        x, gy, _, _ = up_inputs(2, H, W, C, s, dt, 51)
        run_up(dev, dt, x, gy, s, mode, False, what="shape")


# ------------------------------------------------------------------------------ e. C = 1 limits --
C1_CASES = [  # N, H, W, scale, mode
    (1, 3, 300, 32, 0),      # the input-column tile halved to 128
    (1, 3, 300, 40, 0),      # 3 * 40 + 8 = 128 rows of weights: the last scale on the LDS kernel
    (1, 3, 300, 41, 0),      # the first on the per-pixel kernel
    (13107, 5, 2, 2, 0), (13107, 5, 2, 2, 1),   # N H = 65535: the last grid the LDS kernel takes
    (16384, 4, 2, 2, 0), (16384, 4, 2, 2, 1),   # N H = 65536: the per-pixel kernel
    (2, 2, 5, 16, 1),        # rh = 31
]


@dtypes
@pytest.mark.parametrize("N,H,W,s,mode", C1_CASES)
def test_c1_limits(dev, dt, N, H, W, s, mode, monkeypatch):
    """The limits of upsample_bwd_c1_kernel, each also with the C = 1 kernels switched off: both forms meet
    the bound against the reference (with a second gradient and the accumulate operand)."""
    x, gy, gy2, acc = up_inputs(N, H, W, 1, s, dt, 61, gy2=True, acc=True)
    run_up(dev, dt, x, gy, s, mode, False, gy2=gy2, acc=acc, what="c1")
    monkeypatch.setenv("DGVCC_UP_C1_OFF", "1")
    run_up(dev, dt, x, gy, s, mode, False, gy2=gy2, acc=acc, what="c1 off")


# ------------------------------------------------------------------------------ f. grid stride ---
# More than 16384 blocks x 256 threads of work items, + a ragged tail: every loop takes a second trip.  Small
# integers at power-of-two scales: every sum is exact in float32, the reference runs in float32 (gather form)
# and the comparison is equality.
def _eq(out, ref, what):
    out, ref = out.float().cpu(), ref.float()
    bad = out != ref
    print(f"  {what}: {int(bad.sum())} of {bad.numel()} elements differ")
    assert not bad.any(), (what, "first difference at %s" % (tuple(torch.nonzero(bad)[0].tolist()),))


def test_grid_stride_pool2(dev):
    K = _k()
    x, gy = R.ints((1, 4098, 4098, 4), F32, 71), R.ints((1, 2049, 2049, 4), F32, 72)
    y_ref, arg = R.pool(x, 2, 2, 0, work=F32)
    gx_ref = R.pool_bwd(arg, gy, 2, 2, 0, 4098, 4098, work=F32)["gx"]
    xA, yA, gxA = act_of(x, dev), out_like(y_ref.shape, F32, dev, False), out_like(x.shape, F32, dev, False)
    K.maxpool_fwd(xA, yA)
    K.maxpool_bwd(xA, act_of(gy, dev), gxA)
    torch.cuda.synchronize()
    _eq(yA.buf, y_ref, "maxpool_fwd_kernel, 2049^2 work items")
    _eq(gxA.buf, gx_ref, "maxpool_bwd_kernel, 2049^2 work items")


def test_grid_stride_pool_k_fwd(dev):
    K = _k()
    x = R.ints((1, 4097, 4097, 4), F32, 73)
    y_ref, arg = R.pool(x, 3, 2, 1, work=F32)
    xA, yA, y2A = act_of(x, dev), out_like(y_ref.shape, F32, dev, False), out_like(y_ref.shape, F32, dev, False)
    K.maxpool_k_fwd(xA, 3, 2, 1, yA)
    idx = K.maxpool_k_fwd_idx(xA, 3, 2, 1, y2A)
    torch.cuda.synchronize()
    _eq(yA.buf, y_ref, "maxpool_gen_fwd, 2049^2 work items")
    _eq(y2A.buf, y_ref, "maxpool_idx_fwd, 2049^2 work items")
    assert torch.equal(idx.cpu(), arg.to(torch.uint8))


def test_grid_stride_pool_k_bwd(dev):
    K = _k()
    x, gy = R.ints((1, 2049, 2049, 4), F32, 74), R.ints((1, 1025, 1025, 4), F32, 75)
    y_ref, arg = R.pool(x, 3, 2, 1, work=F32)
    gx_ref = R.pool_bwd(arg, gy, 3, 2, 1, 2049, 2049, work=F32)["gx"]
    xA, gyA = act_of(x, dev), act_of(gy, dev)
    gxA, gx2A = out_like(x.shape, F32, dev, False), out_like(x.shape, F32, dev, False)
    K.maxpool_k_bwd(xA, gyA, 3, 2, 1, gxA)
    idx = K.maxpool_k_fwd_idx(xA, 3, 2, 1, out_like(y_ref.shape, F32, dev, False))
    K.maxpool_k_bwd_idx(idx, gyA, 3, 2, 1, gx2A)
    torch.cuda.synchronize()
    _eq(gxA.buf, gx_ref, "maxpool_gen_bwd, 2049^2 work items")
    _eq(gx2A.buf, gx_ref, "maxpool_idx_bwd, 2049^2 work items")


@pytest.mark.parametrize("name,dt,C,H,s,mode", [
    ("upsample_fwd_kernel<V>", F32, 4, 1025, 2, 0),
    ("upsample_fwd_c1_kernel", F16, 1, 1025, 4, 0),
    ("upsample_fwd_kernel<1>", F16, 1, 1025, 2, 0),   # output width 2050, no multiple of 4: not the C = 1 kernel
])
def test_grid_stride_upsample_fwd(dev, name, dt, C, H, s, mode):
    K = _k()
    x = R.ints((1, H, H, C), dt, 76)
    y_ref = R.up_fwd(x, s, mode, work=F32, want_abs=False)["y"]
    yA = out_like(y_ref.shape, dt, dev, False)
    K.upsample_fwd(act_of(x, dev), s, mode, yA)
    torch.cuda.synchronize()
    _eq(yA.buf, y_ref, f"{name}, {y_ref.numel() // (4 if name != 'upsample_fwd_kernel<1>' else 1)} work items")


@pytest.mark.parametrize("name,C,H,s,mode", [
    ("upsample_bwd_bl_kernel<2>", 4, 2049, 2, 0),
    ("upsample_bwd_bl_kernel<4>", 4, 2049, 4, 0),
    ("upsample_bwd_kernel<V>", 4, 2049, 2, 2),
    ("upsample_bwd_kernel<1>", 3, 1183, 2, 0),
])
def test_grid_stride_upsample_bwd(dev, name, C, H, s, mode):
    K = _k()
    if s == 4:   # 8196^2 x 4 gradients: a 683^2 block of random integers, tiled 12 x 12 (cheaper to make)
        gy = R.ints((1, 683, 683, C), F32, 77).repeat(1, 12, 12, 1)
    else:
        gy = R.ints((1, H * s, H * s, C), F32, 77)
    gx_ref = R.up_bwd(gy, s, mode, work=F32, want_abs=False)["gx"]
    gxA = out_like(gx_ref.shape, F32, dev, False)
    K.upsample_bwd(act_of(gy, dev), s, mode, gxA)
    torch.cuda.synchronize()
    _eq(gxA.buf, gx_ref, f"{name}, {H * H * (C // 4 if C % 4 == 0 else C)} work items")


# ------------------------------------------------------------------------------ g. refusals ------
def _refused(fn, outs, what):
    """fn raises DGError on the host: nothing is launched, the output buffers stay bit-unchanged."""
    K = _k()
    before = [o.clone() for o in outs]
    with pytest.raises(K.DGError):
        fn()
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o, b), (what, "an output buffer changed")


@dtypes
def test_refusals(dev, dt):
    K = _k()
    V = R.VEC[dt]

    def A(N, H, W, C):
        return out_like((N, H, W, C), dt, dev, False)

    # the 2x2 pool: odd H, odd W, C no multiple of V
    for H, W, C in ((5, 4, V), (4, 5, V), (4, 4, V + 1), (4, 4, V // 2)):
        x, y, gy, gx = A(1, H, W, C), A(1, H // 2, W // 2, C), A(1, H // 2, W // 2, C), A(1, H, W, C)
        _refused(lambda: K.maxpool_fwd(x, y), [y.buf], "maxpool_fwd")
        _refused(lambda: K.maxpool_bwd(x, gy, gx), [gx.buf], "maxpool_bwd")
    # k > 15 on the idx pool
    x, y = A(1, 16, 16, V), A(1, 1, 1, V)
    idx = torch.zeros(1, 1, 1, V, dtype=torch.uint8, device=dev)
    _refused(lambda: K.maxpool_k_fwd_idx(x, 16, 16, 0, y), [y.buf], "k 16 idx fwd")
    _refused(lambda: K.maxpool_k_bwd_idx(idx, y, 16, 16, 0, x), [x.buf], "k 16 idx bwd")
    # 2 pad > k; a window that does not fit the padded map (H + 2 pad < k)
    for k, st, pad, H, W in ((3, 2, 2, 6, 6), (5, 1, 1, 2, 6), (5, 1, 1, 6, 2)):
        x, gx = A(1, H, W, V), A(1, H, W, V)
        y = A(1, max(1, (H + 2 * pad - k) // st + 1), max(1, (W + 2 * pad - k) // st + 1), V)   # what C division gives
        idx = torch.zeros(y.buf.shape, dtype=torch.uint8, device=dev)
        _refused(lambda: K.maxpool_k_fwd(x, k, st, pad, y), [y.buf], "k fwd")
        _refused(lambda: K.maxpool_k_bwd(x, y, k, st, pad, gx), [gx.buf], "k bwd")
        _refused(lambda: K.maxpool_k_fwd_idx(x, k, st, pad, y), [y.buf], "k fwd idx")
        _refused(lambda: K.maxpool_k_bwd_idx(idx, y, k, st, pad, gx), [gx.buf], "k bwd idx")
        # the C entry points themselves
        from dgvcc_amd._capi import call, ptr, stream
        cx = (x.dt, x.ptr, x.ld, 1, H, W, V, k, st, pad)
        _refused(lambda: call("dg_maxpool_fwd", *cx, y.ptr, y.ld, stream()), [y.buf], "dg_maxpool_fwd")
        _refused(lambda: call("dg_maxpool_bwd", x.dt, x.ptr, x.ld, y.ptr, y.ld, 1, H, W, V, k, st, pad, gx.ptr, gx.ld,
                              0, stream()), [gx.buf], "dg_maxpool_bwd")
        _refused(lambda: call("dg_maxpool_fwd_idx", *cx, y.ptr, y.ld, ptr(idx), stream()), [y.buf, idx],
                 "dg_maxpool_fwd_idx")
        _refused(lambda: call("dg_maxpool_bwd_idx", x.dt, ptr(idx), y.ptr, y.ld, 1, H, W, V, k, st, pad, gx.ptr, gx.ld,
                              0, stream()), [gx.buf], "dg_maxpool_bwd_idx")
    # the wrappers' extent guards: k3/s2/p1 on 7 x 6 gives 4 x 3
    x, gx = A(2, 7, 6, V), A(2, 7, 6, V)
    good = A(2, 4, 3, V)
    gidx = torch.zeros(2, 4, 3, V, dtype=torch.uint8, device=dev)
    for bad in (A(2, 3, 3, V), A(2, 5, 3, V), A(2, 4, 4, V), A(1, 4, 3, V), A(2, 4, 3, 2 * V)):
        _refused(lambda: K.maxpool_k_fwd(x, 3, 2, 1, bad), [bad.buf], "y extent")
        _refused(lambda: K.maxpool_k_fwd_idx(x, 3, 2, 1, bad), [bad.buf], "y extent (idx)")
        _refused(lambda: K.maxpool_k_bwd(x, bad, 3, 2, 1, gx), [gx.buf], "gy extent")
        _refused(lambda: K.maxpool_k_bwd_idx(gidx, bad, 3, 2, 1, gx), [gx.buf], "gy extent (idx)")
    for bad in (A(2, 7, 7, V), A(2, 8, 6, V), A(3, 7, 6, V), A(2, 7, 6, 2 * V)):
        _refused(lambda: K.maxpool_k_bwd(x, good, 3, 2, 1, bad), [bad.buf], "gx extent")
    for bad in (torch.zeros(2, 4, 3, 2 * V, dtype=torch.uint8, device=dev), torch.zeros(2, 3, 3, V, dtype=torch.uint8, device=dev),
                torch.zeros(2, 4, 3, V, dtype=torch.int32, device=dev), torch.zeros(2, 4, 3, V, dtype=torch.uint8),
                torch.zeros(2, 4, 3, 2 * V, dtype=torch.uint8, device=dev)[..., ::2]):
        _refused(lambda: K.maxpool_k_bwd_idx(bad, good, 3, 2, 1, gx), [gx.buf], "idx")
