"""Kernel-level tests of the first layer (stem.hip: dg_stem_fwd_f32, dg_stem_fwd, dg_stem_stats, dg_stem_apply,
dg_stem_bwd_coef, dg_stem_bwd_f32, dg_stem_bwd with stored and with recomputed z) and of the part-row machinery it
shares with the conv epilogue statistics and SyncBatchNorm (dg_bn_part_finalize, its bn_part_merge first stage,
dg_bn_part_row), against the float64 restatements of tests/stem_ref.py and tests/bn_ref.py: per element and per
channel, never against a whole-tensor maximum.  The references take the stored inputs and the kernels' own stored
f32 rows, so each kernel is judged as the function it implements; tests/test_stem_ref_cpu.py asserts the input
conditions (planted borders, ReLU margin, part counts) on the references alone.

Shapes: (1,1,64) one segment, three idle waves; (3,2,64) both halo rows in one window, three images; (2,3,128),
(1,5,192) an odd number of segments per row; (2,3,32), (1,4,96), (1,2,160) widths only the backward accepts;
(2,33,4096): 4224 forward segments (2 or 3 per wave in the statistics passes, 1 or 2 in dg_stem_apply), 8448
backward segments (4 or 5 per wave: both exits of the register ping-pong), an image boundary mid-grid.

Bounds (derived, not measured; e = 2^-24, S = 512 e; helpers of tests/test_bn_kernels_gpu.py).
  z, f32: 32 e sum|terms| + e |ref|: 27 FMAs and the bias add in any order.  bf16: the same on the bf16-rounded
    operands + one bf16 ulp 2^-8 |ref| (the MFMA's internal order is not documented; any order is covered).
  part rows: n equal to the launch rule's count exactly; the zero-filter channel M2 = 0 exactly in every row.
    Merged M2: the larger of S M2 + e M2 (M2 is its own sum of absolute terms) and 1e-5 (1 + d^2) M2, the rule of
    the BN stress tests for sums shifted by a pixel d deviations from the mean (the planted corner is pixel 0 of
    every case), + 12 e |mean| sqrt(n M2): a row's mean is kept in f32, so each of the at most 6 roundings of it
    (the wave's own mean, 4 wave merges, the stored row) moves the between-row terms sum n_b (mean_b - mean)^2
    by at most 2 e |mean| sum n_b |mean_b - mean| <= 2 e |mean| sqrt(n M2); relative to M2 that is
    12 e |mean| / std: nothing for an ordinary channel, 1e-2 for the bias-100 channel in f32.
  mean (merged and finalized): 1e-5 max(|ref|, std) per channel, which is 1e-5 |ref| wherever |mean| >= std.  A
    mean is a sum and its rounding is relative to its terms: the zero-bias channel at (3,2,64) has mean -0.026
    against std 5.8, where the rounding of 64 f32 terms of that size alone (~ e std sqrt(64) = 3e-6) is 1e-4
    |mean|, so no f32 summation meets 1e-5 |mean| there.  shift = beta - mean scale and the running mean carry it.
  other finalized statistics: 1e-5 |ref| per channel, or where it is larger M2's own bound above carried by the
    derivative (invstd: half the variance's relative bound; the sum bound S alone allows 1.5e-5); the bias-100 channel (|mean| / std ~ 10^4 in f32) by the rule of
    the BN stress tests, variance within 1e-5 (1 + d^2) var, d the distance of the stored first pixel from the
    mean in deviations, + the 12 e |mean| / std of the f32 row means, carried to invstd, scale, shift and the
    running variance by their derivatives.
  y: the y bound of the BN tests.  Backward sums and coefficients: the sum / coefficient bounds of the BN tests
    (g is read as exact bf16: nothing is stored in 16 bits there).
  dw, f32: S sum|dz x| + e |ref| per element of the 64 x 27.  The longest f32 chain at these shapes: 5 segments
    x 32 pixels = 160 pixels per wave in the MFMA accumulators, + 4 waves, + 32 slab rows, + 8 reduce groups and
    2 slab-stage rows = 206 < 512.  bf16: + 2^-8 sum|dz x| for dz's bf16 store (the image taps are read as
    bf16: the reference takes the rounded image).  accumulate: + e |old + ref|.
  uncertain ReLU elements (|z scale + shift| <= 2^-23 (|z scale| + |shift|) in float64): sums and dw widened by
    their own absolute contribution.
  part rows as inputs: n exact, mean 1e-5 |ref|, M2 (S + e) M2, + 160 e M2 for the f32 first stage when
    nblk > 1024 (20 Chan merges of 8 roundings); var = 1 / invstd^2 - eps carries M2's bound.
"""
import pytest
import torch

import bn_ref as R
import stem_ref as SR
from test_bn_kernels_gpu import (E, MOM, S, SENT, _end_run_on_device_fault, act_of, neighbours_intact,  # noqa: F401
                                 rel, stored, sum_bound, within, y_bound)

pytestmark = pytest.mark.gpu

F32, BF16 = R.F32, R.BF16
IDS = R.IDS
NAN = float("nan")
SHAPE_ID = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


def _k():
    from dgvcc_amd import kernels as K
    return K


def _row(v, dev):
    return torch.full((64,), float(v), dtype=F32, device=dev)


class Stem:
    """Device operands of one (shape, dtype) case."""

    def __init__(self, dev, shape, dt):
        K = _k()
        self.dev, self.shape, self.dt = dev, shape, dt
        self.i = i = SR.make_case(*shape)
        self.img = i["img"].to(dev)
        self.w = K.stem_weight_f32(i["w"].to(dev)) if dt == F32 else K.pack_weight(i["w"].to(dev), BF16, cpad=3, row_len=32)
        self.bias = i["bias"].to(dev)
        self.gamma, self.beta = i["gamma"].to(dev), i["beta"].to(dev)
        self.img_r = SR.rounded(i["img"], dt)
        self.g = i["g"].to(dt)  # the stored upstream gradient

    def z_act(self, wide=False, fill=NAN):
        N, H, W = self.shape
        if not wide:
            return _k().Act(torch.full((N, H, W, 64), fill, dtype=self.dt, device=self.dev))
        buf = torch.full((N, H, W, 80), SENT, dtype=self.dt, device=self.dev)
        buf[..., 8:72] = fill
        return _k().Act(buf, off=8, C=64)

    def fwd(self, use_bias=True, wide=False):
        K = _k()
        zA = self.z_act(wide)
        f = K.stem_fwd_f32 if self.dt == F32 else K.stem_fwd
        part, rows = f(self.img, self.w, self.bias if use_bias else None, zA)
        return zA, part, rows

    def finalize(self, part, rows):
        rm, rv = self.i["rm0"].to(self.dev), self.i["rv0"].to(self.dev)
        stats = _k().bn_part_finalize(part, rows, 64, self.gamma, self.beta, rm, rv, MOM, self.i["eps"])
        return stats, rm, rv


# ------------------------------------------------------------------------------ forward: z --------
def check_z(c, zA, use_bias, what):
    ref, a = SR.with_bias(c.shape, c.dt, use_bias)
    within(zA.view(), ref, stored(32 * E * a, ref, c.dt) + (E * ref.abs() if c.dt == F32 else 0.0), what)
    neighbours_intact(zA, what)


@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SR.FWD_SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: IDS[d])
def test_stem_fwd_z(dev, dt, shape, use_bias):
    """dg_stem_fwd_f32 / dg_stem_fwd: every z (prefilled with NaN) against the float64 convolution."""
    c = Stem(dev, shape, dt)
    zA, _, _ = c.fwd(use_bias)
    torch.cuda.synchronize()
    check_z(c, zA, use_bias, f"z {IDS[dt]}")


@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: IDS[d])
def test_stem_fwd_channel_slice(dev, dt):
    """z as channels [8, 72) of an 80-channel buffer (ldz = 80): the neighbours keep their sentinel."""
    c = Stem(dev, (2, 3, 128), dt)
    zA, part, rows = c.fwd(True, wide=True)
    zB, part2, _ = c.fwd(True)
    torch.cuda.synchronize()
    check_z(c, zA, True, "z slice")
    assert torch.equal(zA.view(), zB.view()) and torch.equal(part, part2), "slice != contiguous"


def test_stem_fwd_equals_im2col_gemm(dev):
    """The fused bf16 forward stores the bits of the im2col + K = 64 GEMM route."""
    K = _k()
    c = Stem(dev, (2, 3, 128), BF16)
    zA, _, _ = c.fwd()
    col = K.Act(K.im2col_c3(c.img, BF16))
    z0 = c.z_act()
    K.conv_fwd(col, K.pack_weight(c.i["w"].to(dev), BF16, cpad=3, row_len=64), 64, 1, 0, z0, bias=c.bias)
    torch.cuda.synchronize()
    assert torch.equal(zA.buf, z0.buf), "stem z differs from the im2col GEMM"


# ------------------------------------------------------------------------------ forward: statistics
def delta_of(zs):
    """Distance of the stored first pixel from the channel mean in deviations (0 for a constant channel)."""
    x = zs.double().reshape(-1, 64)
    sd = x.std(0, unbiased=False)
    return torch.where(sd > 0, (x[0] - x.mean(0)).abs() / sd.clamp_min(1e-300), torch.zeros_like(sd))


def mean_grain(zs):
    """12 e |mean| / std per channel (0 for a constant channel): the relative effect on M2 of keeping the row
    means in f32, see the module docstring."""
    x = zs.double().reshape(-1, 64)
    sd = x.std(0, unbiased=False)
    return torch.where(sd > 0, 12 * E * x.mean(0).abs() / sd.clamp_min(1e-300), torch.zeros_like(sd))


def relm2_of(zs):
    """Relative bound of M2 (and of the variance) per channel: the larger of S + e and 1e-5 (1 + d^2), + the
    12 e |mean| / std of the f32 row means (see the module docstring)."""
    d = delta_of(zs)
    return torch.maximum(torch.full_like(d, S + E), 1e-5 * (1.0 + d * d)) + mean_grain(zs)


def mean_bound(zs):
    """1e-5 max(|mean|, std) per channel: 1e-5 |ref| wherever |mean| >= std (see the module docstring)."""
    x = zs.double().reshape(-1, 64)
    return 1e-5 * torch.maximum(x.mean(0).abs(), x.std(0, unbiased=False))


def check_parts(part, zs, shape, what):
    p = part.double().cpu()
    counts = SR.part_counts(*shape)
    assert p.shape == (counts.numel(), 3, 64), (what, p.shape)
    assert torch.equal(p[:, 0, :], counts[:, None].expand(-1, 64)), (what, "part counts")
    assert not p[:, 2, SR.CH_ZERO].any(), (what, "M2 of the constant channel")
    m, r = R.merge(p), R.row(zs)
    assert torch.equal(m[0], r[0]), (what, "merged n")
    within(m[1], r[1], mean_bound(zs), what + " merged mean")
    within(m[2], r[2], relm2_of(zs) * r[2], what + " merged M2")


def check_stem_stats(sd, rm, rv, zs, i, what):
    """The finalized rows against R.stats of the stored z: 1e-5 |ref|; the bias-100 channel by the variance rule."""
    st = R.stats(zs, i["gamma"], i["beta"], i["eps"])
    relv = relm2_of(zs)
    b = {k: 1e-5 * st[k].abs() for k in ("mean", "invstd", "scale", "shift")}
    b["mean"] = mean_bound(zs)
    frac = st["var"] / (st["var"] + i["eps"])
    b["invstd"] = torch.maximum(b["invstd"], (0.5 * relv * frac + 4 * E) * st["invstd"])
    b["scale"] = torch.maximum(b["scale"], b["invstd"] * i["gamma"].abs().double() + 2 * E * st["scale"].abs())
    b["shift"] = torch.maximum(b["shift"], st["mean"].abs() * b["scale"] + b["mean"] * st["scale"].abs()
                               + 4 * E * st["shift"].abs())
    for k, row in zip(("mean", "invstd", "scale", "shift"), sd):
        within(row, st[k], b[k], f"{what} {k}")
    rmr = R.running(i["rm0"], st["mean"], MOM)
    within(rm, rmr, torch.maximum(1e-5 * rmr.abs(), MOM * b["mean"] + 4 * E * (i["rm0"].double().abs() + st["mean"].abs())),
           what + " running_mean")
    rvr = R.running(i["rv0"], st["unbiased"], MOM)
    bv = torch.maximum(1e-5 * rvr.abs(), MOM * relv * st["unbiased"] + 4 * E * rvr.abs())
    within(rv, rvr, bv, what + " running_var")
    z0 = SR.CH_ZERO  # variance 0: invstd = 1 / sqrt(eps) to one ulp
    ref0 = 1.0 / torch.tensor(i["eps"], dtype=F32).double().sqrt()
    assert st["var"][z0] == 0 and abs(sd[1][z0].double().item() - ref0.item()) <= 2.0 ** -23 * ref0.item(), what


@pytest.mark.parametrize("shape", SR.FWD_SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: IDS[d])
def test_stem_statistics(dev, dt, shape):
    """The part rows of both forwards (and of dg_stem_stats, bit-equal to dg_stem_fwd's) and their finalized
    statistics against the stored z."""
    K = _k()
    c = Stem(dev, shape, dt)
    zA, part, rows = c.fwd()
    stats, rm, rv = c.finalize(part, rows)
    part1 = K.stem_stats(c.img, c.w, c.bias)[0] if dt == BF16 else None
    torch.cuda.synchronize()
    zs = zA.buf.cpu()
    check_parts(part, zs, shape, f"{IDS[dt]} fwd")
    if part1 is not None:
        assert torch.equal(part1, part), "dg_stem_stats rows != dg_stem_fwd rows"
    check_stem_stats(stats.cpu(), rm, rv, zs, c.i, f"{IDS[dt]} stats")


# ------------------------------------------------------------------------------ dg_stem_apply -----
@pytest.mark.parametrize("shape,bpc", [((1, 1, 64), None), (SR.LONG, None), (SR.LONG, "2")], ids=SHAPE_ID)
def test_stem_apply(dev, shape, bpc, monkeypatch):
    """y with z recomputed: the bits of dg_bn_apply on the stored z, and per element against float64."""
    K = _k()
    if bpc:
        monkeypatch.setenv("DGVCC_STEM_APPLY_BPC", bpc)
    c = Stem(dev, shape, BF16)
    zA, part, rows = c.fwd()
    stats, _, _ = c.finalize(part, rows)
    y0, y1 = c.z_act(fill=SENT), c.z_act(wide=True, fill=SENT)
    K.bn_apply(zA, stats, 1, y0)
    K.stem_apply(c.img, c.w, c.bias, stats, y1)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(), y0.buf), "dg_stem_apply != dg_stem_fwd + dg_bn_apply"
    neighbours_intact(y1, "y")
    sd, zs = stats.cpu(), zA.buf.cpu()
    yr = R.apply(zs, sd[2], sd[3], 1)
    within(y1.view(), yr, y_bound(zs, sd[2], sd[3], yr, BF16), "y")


# ------------------------------------------------------------------------------ dg_stem_bwd_coef --
def unc_sums(g, zs, sd):
    """(sum |g|, sum |g xhat|) per channel over the uncertain elements (None when there are none)."""
    u = SR.uncertain(zs, sd[2], sd[3])
    ok, n, total = SR.margin_ok(zs, sd[2], sd[3])
    assert ok, ("ReLU margin on the stored values", n, total)
    if not u.any():
        return None
    ga = g.double().reshape(-1, 64).abs() * u
    return ga.sum(0), (ga * R.xhat(zs, sd[0], sd[1]).abs()).sum(0)


def check_coef(s, a, M, gamma, sd, coef, dgam, dbet, dbias, extra, what):
    x0, x1 = extra if extra is not None else (0.0, 0.0)
    k1 = gamma.double() * sd[1].double()
    k2, k3 = k1 * s[1] / M, k1 * s[0] / M
    bs0, bs1 = sum_bound(a[0], s[0]) + x0, sum_bound(a[1], s[1]) + x1
    bk2 = k1.abs() / M * bs1 + 2 * E * k2.abs()
    bk3 = k1.abs() / M * bs0 + 2 * E * k3.abs()
    within(coef[0], k1, E * k1.abs(), what + " k1")
    within(coef[1], k2, bk2, what + " k2")
    within(coef[2], k3, bk3, what + " k3")
    within(dgam, s[1], bs1, what + " dgamma")
    within(dbet, s[0], bs0, what + " dbeta")
    within(dbias, -k2 * s[2], S * k2.abs() * a[2] + s[2].abs() * bk2 + E * (k2 * s[2]).abs(), what + " dbias")


@pytest.mark.parametrize("shape", [(3, 2, 64), SR.LONG], ids=SHAPE_ID)
def test_stem_bwd_coef(dev, shape):
    """Mode 3 (z recomputed): the coefficient rows, dgamma, dbeta, dbias per channel against float64 on the
    stored z, g and statistics rows."""
    K = _k()
    c = Stem(dev, shape, BF16)
    zA, part, rows = c.fwd()
    stats, _, _ = c.finalize(part, rows)
    gA = act_of(c.g, dev, sliced=True)
    dgam, dbet, dbias = (_row(SENT, dev) for _ in range(3))
    coef = K.stem_bwd_coef(c.img, c.w, c.bias, gA, c.gamma, stats, dgam, dbet, dbias)
    torch.cuda.synchronize()
    sd, zs = stats.cpu(), zA.buf.cpu()
    s, a = R.sums3(c.g, zs, sd[0], sd[1], sd[2], sd[3], 1)
    check_coef(s, a, zA.M, c.i["gamma"], sd, coef.cpu(), dgam, dbet, dbias, unc_sums(c.g, zs, sd), "coef")


# ------------------------------------------------------------------------------ backward: dw ------
def dw_bound(dt, ref, terms, extra=None, old=None):
    b = S * terms + E * ref.abs()
    if dt == BF16:
        b = b + 2.0 ** -8 * terms
    if extra is not None:
        b = b + extra
    if old is not None:
        b = b + E * (ref + old).abs()
    return b


class Bwd:
    """One backward case on the device: stored z (the forward kernel's where W % 64 == 0, else the float64
    convolution rounded to the storage type), statistics and coefficients of the generic BN entries."""

    def __init__(self, dev, shape, dt, sliced=False):
        K = _k()
        self.c = c = Stem(dev, shape, dt)
        self.dt, self.dev = dt, dev
        if shape[2] % 64 == 0:
            self.zs = c.fwd()[0].buf.cpu()
        else:
            self.zs = SR.stored_z(shape, dt)
        self.zA, self.gA = act_of(self.zs, dev, sliced), act_of(c.g, dev, sliced)
        self.stats = K.bn_fwd_train(self.zA, c.gamma, c.beta, None, None, MOM, c.i["eps"])
        self.coef = K.bn_bwd_coef(self.gA, self.zA, c.gamma, self.stats, 1, _row(0, dev), _row(0, dev), _row(0, dev))
        self._ref = None

    def run(self, kind, dw=None, accumulate=False, stats=None, coef=None, gA=None):
        K, c = _k(), self.c
        stats, coef = self.stats if stats is None else stats, self.coef if coef is None else coef
        gA = self.gA if gA is None else gA
        dw = torch.full((64, 3, 3, 3), NAN, device=self.dev) if dw is None else dw
        if kind == "f32":
            K.stem_bwd_f32(c.img, gA, self.zA, stats, coef, dw, accumulate)
        elif kind == "stored":
            K.stem_bwd(c.img, gA, self.zA, stats, coef, dw, accumulate)
        else:
            K.stem_bwd(c.img, gA, None, stats, coef, dw, accumulate, wp=c.w, bias=c.bias)
        return dw

    def kinds(self):
        if self.dt == F32:
            return ["f32"]
        return ["stored", "zfree"] if self.c.shape[2] % 64 == 0 else ["stored"]

    def ref(self):
        """(dw, sum |dz x|, the uncertain elements' contribution) in float64 from the stored inputs and the
        stored statistics and coefficient rows."""
        if self._ref is None:
            c = self.c
            sd, cf = self.stats.cpu(), self.coef.cpu()
            dz, _ = R.apply_coef(c.g, self.zs, sd[0], sd[1], sd[2], sd[3], 1, cf[0], cf[1], cf[2])
            dw, terms = SR.wgrad(c.img_r, dz)
            ok, n, total = SR.margin_ok(self.zs, sd[2], sd[3])
            assert ok, ("ReLU margin on the stored values", n, total)
            u = SR.uncertain(self.zs, sd[2], sd[3])
            extra = None
            if u.any():
                ku = (cf[0].double() * c.g.double().reshape(-1, 64)).abs() * u
                extra = SR.wgrad(c.img_r.abs(), ku.reshape(dz.shape))[1]
            self._ref = (dw, terms, extra)
        return self._ref


@pytest.mark.parametrize("shape", SR.BWD_SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: IDS[d])
def test_stem_bwd_dw(dev, dt, shape):
    """dw of dg_stem_bwd_f32 / dg_stem_bwd (stored z, and z-free where W % 64 == 0), all 64 x 27 elements; the
    stored-z and z-free kernels given the same rows agree bit for bit."""
    b = Bwd(dev, shape, dt)
    out = {k: b.run(k) for k in b.kinds()}
    torch.cuda.synchronize()
    ref, terms, extra = b.ref()
    for k, dw in out.items():
        within(dw, ref, dw_bound(dt, ref, terms, extra), f"dw {k}")
    if "zfree" in out:
        assert torch.equal(out["zfree"], out["stored"]), "z-free dw != stored-z dw"


@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: IDS[d])
def test_stem_bwd_accumulate_and_slices(dev, dt):
    """accumulate = 1 onto a non-zero dw; g and z as channel slices of wider buffers (ldg, ldz > 64)."""
    shape = (2, 3, 128)
    b, bs = Bwd(dev, shape, dt), Bwd(dev, shape, dt, sliced=True)
    old = torch.randn(64, 3, 3, 3, generator=torch.Generator().manual_seed(4)) * 50.0
    acc = {k: b.run(k, dw=old.to(dev), accumulate=True) for k in b.kinds()}
    sl = {k: bs.run(k) for k in bs.kinds()}
    plain = {k: b.run(k) for k in b.kinds()}
    torch.cuda.synchronize()
    ref, terms, extra = b.ref()
    for k in b.kinds():
        within(acc[k], ref + old.double(), dw_bound(dt, ref, terms, extra, old.double()), f"dw {k} accumulate")
        assert torch.equal(sl[k], plain[k]), f"dw {k}: slices != contiguous"


# ------------------------------------------------------------------------------ one segment -------
def _long_bwd_segments():
    N, H, W = SR.LONG
    nseg, spr = N * H * (W // 32), W // 32
    w0 = SR.wave_segments(nseg, 0, 0)          # five slots
    w4 = SR.wave_segments(nseg, 75, 0)         # a wave with four
    assert len(w0) == 5 and len(w4) == 4
    per_img = H * spr
    return sorted({0, nseg - 1, *w0, w4[-1], per_img - 1, per_img, 10 * spr, 11 * spr - 1})


def _long_fwd_segments():
    N, H, W = SR.LONG
    nseg, spr = N * H * (W // 64), W // 64
    w0 = SR.wave_segments(nseg, 0, 0)          # three slots
    w2 = SR.wave_segments(nseg, 75, 0)         # a wave with two
    assert len(w0) == 3 and len(w2) == 2
    per_img = H * spr
    return sorted({0, nseg - 1, *w0, w2[-1], per_img - 1, per_img, 10 * spr, 11 * spr - 1})


def _synthetic_rows(dev):
    """scale 1, shift 1000 (every element active, far from zero), mean 0, invstd 1 (xhat = z); k1 1, k2 k3 0."""
    stats = torch.stack([_row(0, dev), _row(1, dev), _row(1, dev), _row(1000, dev)])
    coef = torch.stack([_row(1, dev), _row(0, dev), _row(0, dev)])
    return stats, coef


@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: IDS[d])
def test_stem_bwd_one_segment(dev, dt):
    """g non-zero on the 32 pixels of one backward segment of the long shape, coefficients (1, 0, 0): dw is that
    segment's contribution alone, so a lost, doubled or misplaced segment shows in every element (in bf16 too,
    where the whole-tensor 2^-8 term is larger than one segment's share)."""
    K = _k()
    N, H, W = SR.LONG
    c = Stem(dev, SR.LONG, dt)
    b = Bwd.__new__(Bwd)
    b.c, b.dt, b.dev = c, dt, dev
    b.zA = c.fwd()[0]
    stats, coef = _synthetic_rows(dev)
    gbuf = torch.zeros(N, H, W, 64, dtype=dt, device=dev)
    gA, gflat = K.Act(gbuf), gbuf.view(-1, 64)
    grows = c.g.reshape(-1, 64)
    for seg in _long_bwd_segments():
        pix = SR.segment_pixels(N, H, W, seg, 32)
        gflat[pix.to(dev)] = grows[pix].to(dev)
        out = {k: b.run(k, stats=stats, coef=coef, gA=gA) for k in b.kinds()}
        gflat[pix.to(dev)] = 0
        torch.cuda.synchronize()
        ref, terms = SR.wgrad_pixels(c.img_r, pix, grows[pix])
        for k, dw in out.items():
            within(dw, ref, dw_bound(dt, ref, terms), f"segment {seg} dw {k}")


def test_stem_bwd_coef_one_segment(dev):
    """Mode 3 with g non-zero on one 64-pixel forward segment of the long shape: sum g' (dbeta) and sum g' xhat
    (dgamma, xhat = z under the synthetic rows) are that segment's alone."""
    K = _k()
    N, H, W = SR.LONG
    c = Stem(dev, SR.LONG, BF16)
    zs = c.fwd()[0].buf.cpu().double().reshape(-1, 64)
    stats, _ = _synthetic_rows(dev)
    ones = _row(1, dev)
    gbuf = torch.zeros(N, H, W, 64, dtype=BF16, device=dev)
    gA, gflat = K.Act(gbuf), gbuf.view(-1, 64)
    grows = c.g.reshape(-1, 64)
    for seg in _long_fwd_segments():
        pix = SR.segment_pixels(N, H, W, seg, 64)
        gflat[pix.to(dev)] = grows[pix].to(dev)
        dgam, dbet, dbias = (_row(SENT, dev) for _ in range(3))
        K.stem_bwd_coef(c.img, c.w, c.bias, gA, ones, stats, dgam, dbet, dbias)
        gflat[pix.to(dev)] = 0
        torch.cuda.synchronize()
        gd, zd = grows[pix].double(), zs[pix]
        within(dbet, gd.sum(0), sum_bound(gd.abs().sum(0), gd.sum(0)), f"segment {seg} sum g'")
        within(dgam, (gd * zd).sum(0), sum_bound((gd * zd).abs().sum(0), (gd * zd).sum(0)), f"segment {seg} sum g' xhat")


# ------------------------------------------------------------------------------ part rows ---------
def make_rows(nblk, C, seed, empty=False):
    """Seeded (n, mean, M2) rows [nblk][3][C] (f32) of random pixel groups of 1 .. 16 pixels, channel c centred at
    +-5 with deviation 3 (what R.row gives per group); empty: a third of the rows (the first, the last and,
    where there is one, the whole second group of 64 among them) hold n = 0 with NaN mean and M2."""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, 17, (nblk,), generator=g)
    gid = torch.repeat_interleave(torch.arange(nblk), sizes)
    sgn = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    x = sgn * 5.0 + 3.0 * torch.randn(int(sizes.sum()), C, generator=g, dtype=torch.float64)
    n = sizes.double()[:, None].expand(-1, C)
    mean = torch.zeros(nblk, C, dtype=torch.float64).index_add_(0, gid, x) / n
    m2 = torch.zeros(nblk, C, dtype=torch.float64).index_add_(0, gid, (x - mean[gid]) ** 2)
    rows = torch.stack([n, mean, m2], 1).float()
    k = nblk // 2
    assert torch.allclose(rows[k].double(), R.row(x[gid == k]), rtol=1e-6, atol=1e-6)
    if empty:
        z = torch.rand(nblk, generator=g) < 0.3
        z[0] = z[-1] = True
        if nblk > 128:
            z[64:128] = True
        if z.all():
            z[nblk // 2] = False
        rows[z, 0] = 0.0
        rows[z, 1:] = NAN
    return rows


def run_part_rows(dev, nblk, C, empty):
    K = _k()
    rows = make_rows(nblk, C, 31 * nblk + C, empty)
    g = torch.Generator().manual_seed(nblk + C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    part = rows.to(dev)
    keep = part.clone()
    rm, rv = rm0.to(dev), rv0.to(dev)
    eps = 1e-5
    stats = K.bn_part_finalize(part, nblk, C, gamma.to(dev), beta.to(dev), rm, rv, MOM, eps)
    out = torch.full((3, C), SENT, dtype=F32, device=dev)
    work = torch.empty(K.query("dg_bn_part_workspace", nblk, C) // 4 + 1, dtype=F32, device=dev)
    K.call("dg_bn_part_row", K.ptr(part), nblk, C, K.ptr(out), K.ptr(work), K.stream())
    torch.cuda.synchronize()
    assert torch.equal(part.view(torch.int32), keep.view(torch.int32)), "input rows modified"
    live = rows[rows[:, 0, 0] > 0]
    m = R.merge(live)
    M = m[0]
    chain = 160 * E if nblk > 1024 else 0.0
    bm2 = (S + E + chain) * m[2]
    what = f"nblk {nblk} C {C}"
    o = out.double().cpu()
    assert torch.equal(o[0], M), (what, "row n")
    rel(o[1], m[1], 1e-5, what + " row mean")
    within(o[2], m[2], bm2, what + " row M2")
    st = R.stats_from_rows(live, gamma, beta, eps)
    sd = stats.double().cpu()
    eps32 = torch.tensor(eps, dtype=F32).double()
    rel(sd[0], st["mean"], 1e-5, what + " mean")
    var = m[2] / M
    within(1.0 / sd[1] ** 2 - eps32, var, bm2 / M + 3 * E * (var + eps32), what + " invstd^-2 - eps")
    # scale, shift and the running rows as functions of the stored mean / invstd
    within(sd[2], gamma.double() * sd[1], E * (gamma.double() * sd[1]).abs(), what + " scale")
    ms = sd[0] * sd[2]
    within(sd[3], beta.double() - ms, E * ms.abs() + E * (beta.double() - ms).abs(), what + " shift")
    rmr = R.running(rm0, sd[0], MOM)
    within(rm, rmr, 3 * E * (rm0.double().abs() + sd[0].abs()), what + " running_mean")
    unb = var * M / (M - 1) if float(M[0]) > 1 else var
    rvr = R.running(rv0, unb, MOM)
    within(rv, rvr, MOM * bm2 / (M - 1).clamp_min(1) + 3 * E * (rv0.double().abs() + unb.abs()), what + " running_var")


@pytest.mark.parametrize("nblk", [1, 3, 256, 1024, 1025, 1088, 2500])
@pytest.mark.parametrize("C", [64, 70, 256])
def test_part_rows(dev, C, nblk):
    """dg_bn_part_finalize and dg_bn_part_row as functions of their rows: 1025 leaves a merge group of one row,
    C = 70 a partly filled second channel block of bn_part_merge."""
    run_part_rows(dev, nblk, C, False)


@pytest.mark.parametrize("nblk", [3, 256, 1088, 2500])
def test_part_rows_with_empty_rows(dev, nblk):
    """A third of the rows with n = 0 and NaN mean / M2 (the first, a whole group of 64, the last): not read."""
    run_part_rows(dev, nblk, 70, True)


# ------------------------------------------------------------------------------ guards ------------
def test_stem_rejected_shapes(dev):
    """W = 96 in the entries that walk 64-pixel segments, W = 48 in the backwards, ldz = 60: DGError and the
    sentinel-filled outputs untouched."""
    K = _k()
    DGError, p, s = K.DGError, K.ptr, K.stream()
    g = torch.Generator().manual_seed(2)

    def bufs(W, ld=64):
        N, H = 1, 2
        img = torch.randn(N, 3, H, W, generator=g).to(dev)
        return (N, H, W), img, {dt: torch.full((N, H, W, ld), SENT, dtype=dt, device=dev) for dt in (F32, BF16)}

    w = torch.randn(64, 3, 3, 3, generator=g).to(dev)
    wk, wp = K.stem_weight_f32(w), K.pack_weight(w, BF16, cpad=3, row_len=32)
    rows = torch.full((8, 3, 64), SENT, dtype=F32, device=dev)
    ones = torch.ones(4, 64, dtype=F32, device=dev)
    dw = torch.full((64, 3, 3, 3), SENT, dtype=F32, device=dev)
    work = torch.full((1 << 16,), SENT, dtype=F32, device=dev)
    ws = work.numel() * 4

    def rejected(name, *args):
        with pytest.raises(DGError):
            K.call(name, *args)

    (N, H, W), img, z = bufs(96)
    rejected("dg_stem_fwd", p(img), N, H, W, p(wp), None, p(z[BF16]), 64, p(rows), s)
    rejected("dg_stem_fwd_f32", p(img), N, H, W, p(wk), None, p(z[F32]), 64, p(rows), s)
    rejected("dg_stem_stats", p(img), N, H, W, p(wp), None, p(rows), s)
    rejected("dg_stem_apply", p(img), N, H, W, p(wp), None, p(ones[0]), p(ones[1]), p(z[BF16]), 64, s)
    rejected("dg_stem_bwd_coef", p(img), N, H, W, p(wp), None, p(z[BF16]), 64, p(ones[0]), p(ones[0]), p(ones[1]),
             p(ones[2]), p(ones[3]), p(rows[0]), p(rows[1, 0]), p(rows[1, 1]), p(rows[1, 2]), p(rows[2]), s)
    (N, H, W), img48, z48 = bufs(48)
    rejected("dg_stem_bwd_f32", p(img48), N, H, W, p(z48[F32]), 64, p(z48[F32]), 64, p(ones[0]), p(ones[1]),
             p(ones[2]), p(ones[3]), p(ones), p(dw), p(work), ws, 0, s)
    for zp, wpk in ((p(z48[BF16]), None), (None, p(wp))):
        rejected("dg_stem_bwd", p(img48), N, H, W, p(z48[BF16]), 64, zp, 64, p(ones[0]), p(ones[1]), p(ones[2]),
                 p(ones[3]), p(ones), p(dw), p(work), ws, 0, wpk, None, s)
    (N, H, W), img64, z60 = bufs(64, ld=60)
    rejected("dg_stem_fwd", p(img64), N, H, W, p(wp), None, p(z60[BF16]), 60, p(rows), s)
    rejected("dg_stem_fwd_f32", p(img64), N, H, W, p(wk), None, p(z60[F32]), 60, p(rows), s)
    rejected("dg_stem_apply", p(img64), N, H, W, p(wp), None, p(ones[0]), p(ones[1]), p(z60[BF16]), 60, s)
    rejected("dg_stem_bwd_f32", p(img64), N, H, W, p(z60[F32]), 64, p(z60[F32]), 60, p(ones[0]), p(ones[1]),
             p(ones[2]), p(ones[3]), p(ones), p(dw), p(work), ws, 0, s)
    rejected("dg_stem_bwd", p(img64), N, H, W, p(z60[BF16]), 64, p(z60[BF16]), 60, p(ones[0]), p(ones[1]),
             p(ones[2]), p(ones[3]), p(ones), p(dw), p(work), ws, 0, None, None, s)
    torch.cuda.synchronize()
    for t in (rows, dw, work, *z.values(), *z48.values(), *z60.values()):
        assert torch.equal(t, torch.full_like(t, SENT)), "an output was written"
