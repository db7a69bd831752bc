"""The restatements of tests/resample_ref.py against ATen on the CPU, at every shape family the kernel tests of
tests/test_resample_kernels_gpu.py use (small sizes), and the conditions the input makers promise, so that a
failure there cannot be blamed on the reference or on its inputs.  No GPU.

  max pool   F.max_pool2d(..., return_indices=True) and its autograd, bit-equal, the planted non-finite and tie
             cases included (gradients are float32 values, so their float64 sums are exact in any order).
  upsample   F.interpolate in float64 (the operation: its taps are double, so it is compared to the precision
             of a float32 tap unless the taps are exact) and in float32, where ATen's own float32 arithmetic
             must meet the kernel tests' bounds (8 e sum |w x| forward, (n + 4) e sum |w g| backward) at every
             shape, and at the twelve shapes of UP_TABLE stays within 3.2 e sum |w x| and 3.2 e sum |w g|: an
             independent float32 implementation meets the bounds with room.  The 3.2 is a figure of the data,
             not a derived bound: ATen adds a backward's taps one by one in float32, and over forty seeds of
             these inputs the worst ratio of a seed lay between 2.85 and 5.4 (a third of them under 3.2; SEED
             is one of those); the derived bounds held for all.
"""
import pytest
import torch
import torch.nn.functional as F

import resample_ref as R

E = R.E
NAN = float("nan")


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def same(a, b):
    """Bit-equal, NaN equal to NaN, -0 different from +0."""
    a, b = a.double(), b.double()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(
        torch.where(na, torch.zeros_like(a), a).view(torch.int64), torch.where(nb, torch.zeros_like(b), b).view(torch.int64))


def _aten_pool(x, gy, k, st, pad):
    xr = _nchw(x.double()).requires_grad_(True)
    y, idx = F.max_pool2d(xr, k, st, pad, return_indices=True)
    y.backward(_nchw(gy.double()))
    return _nhwc(y.detach()), _nhwc(idx), _nhwc(xr.grad)


@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "k%ds%dp%d_%dx%d" % c)
def test_pool_against_aten(case):
    k, st, pad, H, W = case
    x, gy, acc, plants = R.pool_case(k, st, pad, H, W, R.F32)
    y, arg = R.pool(x, k, st, pad)
    ya, idx, gxa = _aten_pool(x, gy, k, st, pad)
    assert same(y, ya)
    assert torch.equal(R.pool_flat(arg, k, st, pad, W), idx)
    b = R.pool_bwd(arg, gy, k, st, pad, H, W)
    assert same(b["gx"], gxa)
    b2 = R.pool_bwd(arg, gy, k, st, pad, H, W, acc=acc)
    assert same(b2["gx"], gxa + acc.double())
    assert torch.equal(b2["n"], b["n"] + 1) and same(b2["abs"], b["abs"] + acc.double().abs())
    assert b["n"].max() <= 4 or st < (k + 1) // 2   # at most 4 windows per pixel when the stride is >= k / 2
    assert b["n"].sum() == arg.numel()


@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "k%ds%dp%d_%dx%d" % c)
def test_plants_are_what_they_say(case):
    k, st, pad, H, W = case
    x, gy, acc, plants = R.pool_case(k, st, pad, H, W, R.F32)
    y, arg = R.pool(x, k, st, pad)
    kinds = {p[0] for p in plants}
    assert kinds == set(R.PLANTS)
    seen_first = set()
    for kind, n, p, q, c in plants:
        inb = [r * k + s for r in range(k) for s in range(k)
               if 0 <= p * st - pad + r < H and 0 <= q * st - pad + s < W]
        win = [x[n, p * st - pad + o // k, q * st - pad + o % k, c].item() for o in inb]
        a, v = arg[n, p, q, c].item(), y[n, p, q, c].item()
        if kind == "all_equal":
            assert len(set(win)) == 1 and a == inb[0]
        elif kind == "zeros_neg_first":
            assert all(w == 0 for w in win) and a == inb[0] and str(v) == "-0.0"
        elif kind == "zeros_pos_first":
            assert all(w == 0 for w in win) and a == inb[0] and str(v) == "0.0"
        elif kind == "one_nan":
            assert sum(w != w for w in win) == 1 and v != v and a == inb[len(inb) // 2]
        elif kind == "two_nans":
            assert sum(w != w for w in win) == (2 if len(inb) > 1 else 1) and v != v and a == inb[-1]
        elif kind == "all_ninf":
            assert (x[..., c] == R.NINF).all() and (y[..., c] == R.NINF).all()
            first = R.pool(torch.zeros_like(x), k, st, pad)[1]     # all equal: the first in-bounds element
            assert torch.equal(arg[..., c], first[..., c])
        elif kind == "pos_inf":
            assert v == float("inf") and a == inb[len(inb) // 2]
        elif kind == "tie_at":
            assert win.count(max(win)) >= 1 and win[inb.index(a)] == max(win)
            assert all(w < max(win) for w in win[:inb.index(a)])
            seen_first.add(a)
    assert len(seen_first) >= 2 or H * W < 20 or k > 5, seen_first   # the planted first maximum moves through the window
    if k <= 3 and H * W >= 20:   # and with the tied values of the other channels it is found at every position
        assert set(arg.flatten().tolist()) == set(range(k * k))


def test_pool_rules_confirmed_on_aten():
    """Two NaNs: the later takes the gradient.  All -inf: the first in-bounds element.  k3/s2/p1 on a 3 x 3
    all -inf map: indices [0, 1, 3, 4]."""
    x = torch.tensor([[1.0, NAN], [NAN, 2.0]]).reshape(1, 2, 2, 1)
    y, arg = R.pool(x, 2, 2, 0)
    ya, idx, gxa = _aten_pool(x, torch.ones(1, 1, 1, 1), 2, 2, 0)
    assert arg.item() == 2 and idx.item() == 2 and gxa.flatten().tolist() == [0, 0, 1, 0]
    x = torch.full((1, 3, 3, 1), R.NINF)
    y, arg = R.pool(x, 3, 2, 1)
    ya, idx, _ = _aten_pool(x, torch.ones(1, 2, 2, 1), 3, 2, 1)
    assert R.pool_flat(arg, 3, 2, 1, 3).flatten().tolist() == [0, 1, 3, 4] == idx.flatten().tolist()
    assert (y == R.NINF).all() and (ya == R.NINF).all()


def test_pool_2x2_is_the_window_maximum():
    x, gy, acc, _ = R.pool_case(2, 2, 0, 4, 6, R.F32)
    y, arg = R.pool(x, 2, 2, 0)
    N, H, W, C = x.shape
    w = x.double().reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
    fin = ~torch.isnan(w).any(-1)
    assert torch.equal(y[fin], w.max(-1).values[fin])
    assert (arg >= 0).all() and (arg <= 3).all()


# ------------------------------------------------------------------------------ upsample ---------
UP_TABLE = [(6, 5, 2, 0), (6, 5, 4, 0), (3, 7, 16, 1), (1, 3, 2, 1), (9, 7, 2, 1), (5, 12, 8, 0), (7, 1, 4, 1),
            (4, 4, 4, 2), (1, 1, 4, 0), (1, 1, 4, 1), (33, 17, 3, 1), (2, 2, 16, 1)]
UP_ALL = sorted(set(UP_TABLE) | {(H, W, s, m) for m, s, H, W in R.up_shapes()})


SEED = 26


def _interp(x, s, mode):
    if mode == 2:
        return F.interpolate(x, scale_factor=s, mode="nearest")
    return F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=(mode == 1))


def _aten_up(x, gy, s, mode, dt):
    xr = _nchw(x.to(dt)).requires_grad_(True)
    y = _interp(xr, s, mode)
    y.backward(_nchw(gy.to(dt)))
    return _nhwc(y.detach()), _nhwc(xr.grad)


def _ratios(x, gy, s, mode, y32, gx32, fused):
    f, b = R.up_fwd(x, s, mode, fused=fused), R.up_bwd(gy, s, mode, fused=fused)
    ef, eb = (y32.double() - f["y"]).abs(), (gx32.double() - b["gx"]).abs()
    return f, b, ef, eb, (ef / (E * f["abs"]).clamp_min(1e-300)).max().item(), (eb / (E * b["abs"]).clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("H,W,s,mode", UP_ALL)
def test_upsample_against_aten(H, W, s, mode):
    N, C = 2, 3
    x, gy = R.values((N, H, W, C), R.F32, SEED), R.values((N, H * s, W * s, C), R.F32, SEED + 1)
    # float32 ATen: an independent float32 implementation against the restatement
    y32, gx32 = _aten_up(x, gy, s, mode, torch.float32)
    f, b, ef, eb, rf, rb = _ratios(x, gy, s, mode, y32, gx32, True)
    if mode == 0 and s & (s - 1) and rf > 8:
        # 1 / scale is inexact and this ATen build rounds r (o + 0.5) before it subtracts 0.5: judge it by that form
        f, b, ef, eb, rf, rb = _ratios(x, gy, s, mode, y32, gx32, False)
    print(f"  {H}x{W} x{s} mode {mode}: ATen f32 err / (e sum|w x|) fwd {rf:.2f} bwd {rb:.2f}")
    if mode == 2:
        assert torch.equal(y32.double(), f["y"]) and rf == 0
    if (H, W, s, mode) in UP_TABLE:
        assert (ef <= 3.2 * E * f["abs"]).all(), rf
        assert (eb <= 3.2 * E * b["abs"]).all(), rb
    assert (ef <= R.up_fwd_bound(f, R.F32)).all() and (eb <= R.up_bwd_bound(b, R.F32)).all()
    f, b = R.up_fwd(x, s, mode), R.up_bwd(gy, s, mode)
    # float64 ATen: the same operation (its taps are double: exact where ours are, else a float32 tap apart)
    y64, gx64 = _aten_up(x, gy, s, mode, torch.float64)
    exact = mode == 2 or (mode == 0 and s & (s - 1) == 0)
    tf = 1e-12 if exact else 2.0 ** -21 * max(H, W) * s
    assert ((y64 - f["y"]).abs() <= tf * x.abs().max()).all()
    assert ((gx64 - b["gx"]).abs() <= tf * b["abs"].clamp_min(1e-30) * (1 if exact else 4)).all()
    # the tap count: every output index has weight on one or two inputs, and weights sum to 1
    assert b["n"].min() >= 1
    ones = R.up_fwd(torch.ones(1, H, W, 1), s, mode)["y"]
    assert ((ones - 1).abs() <= 2 * E).all()


def test_upsample_gy2_and_accumulate():
    H, W, s, mode = 6, 5, 2, 0
    gy, gy2 = R.values((2, H * s, W * s, 3), R.F32, 5), R.values((2, H * s, W * s, 3), R.F32, 6)
    acc = R.values((2, H, W, 3), R.F32, 7)
    b = R.up_bwd(gy, s, mode, gy2=gy2, acc=acc)
    b0 = R.up_bwd((gy.double() + gy2.double()), s, mode)
    assert torch.equal(b["gx"], b0["gx"] + acc.double())
    assert torch.equal(b["abs"], b0["abs"] + acc.double().abs())
    assert torch.equal(b["n"], b0["n"])
    # scale 2, align_corners=False: 2 x 2 taps at a corner, 4 x 4 inside (rows 3, 4 | 4 ... 4 | 4, 3 -> 3 at the ends)
    n = R.tap_count(6, 2, 0)
    assert n.tolist() == [3, 4, 4, 4, 4, 3]


def test_float32_work_type_is_exact_on_integers():
    """The grid-stride cases run the restatement in float32 on small integers at power-of-two scales in
    mode 0 / 2: every product and partial sum is a multiple of 2^-6 below 2^24, so float32 loses nothing."""
    for s, mode in ((2, 0), (4, 0), (2, 2)):
        x, gy = R.ints((1, 9, 7, 4), R.F32, 1), R.ints((1, 9 * s, 7 * s, 4), R.F32, 2)
        assert torch.equal(R.up_fwd(x, s, mode, work=torch.float32, want_abs=False)["y"].double(), R.up_fwd(x, s, mode)["y"])
        assert torch.equal(R.up_bwd(gy, s, mode, work=torch.float32, want_abs=False)["gx"].double(),
                           R.up_bwd(gy, s, mode)["gx"])
    x = R.ints((1, 9, 7, 4), R.F32, 3)
    y32, a32 = R.pool(x, 3, 2, 1, work=torch.float32)
    y64, a64 = R.pool(x, 3, 2, 1)
    assert torch.equal(y32.double(), y64) and torch.equal(a32, a64)


def test_shape_list_covers_the_kernels():
    shapes = R.up_shapes()
    assert (1, 3, 33, 17) in shapes
    for m in (0, 1, 2):
        assert {s for mm, s, H, W in shapes if mm == m} >= {1, 2, 4, 16}
    assert len(shapes) <= 70
