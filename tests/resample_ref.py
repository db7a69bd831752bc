"""Float64 restatements of the resampling kernels of resample.hip (max pool, bilinear / nearest upsample) in
plain torch, NHWC, with the error-bound inputs (term counts, sums of absolute terms) the kernel tests need,
the bound functions both test files share, and the input makers.  tests/test_resample_ref_cpu.py pins these
to ATen on the CPU; tests/test_resample_kernels_gpu.py judges the kernels against them.

Max pool (k, stride, pad; -inf padding): scan (r, s) ascending; an element becomes the maximum if
`v > m or isnan(v)`, or if it is the first in-bounds element of its window.  The argmax is the in-window
offset r * k + s.  The backward sums, per input element, the gradients of the windows whose argmax it is.

Upsample (integer scale; mode 0 bilinear, 1 bilinear align_corners, 2 nearest): the per-axis taps
(i0, i1, l1) are formed in float32 as the kernels' src_tap and ATen do (mode 0: r = 1f / scale,
src = max(fma(r, o + 0.5f, -0.5f), 0); mode 1: r = (in - 1) / (out - 1), src = r o; mode 2: o // scale); the weights
are 1f - l1 and l1 in float32; everything after that (products, sums) is in the work type, float64 unless a
caller asks for float32 at a shape whose arithmetic is exact.  Forward and backward are gathers and
index_add_ along one axis at a time, never dense matrices.
"""
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
VEC = {F32: 4, BF16: 8, F16: 8}
E = 2.0 ** -24
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
NINF = float("-inf")


# ------------------------------------------------------------------------------ bounds -----------
def stored(bound, ref, dt):
    """The bound of a value stored once in dt from an f32 value with bound `bound`."""
    if dt == F32:
        return bound
    return bound + U[dt] * ref.abs() + (2.0 ** -24 if dt == F16 else 0.0)


def pool_bwd_bound(b, dt):
    """General / idx pool backward: a chain of n f32 adds (n <= 4 windows + the accumulate operand)."""
    return stored(b["n"] * E * b["abs"], b["gx"], dt)


def up_fwd_bound(f, dt):
    """Bilinear forward: six f32 roundings on a path (tap weight, two products and an add per row, the
    row product, the final add), taken as 8 e sum |w x|.  Nearest (mode 2) is exact."""
    return stored(8 * E * f["abs"], f["y"], dt)


def up_bwd_bound(b, dt):
    """Bilinear backward: the weight product, an fma chain of n taps, the gy + gy2 add and the accumulate
    add: (n + 4) e sum |w g| (the accumulate operand counts among the terms)."""
    return stored((b["n"] + 4) * E * b["abs"], b["gx"], dt)


# ------------------------------------------------------------------------------ max pool ---------
def pool_out(H, k, st, pad):
    return (H + 2 * pad - k) // st + 1


def pool(x, k, st, pad, work=torch.float64):
    """x [N, H, W, C] -> (y [N, P, Q, C] in `work`, arg int64 [N, P, Q, C] = r * k + s of the maximum)."""
    N, H, W, C = x.shape
    P, Q = pool_out(H, k, st, pad), pool_out(W, k, st, pad)
    xp = torch.full((N, H + 2 * pad, W + 2 * pad, C), NINF, dtype=work)
    xp[:, pad:pad + H, pad:pad + W] = x.to(work)
    inb = torch.zeros(H + 2 * pad, W + 2 * pad, dtype=torch.bool)
    inb[pad:pad + H, pad:pad + W] = True
    m = torch.full((N, P, Q, C), NINF, dtype=work)
    am = torch.full((N, P, Q, C), -1, dtype=torch.int64)
    for r in range(k):
        for s in range(k):
            hs, ws = slice(r, r + (P - 1) * st + 1, st), slice(s, s + (Q - 1) * st + 1, st)
            v, ok = xp[:, hs, ws], inb[hs, ws][None, :, :, None]
            take = ok & ((v > m) | torch.isnan(v) | (am < 0))
            m = torch.where(take, v, m)
            am = torch.where(take, torch.full_like(am, r * k + s), am)
    return m, am


def pool_flat(arg, k, st, pad, W):
    """The flat input index h * W + w of each window's maximum."""
    N, P, Q, C = arg.shape
    h = torch.arange(P)[None, :, None, None] * st - pad + arg // k
    w = torch.arange(Q)[None, None, :, None] * st - pad + arg % k
    return h * W + w


def pool_bwd(arg, gy, k, st, pad, H, W, acc=None, work=torch.float64):
    """gx [N, H, W, C] = (acc or 0) + sum of gy over the windows whose argmax is the pixel; n: the number
    of terms of each element (the accumulate operand among them), abs: the sum of their absolute values."""
    N, P, Q, C = arg.shape
    flat = pool_flat(arg, k, st, pad, W).reshape(N, P * Q, C)
    g = gy.to(work).reshape(N, P * Q, C)
    base = torch.zeros(N, H * W, C, dtype=work) if acc is None else acc.to(work).reshape(N, H * W, C).clone()
    gx = base.clone().scatter_add_(1, flat, g)
    ab = base.abs().scatter_add_(1, flat, g.abs())
    n = torch.full((N, H * W, C), 0.0 if acc is None else 1.0, dtype=work).scatter_add_(1, flat, torch.ones_like(g))
    return {"gx": gx.reshape(N, H, W, C), "n": n.reshape(N, H, W, C), "abs": ab.reshape(N, H, W, C)}


# ------------------------------------------------------------------------------ upsample ---------
def taps(n_in, scale, mode, fused=True):
    """(i0, i1 int64, l0, l1 float32) per output index of one axis, in float32 as src_tap / ATen.  fused=False:
    mode 0 with the product rounded before the subtraction, as a build without fma contraction has it (it
    differs only where 1 / scale is inexact; test_resample_ref_cpu accepts either of ATen)."""
    out = n_in * scale
    o = torch.arange(out)
    if mode == 2:
        i0 = (o // scale).clamp_max(n_in - 1)
        return i0, i0.clone(), torch.ones(out, dtype=F32), torch.zeros(out, dtype=F32)
    of = o.to(F32)
    if mode == 1:
        r = (torch.tensor(float(n_in - 1), dtype=F32) / torch.tensor(float(out - 1), dtype=F32)) if out > 1 \
            else torch.tensor(0.0, dtype=F32)
        src = r * of
    else:
        r = torch.tensor(1.0, dtype=F32) / torch.tensor(float(scale), dtype=F32)
        # one fused multiply-add, as src_tap writes it and as ATen's builds contract it: the double product of
        # two float32 values is exact, so rounding the double result once is the fused result
        src = (r.double() * (of.double() + 0.5) - 0.5).to(F32) if fused else r * (of + 0.5) - 0.5
        src = src.clamp_min(0.0)
    i0 = src.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(F32)
    l0 = torch.tensor(1.0, dtype=F32) - l1
    assert src.dtype == F32 and l0.dtype == F32
    return i0, i1, l0, l1


def _gather_axis(t, dim, tp, work):
    i0, i1, l0, l1 = tp
    shape = [1] * t.dim()
    shape[dim] = -1
    out = t.index_select(dim, i0) * l0.to(work).reshape(shape)
    if l1.any():
        out += t.index_select(dim, i1) * l1.to(work).reshape(shape)
    return out


def _scatter_axis(t, dim, tp, n_in, work):
    i0, i1, l0, l1 = tp
    shape = [1] * t.dim()
    shape[dim] = -1
    size = list(t.shape)
    size[dim] = n_in
    out = torch.zeros(size, dtype=work)
    out.index_add_(dim, i0, t * l0.to(work).reshape(shape))
    if l1.any():
        out.index_add_(dim, i1, t * l1.to(work).reshape(shape))
    return out


def up_fwd(x, scale, mode, work=torch.float64, want_abs=True, fused=True):
    """x [N, H, W, C] -> {"y": [N, H s, W s, C], "abs": sum |w x| per output element}."""
    N, H, W, C = x.shape
    th, tw = taps(H, scale, mode, fused), taps(W, scale, mode, fused)
    xw = x.to(work)
    out = {"y": _gather_axis(_gather_axis(xw, 1, th, work), 2, tw, work)}
    if want_abs:
        out["abs"] = _gather_axis(_gather_axis(xw.abs(), 1, th, work), 2, tw, work)  # the weights are >= 0
    return out


def tap_count(n_in, scale, mode):
    """Per input index of one axis, the number of output indices whose (merged) tap weight on it is not 0."""
    i0, i1, l0, l1 = taps(n_in, scale, mode)
    n = torch.zeros(n_in, dtype=torch.float64)
    n.index_add_(0, i0, (l0 != 0).double())
    n.index_add_(0, i1, ((l1 != 0) & ((i1 != i0) | (l0 == 0))).double())
    return n


def up_bwd(gy, scale, mode, gy2=None, acc=None, work=torch.float64, want_abs=True, fused=True):
    """gy [N, H s, W s, C] -> {"gx": (acc or 0) + the transpose of up_fwd applied to gy + gy2, "n": the
    number of non-zero-weight taps of each input element, "abs": sum |w g| (+ |acc|)}."""
    N, Ho, Wo, C = gy.shape
    H, W = Ho // scale, Wo // scale
    th, tw = taps(H, scale, mode, fused), taps(W, scale, mode, fused)
    g = gy.to(work) if gy2 is None else gy.to(work) + gy2.to(work)
    gx = _scatter_axis(_scatter_axis(g, 2, tw, W, work), 1, th, H, work)
    if acc is not None:
        gx += acc.to(work)
    out = {"gx": gx}
    if want_abs:
        ab = _scatter_axis(_scatter_axis(g.abs(), 2, tw, W, work), 1, th, H, work)
        if acc is not None:
            ab += acc.to(work).abs()
        out["abs"] = ab
        out["n"] = (tap_count(H, scale, mode)[:, None] * tap_count(W, scale, mode)[None, :])[None, :, :, None] \
            .expand(N, H, W, C)
    return out


# ------------------------------------------------------------------------------ inputs -----------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def chan_scale(C):
    """2^((c mod 7) - 3): small channels beside large ones."""
    return torch.tensor([2.0 ** ((c % 7) - 3) for c in range(C)])


def values(shape, dt, seed):
    """Normal values, channel c scaled by 2^((c mod 7) - 3), rounded to dt."""
    return (torch.randn(shape, generator=_gen(seed)) * chan_scale(shape[-1])).to(dt)


def tied(shape, dt, seed):
    """Small integers (many ties in every window) times the channel scale: exact in every type."""
    return (torch.randint(-3, 4, shape, generator=_gen(seed)).float() * chan_scale(shape[-1])).to(dt)


def ints(shape, dt, seed, lo=-4, hi=5):
    """Small integers for the shapes whose sums are exact in float32."""
    return torch.randint(lo, hi, shape, generator=_gen(seed), dtype=torch.int8).to(dt)


PLANTS = ("all_equal", "zeros_neg_first", "zeros_pos_first", "one_nan", "two_nans", "all_ninf", "pos_inf", "tie_at")


def plant(x, k, st, pad):
    """Plants the non-finite and tie cases into x [N, H, W, C >= 8] in place, channel c taking PLANTS[c % 8];
    returns the list of (kind, n, p, q, c) planted, for the CPU test to assert each is what it says.
      all_equal        every element of the window equal
      zeros_neg_first  -0 everywhere in the window, +0 at its last in-bounds element (-0 stays the maximum)
      zeros_pos_first  +0 first, -0 after it
      one_nan          one NaN in the middle of the window's in-bounds elements
      two_nans         two NaNs: the later one is the maximum
      all_ninf         the whole channel -inf: every window's maximum is its first in-bounds element
      pos_inf          +inf twice: the first one is the maximum
      tie_at           window i of the channel: low values, and the maximum value at in-window position
                       (i mod k^2) and at every position after it, so the first maximum sits at each of
                       the k^2 positions in turn (where that position is in bounds)
    """
    N, H, W, C = x.shape
    P, Q = pool_out(H, k, st, pad), pool_out(W, k, st, pad)
    done = []

    def cells(p, q):
        return [(r * k + s, p * st - pad + r, q * st - pad + s) for r in range(k) for s in range(k)
                if 0 <= p * st - pad + r < H and 0 <= q * st - pad + s < W]

    for c in range(C):
        kind = PLANTS[c % 8]
        big = 8.0 * 2.0 ** ((c % 7) - 3)
        if kind == "all_ninf":
            x[..., c] = NINF
            done.append((kind, 0, 0, 0, c))
            continue
        if kind == "tie_at":
            i = 0
            for n in range(N):
                for p in range(0, P, max(1, -(-k // st))):      # windows that do not overlap
                    for q in range(0, Q, max(1, -(-k // st))):
                        j = i % (k * k)
                        for o, h, w in cells(p, q):
                            x[n, h, w, c] = big if o >= j else -big
                        i += 1
                        done.append((kind, n, p, q, c))
            continue
        n, p, q = c % N, (c // 2) % P, (c // 3) % Q
        cl = cells(p, q)
        for j, (o, h, w) in enumerate(cl):
            if kind == "all_equal":
                x[n, h, w, c] = big
            elif kind == "zeros_neg_first":
                x[n, h, w, c] = 0.0 if j == len(cl) - 1 and j > 0 else -0.0
            elif kind == "zeros_pos_first":
                x[n, h, w, c] = 0.0 if j == 0 else -0.0
            elif kind == "one_nan":
                x[n, h, w, c] = float("nan") if j == len(cl) // 2 else -big
            elif kind == "two_nans":
                x[n, h, w, c] = float("nan") if j in (0, len(cl) - 1) else big
            elif kind == "pos_inf":
                x[n, h, w, c] = float("inf") if j in (len(cl) // 2, len(cl) - 1) else big
        if kind in ("zeros_neg_first", "zeros_pos_first"):
            # nothing positive may reach into the window from its neighbours' plants: the rest of the channel < 0
            keep = torch.zeros(H, W, dtype=torch.bool)
            for _, h, w in cl:
                keep[h, w] = True
            x[n, :, :, c] = torch.where(keep, x[n, :, :, c], -x[n, :, :, c].abs() - 1.0)
        done.append((kind, n, p, q, c))
    return done


# pool cases of the kernel tests: (k, stride, pad, H, W)
POOL_CASES = ((3, 2, 1, 5, 4), (3, 2, 1, 2, 3), (2, 2, 0, 4, 6), (3, 1, 1, 5, 4), (3, 3, 0, 7, 8), (5, 2, 2, 7, 6),
              (15, 4, 7, 16, 16))


def pool_case(k, st, pad, H, W, dt, seed=11, N=2, C=8):
    """(x with the plants, gy, acc, plants) of one pool case, all stored in dt."""
    x = tied((N, H, W, C), F32, seed)
    plants = plant(x, k, st, pad)
    P, Q = pool_out(H, k, st, pad), pool_out(W, k, st, pad)
    return x.to(dt), values((N, P, Q, C), dt, seed + 1), values((N, H, W, C), dt, seed + 2), plants


# upsample shapes of the kernel tests: (mode, scale, H, W); see test_resample_kernels_gpu.UP_SHAPES_DOC
def up_shapes():
    full = [(m, s, H, W) for m in (0, 1, 2) for s in (1, 2, 3, 4, 8, 16)
            for (H, W) in ((1, 1), (1, 5), (5, 1), (2, 2), (6, 5))]
    keep = []
    for m, s, H, W in full:
        if m == 2 and s in (3, 8):          # nearest: one rule (o // s) at every scale; 1, 2, 4, 16 kept
            continue
        if s == 8 and (H, W) in ((1, 5), (5, 1), (2, 2)):   # scale 8 selects what 4 and 16 select
            continue
        if s == 1 and (H, W) in ((1, 5), (5, 1)):   # scale 1 is the identity at every shape
            continue
        keep.append((m, s, H, W))
    keep.append((1, 3, 33, 17))
    return keep
