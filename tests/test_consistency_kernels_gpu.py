"""Kernel-level tests of the two-view consistency and loss-side kernels (memread.hip, dg_cat_combine of
resample.hip, dg_bce_loss / dg_grad_unscale of head_loss.hip) against the float64 restatements of
tests/consistency_ref.py, per element in max norm: |out - ref| <= bound, never an L2 norm (one bad row in
16,000 must fail).

Bounds (derived, not measured).  f32: tol * max|ref| with the tolerances the older tests of the same
quantities use (P 1e-6, head output and losses 1e-5, logit gradients 1e-4, dmem / gw / gb 1e-5).  An output
stored once in a 16-bit type T from an f32 value is off by at most half an ulp of T; one full ulp is
allowed, u_T |ref| per element (u = 2^-8 bf16, 2^-11 f16), plus the f32 bound of the quantity, plus for f16
the subnormal spacing 2^-24.  The 16-bit forwards are compared on the rounded logits; where a kernel's loss
or head sees the stored probabilities, so does the reference (P rounded to T).  The backwards take host-made
P (softmax(l).to(T)) and are judged as the functions they implement; a stored zero's logarithm is read as
log(tiny_T) (consistency_ref.TINY; include/dgvcc.h dg_softmax_jsd_bwd).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import consistency_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
CODE = {F32: 0, BF16: 1, F16: 2}
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
VEC = {F32: 4, BF16: 8, F16: 8}
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
dt_ids = lambda d: IDS.get(d, None)


def _k():
    from dgvcc_amd import kernels as K
    return K


def close(out, ref, dt, tol32, what=""):
    """|out - ref| <= tol32 max|ref| (+ u_T |ref| (+ 2^-24 for f16) for an output stored in a 16-bit T)."""
    out, ref = out.double().cpu(), ref.double().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), (what, "non-finite output")
    bound = tol32 * ref.abs().max()
    if dt != F32:
        bound = bound + U[dt] * ref.abs() + (2.0 ** -24 if dt == F16 else 0.0)
    err = (out - ref).abs()
    over = (err - bound).max().item()
    assert over <= 0.0, (what, "max err %.3e, max|ref| %.3e, worst excess %.3e" % (
        err.max().item(), ref.abs().max().item(), over))


def close_scalar(out, ref, tol, what=""):
    out, ref = float(out), float(ref.detach() if torch.is_tensor(ref) else ref)
    assert abs(out - ref) <= tol * abs(ref), (what, out, ref)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(autouse=True)
def _end_run_on_device_fault():
    """A device fault ends the run: nothing more is launched on a faulted device."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device fault: {e}", returncode=3)


# ------------------------------------------------------------------------------ slot softmax ------
SOFTMAX_CASES = [(C, dt, M) for C in (512, 1024, 2048) for dt in DTYPES for M in (1, 7, 130)]
SOFTMAX_CASES.append((512, F32, 16389))  # > 4 * 4096 rows, not a multiple of 4: grid-stride loop
sm_ids = [f"C{C}-{IDS[dt]}-M{M}" for C, dt, M in SOFTMAX_CASES]


@functools.lru_cache(maxsize=None)
def _logits(kind, M, C, dt):
    """(L1, L2) rounded to the storage type, and their float64 softmaxes (shared, not modified)."""
    l1, l2 = R.jsd_inputs(kind, M, C, 1000 + M + C)
    l1, l2 = l1.to(dt), l2.to(dt)
    return l1, l2, R.softmax_fwd(l1), R.softmax_fwd(l2)


def _upstream(M, C, dt, seed):
    g = _gen(seed)
    return (0.3 * torch.randn(M, C, generator=g)).to(dt), (0.3 * torch.randn(M, C, generator=g)).to(dt)


@pytest.mark.parametrize("C,dt,M", SOFTMAX_CASES, ids=sm_ids)
def test_softmax_single(dev, C, dt, M):
    K = _k()
    l1, _, p1, _ = _logits("ordinary", M, C, dt)
    L = l1.to(dev)
    P = torch.empty_like(L)
    K.call("dg_softmax_fwd", CODE[dt], K.ptr(L), M, C, K.ptr(P), K.stream())
    Ph = p1.to(dt)  # host-made stored probabilities: the backward does not depend on the forward kernel
    G, _ = _upstream(M, C, dt, 7)
    Pd, Gd = Ph.to(dev), G.to(dev)
    GL = torch.empty_like(Pd)
    K.call("dg_softmax_bwd", CODE[dt], K.ptr(Pd), K.ptr(Gd), M, C, K.ptr(GL), K.stream())
    torch.cuda.synchronize()
    close(P, p1, dt, 1e-6, "P")
    close(GL, R.softmax_bwd(Ph, G), dt, 1e-4, "GL")


def _pair_like_bwd(K, dev, entry, ref_fn, dt, M, C, p1, p2, coef, **kw):
    """The upstream combinations of dg_softmax_pair_bwd / dg_softmax_jsd_bwd on host-made P: both given, G1 or
    G2 NULL, coef NULL, and the loss term alone (the many-row case runs the first only, for time)."""
    P1h, P2h = p1.to(dt), p2.to(dt)
    G1, G2 = _upstream(M, C, dt, 8)
    P1, P2, G1d, G2d = P1h.to(dev), P2h.to(dev), G1.to(dev), G2.to(dev)
    cf = torch.tensor([coef], dtype=torch.float32, device=dev)
    out = {}
    for name, (a, b, c) in {"both": (G1, G2, coef), "g1": (G1, None, coef), "g2": (None, G2, coef),
                            "nocoef": (G1, G2, None), "loss_only": (None, None, coef)}.items():
        if M > 1000 and name != "both":
            continue
        GL1, GL2 = torch.empty_like(P1), torch.empty_like(P2)
        K.call(entry, CODE[dt], K.ptr(P1), K.ptr(P2), K.ptr(G1d) if a is not None else None,
               K.ptr(G2d) if b is not None else None, M, C, K.ptr(cf) if c is not None else None, K.ptr(GL1),
               K.ptr(GL2), K.stream())
        out[name] = (GL1, GL2, ref_fn(P1h, P2h, a, b, c, **kw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("C,dt,M", SOFTMAX_CASES, ids=sm_ids)
def test_softmax_pair(dev, C, dt, M):
    K = _k()
    l1, l2, p1, p2 = _logits("ordinary", M, C, dt)
    L1, L2 = l1.to(dev), l2.to(dev)
    P1, P2 = torch.empty_like(L1), torch.empty_like(L2)
    loss = torch.full((), -1.0, device=dev)
    work = torch.empty(K.query("dg_softmax_workspace", M) // 4 + 1, device=dev)
    K.call("dg_softmax_pair_fwd", CODE[dt], K.ptr(L1), K.ptr(L2), M, C, K.ptr(P1), K.ptr(P2), K.ptr(loss),
           K.ptr(work), K.stream())
    torch.cuda.synchronize()
    close(P1, p1, dt, 1e-6, "P1")
    close(P2, p2, dt, 1e-6, "P2")
    close_scalar(loss, R.pair_loss(p1.to(dt), p2.to(dt)), 1e-5, "loss_con")  # the loss sees the stored P
    # k = 2 coef / (M C) = 100: the loss term is of the size of the upstream one
    for name, (GL1, GL2, (r1, r2)) in _pair_like_bwd(K, dev, "dg_softmax_pair_bwd", R.pair_bwd, dt, M, C, p1, p2,
                                                     50.0 * M * C).items():
        close(GL1, r1, dt, 1e-4, name + " GL1")
        close(GL2, r2, dt, 1e-4, name + " GL2")


def _jsd_fwd(K, dev, dt, M, C, l1, l2):
    L1, L2 = l1.to(dev), l2.to(dev)
    P1, P2 = torch.empty_like(L1), torch.empty_like(L2)
    loss = torch.full((), -1.0, device=dev)
    work = torch.empty(K.query("dg_softmax_workspace", M) // 4 + 1, device=dev)
    K.call("dg_softmax_jsd_fwd", CODE[dt], K.ptr(L1), K.ptr(L2), M, C, K.ptr(P1), K.ptr(P2), K.ptr(loss),
           K.ptr(work), K.stream())
    torch.cuda.synchronize()
    return P1, P2, loss.item()


@pytest.mark.parametrize("C,dt,M", SOFTMAX_CASES, ids=sm_ids)
def test_softmax_jsd_ordinary(dev, C, dt, M):
    K = _k()
    l1, l2, p1, p2 = _logits("ordinary", M, C, dt)
    P1, P2, loss = _jsd_fwd(K, dev, dt, M, C, l1, l2)
    close(P1, p1, dt, 1e-6, "P1")
    close(P2, p2, dt, 1e-6, "P2")
    close_scalar(loss, R.jsd_loss(l1, l2), 1e-5, "loss_kl")
    # k = coef / (2 M) = 1.5
    for name, (GL1, GL2, (r1, r2)) in _pair_like_bwd(K, dev, "dg_softmax_jsd_bwd", R.jsd_bwd, dt, M, C, p1, p2,
                                                     3.0 * M, tiny=R.TINY[dt]).items():
        close(GL1, r1, dt, 1e-4, name + " GL1")
        close(GL2, r2, dt, 1e-4, name + " GL2")


@pytest.mark.parametrize("dt", DTYPES, ids=dt_ids)
def test_softmax_jsd_separated(dev, dt):
    """Well-separated views (|log p1 - log p2| up to ~48, every probability >= 1e-30, asserted on the CPU):
    the forward loss meets the ordinary bound in every storage type (the term was inf for x <~ -17.33 and
    x >~ 44.3 before its range fix); the f32 and bf16 backwards meet their ordinary bounds; the f16 backward
    is asserted finite only (its stored zeros lose what no backward from P can recover)."""
    K = _k()
    M, C = 37, 512
    l1, l2 = R.jsd_inputs("separated", M, C, 31)
    l1, l2 = l1.to(dt), l2.to(dt)
    p1, p2 = R.softmax_fwd(l1), R.softmax_fwd(l2)
    P1, P2, loss = _jsd_fwd(K, dev, dt, M, C, l1, l2)
    print("separated", IDS[dt], "loss", loss, "ref", R.jsd_loss(l1, l2).item())
    close(P1, p1, dt, 1e-6, "P1")
    close(P2, p2, dt, 1e-6, "P2")
    close_scalar(loss, R.jsd_loss(l1, l2), 1e-5, "loss_kl")
    for name, (GL1, GL2, (r1, r2)) in _pair_like_bwd(K, dev, "dg_softmax_jsd_bwd", R.jsd_bwd, dt, M, C, p1, p2,
                                                     3.0 * M, tiny=R.TINY[dt]).items():
        print("separated", IDS[dt], name, "finite", bool(torch.isfinite(GL1).all() and torch.isfinite(GL2).all()))
        if dt == F16:
            assert torch.isfinite(GL1).all() and torch.isfinite(GL2).all(), name
        else:
            close(GL1, r1, dt, 1e-4, name + " GL1")
            close(GL2, r2, dt, 1e-4, name + " GL2")


def test_softmax_jsd_underflow_f16(dev):
    """f16 storage rounds p < 3e-8 to 0; with a zero in one view only the backward read log(0) = -inf and
    turned the row's logit gradients non-finite.  The contract: a stored zero's logarithm is log(2^-25)."""
    K = _k()
    M, C, dt = 192, 1024, F16
    l1, l2 = R.jsd_inputs("underflow", M, C, 32)
    l1, l2 = l1.to(dt), l2.to(dt)
    p1, p2 = R.softmax_fwd(l1), R.softmax_fwd(l2)
    one_sided = (p1.to(dt) == 0) != (p2.to(dt) == 0)
    assert one_sided.sum().item() >= 1
    for name, (GL1, GL2, (r1, r2)) in _pair_like_bwd(K, dev, "dg_softmax_jsd_bwd", R.jsd_bwd, dt, M, C, p1, p2,
                                                     3.0 * M, tiny=R.TINY[dt]).items():
        bad = (~torch.isfinite(GL1).all(1) | ~torch.isfinite(GL2).all(1)).sum().item()
        print("underflow f16", name, "one-sided zeros", one_sided.sum().item(), "rows hit",
              one_sided.any(1).sum().item(), "non-finite rows", bad)
        close(GL1, r1, dt, 1e-4, name + " GL1")
        close(GL2, r2, dt, 1e-4, name + " GL2")


# ------------------------------------------------------------------------------ fused memory head -
# dt, C, M, nv, loss, act, bias, KL-JSD inputs
HEAD_CASES = [
    (F32, 2048, 130, 2, 2, 1, True, "ordinary"),
    (BF16, 2048, 130, 2, 1, 2, True, "ordinary"),
    (F16, 2048, 7, 2, 2, 0, False, "ordinary"),
    (F32, 512, 1, 1, 0, 0, False, "ordinary"),
    (BF16, 512, 7, 1, 0, 1, True, "ordinary"),
    (F16, 512, 130, 2, 0, 2, True, "ordinary"),
    (F32, 1024, 7, 2, 0, 2, False, "ordinary"),
    (BF16, 1024, 130, 2, 2, 1, True, "ordinary"),
    (F16, 1024, 1, 2, 1, 1, True, "ordinary"),
    (F32, 2048, 1, 2, 1, 0, True, "ordinary"),
    (BF16, 2048, 1, 1, 0, 2, False, "ordinary"),
    (F16, 2048, 130, 1, 0, 1, True, "ordinary"),
    (F32, 512, 16389, 2, 2, 1, True, "ordinary"),  # > 4096 partial rows into mem_head_colsum's 16 chunks
    (F32, 512, 37, 2, 2, 1, True, "separated"),
    (BF16, 512, 37, 2, 2, 1, True, "separated"),
    (F16, 512, 37, 2, 2, 1, True, "separated"),    # backward asserted finite only
    (F16, 1024, 192, 2, 2, 1, True, "underflow"),
]
head_ids = [f"{IDS[c[0]]}-C{c[1]}-M{c[2]}-nv{c[3]}-loss{c[4]}-act{c[5]}-{'b' if c[6] else 'nob'}-{c[7]}"
            for c in HEAD_CASES]


@pytest.mark.parametrize("dt,C,M,nv,loss,act,bias,kind", HEAD_CASES, ids=head_ids)
def test_softmax_head(dev, dt, C, M, nv, loss, act, bias, kind):
    K = _k()
    k = 24
    g = _gen(50 + C + M)
    l1, l2 = R.jsd_inputs(kind, M, C, 31 if kind == "separated" else 32 if kind == "underflow" else 40 + M)
    ls = [l1.to(dt), l2.to(dt)][:nv]
    ps = [R.softmax_fwd(l) for l in ls]
    mem = torch.randn(k, C, generator=g)
    w = 0.05 * torch.randn(k, generator=g)
    b = torch.tensor([0.02]) if bias else None
    coef = (50.0 * M * C if loss == 1 else 3.0 * M) if loss else None

    memd, wd = mem.to(dev), w.to(dev)
    bd = b.to(dev) if bias else None
    v = torch.empty(C, device=dev)
    K.call("dg_mem_head_vec", K.ptr(memd), K.ptr(wd), k, C, K.ptr(v), K.stream())
    torch.cuda.synchronize()
    close(v, R.head_vec(mem, w), F32, 1e-5, "v")
    vh = R.head_vec(mem, w).float()  # host-made f32 v for both passes
    vd = vh.to(dev)

    # forward: stored P, head outputs, loss; then P = NULL (eval): the same head bits
    Ls = [l.to(dev) for l in ls]
    Ps = [torch.empty_like(L) for L in Ls]
    yh = [torch.empty(M, device=dev) for _ in Ls]
    yh0 = [torch.empty(M, device=dev) for _ in Ls]
    lo = torch.full((), -1.0, device=dev)
    work = torch.empty(K.query("dg_mem_head_workspace", M, C) // 4 + 1, device=dev)
    two = nv == 2
    for P_, y_ in ((Ps, yh), (None, yh0)):
        K.call("dg_softmax_head_fwd", CODE[dt], nv, loss, K.ptr(Ls[0]), K.ptr(Ls[1]) if two else None, M, C,
               K.ptr(vd), K.ptr(bd), act, K.ptr(P_[0]) if P_ else None, K.ptr(P_[1]) if (P_ and two) else None,
               K.ptr(y_[0]), K.ptr(y_[1]) if two else None, K.ptr(lo) if loss else None, K.ptr(work), K.stream())
    torch.cuda.synchronize()
    pst = [p.to(dt) for p in ps]  # the head and the JSD-MSE see the stored probabilities
    yref = [R.head_fwd(p, vh, b.item() if bias else None, act) for p in pst]
    for i in range(nv):
        close(Ps[i], ps[i], dt, 1e-6, f"P{i + 1}")
        close(yh[i], yref[i], F32, 1e-5, f"yh{i + 1}")
        assert torch.equal(yh[i], yh0[i]), f"yh{i + 1} with P = NULL"
    if loss:
        lref = R.pair_loss(pst[0], pst[1]) if loss == 1 else R.jsd_loss(ls[0], ls[1])
        print("head", kind, IDS[dt], "loss", lo.item(), "ref", lref.item())
        close_scalar(lo, lref, 1e-5, "loss")

    # backward on host-made P, yh, gyh
    yhh = [y.float() for y in yref]
    gyh = [torch.randn(M, generator=g) for _ in range(nv)]
    gL, u, gb = R.head_bwd(pst, vh, act, yhh, gyh, loss, coef, R.TINY[dt])
    Pd = [p.to(dev) for p in pst]
    yd, gd = [y.to(dev) for y in yhh], [q.to(dev) for q in gyh]
    GL = [torch.empty_like(P) for P in Pd]
    cf = torch.tensor([coef], dtype=torch.float32, device=dev) if loss else None
    nw = K.amax_words(C)
    am = torch.full((2 * nw,) if dt == F32 else (2,), -1.0, device=dev)
    K.call("dg_softmax_head_bwd", CODE[dt], nv, loss, K.ptr(Pd[0]), K.ptr(Pd[1]) if two else None, M, C, K.ptr(vd),
           act, K.ptr(yd[0]), K.ptr(yd[1]) if two else None, K.ptr(gd[0]), K.ptr(gd[1]) if two else None,
           K.ptr(cf), K.ptr(GL[0]), K.ptr(GL[1]) if two else None, K.ptr(work), K.ptr(am), K.stream())
    dmem, gw, gbo = torch.empty(k, C, device=dev), torch.empty(k, device=dev), torch.empty(1, device=dev)
    K.call("dg_mem_head_grads", K.ptr(work), M, C, K.ptr(memd), K.ptr(wd), k, K.ptr(dmem), K.ptr(gw), K.ptr(gbo),
           K.stream())
    torch.cuda.synchronize()
    for i in range(nv):
        if dt == F16 and kind == "separated":
            assert torch.isfinite(GL[i]).all(), f"GL{i + 1}"
            continue
        close(GL[i], gL[i], dt, 1e-4, f"GL{i + 1}")
        stored = GL[i].abs().max().item()
        if dt == F32:  # per-slot operand maxima: exact
            assert am[i * nw].item() == stored
            assert torch.equal(am[i * nw + 1:i * nw + 1 + C], GL[i].abs().amax(dim=0))
        else:  # one word per view: bounds the stored values, within one ulp of T
            assert stored <= am[i].item() <= stored * (1.0 + U[dt]), (i, am[i].item(), stored)
    rdmem, rgw = R.head_grads(mem, w, u)
    close(dmem, rdmem, F32, 1e-5, "dmem")
    close(gw, rgw, F32, 1e-5, "gw")
    assert abs(gbo.item() - gb.item()) <= 1e-5 * max(1.0, abs(gb.item())), (gbo.item(), gb.item())

    # GL = NULL (head gradients only): the same u, so the same gw / gb bits
    K.call("dg_softmax_head_bwd", CODE[dt], nv, loss, K.ptr(Pd[0]), K.ptr(Pd[1]) if two else None, M, C, K.ptr(vd),
           act, K.ptr(yd[0]), K.ptr(yd[1]) if two else None, K.ptr(gd[0]), K.ptr(gd[1]) if two else None,
           None, None, None, K.ptr(work), None, K.stream())
    gw2, gb2 = torch.empty_like(gw), torch.empty_like(gbo)
    K.call("dg_mem_head_grads", K.ptr(work), M, C, K.ptr(memd), K.ptr(wd), k, None, K.ptr(gw2), K.ptr(gb2),
           K.stream())
    torch.cuda.synchronize()
    assert torch.equal(gw2, gw) and torch.equal(gb2, gbo)


# ------------------------------------------------------------------------------ e-mask ------------
def _strided(t2d, ld, off, fill):
    """[M, C] values placed at columns [off, off + C) of a [M, ld] buffer filled with `fill`."""
    buf = torch.full((t2d.shape[0], ld), fill, dtype=t2d.dtype)
    buf[:, off:off + t2d.shape[1]] = t2d
    return buf


def _emask_run(K, dev, dt, N, HW, C, y1, y2, stats, thr, drops, seed):
    """Forward and backward on a channel slice of wider buffers; returns CPU tensors."""
    V, M = VEC[dt], N * HW
    ld, ldgy = C + 2 * V, C + V
    Y1 = _strided(y1.reshape(M, C), ld, V, 7.0).to(dev)
    Y2 = _strided(y2.reshape(M, C), ld, V, 7.0).to(dev)
    sd = [s.contiguous().to(dev) for s in stats]
    dd = [d.contiguous().to(dev) if d is not None else None for d in drops]
    m1, m2 = torch.empty(M, C, dtype=dt, device=dev), torch.empty(M, C, dtype=dt, device=dev)
    mask = torch.full((M, C), 9, dtype=torch.uint8, device=dev)
    K.call("dg_emask_fwd", CODE[dt], K.ptr(Y1[:, V:]), K.ptr(Y2[:, V:]), ld, N, HW, C, K.ptr(sd[0]), K.ptr(sd[1]),
           K.ptr(sd[2]), K.ptr(sd[3]), thr, K.ptr(dd[0]), K.ptr(dd[1]), K.ptr(m1), K.ptr(m2), K.ptr(mask),
           K.stream())
    g = _gen(seed)
    gm1 = torch.randn(M, C, generator=g).to(dt)
    gm2 = torch.randn(M, C, generator=g).to(dt)
    GY1 = torch.full((M, ldgy), 5.0, dtype=dt, device=dev)
    GY2 = torch.full((M, ldgy), 5.0, dtype=dt, device=dev)
    g1d, g2d = gm1.to(dev), gm2.to(dev)
    K.call("dg_emask_bwd", CODE[dt], K.ptr(g1d), K.ptr(g2d), N, HW, C, K.ptr(mask), K.ptr(dd[0]), K.ptr(dd[1]),
           K.ptr(GY1), K.ptr(GY2), ldgy, K.stream())
    torch.cuda.synchronize()
    assert (Y1[:, :V] == 7).all() and (Y1[:, V + C:] == 7).all() and (Y2[:, :V] == 7).all()
    return m1.cpu(), m2.cpu(), mask.cpu(), gm1, gm2, GY1.cpu(), GY2.cpu()


def _emask_check(dt, N, HW, C, y1, y2, drops, dist, thr, res):
    m1, m2, mask, gm1, gm2, GY1, GY2 = res
    M = N * HW
    # the mask bytes: 0/1, exact except within 1e-5 thr of the threshold (<= 0.1 % of the elements)
    assert ((mask == 0) | (mask == 1)).all()
    near = ((dist - thr).abs() <= 1e-5 * thr).reshape(M, C)
    assert near.double().mean().item() <= 1e-3
    want = (dist < thr).reshape(M, C)
    assert torch.equal(mask.bool() | near, want | near)
    keep = mask.bool()
    per_px = lambda d: torch.ones(M, C) if d is None else d[:, None, :].expand(N, HW, C).reshape(M, C)
    d1, d2 = per_px(drops[0]), per_px(drops[1])
    zero = torch.zeros(M, C, dtype=dt)
    # one f32 product stored in T where kept, 0 elsewhere: exact
    assert torch.equal(m1, torch.where(keep, (y1.reshape(M, C).float() * d1).to(dt), zero))
    assert torch.equal(m2, torch.where(keep, (y2.reshape(M, C).float() * d2).to(dt), zero))
    assert torch.equal(GY1[:, :C], torch.where(keep, (gm1.float() * d1).to(dt), zero))
    assert torch.equal(GY2[:, :C], torch.where(keep, (gm2.float() * d2).to(dt), zero))
    assert (GY1[:, C:] == 5).all() and (GY2[:, C:] == 5).all()  # outside the written channels: untouched


@pytest.mark.parametrize("C,dt,seed", R.EMASK_CASES, ids=[f"C{c}-{IDS[d]}" for c, d, _ in R.EMASK_CASES])
@pytest.mark.parametrize("use_drop", [True, False], ids=["drop", "nodrop"])
def test_emask(dev, C, dt, seed, use_drop):
    K = _k()
    N, HW = 3, 35  # instance boundaries inside blocks
    y1, y2, mu1, is1, mu2, is2, drop1, drop2, thr = R.emask_inputs(N, HW, C, dt, seed)
    drops = (drop1, drop2) if use_drop else (None, None)
    if use_drop:
        assert (drop1 == 0).any() and (drop1 > 1).any()
    dist = R.emask_dist(y1, y2, mu1, is1, mu2, is2)
    res = _emask_run(K, dev, dt, N, HW, C, y1, y2, (mu1, is1, mu2, is2), thr, drops, seed + 100)
    _emask_check(dt, N, HW, C, y1, y2, drops, dist, thr, res)


def test_emask_grid_stride(dev):
    """N HW = 1,048,600 pixels of 16 f32 channels: 64 pixels per block, one block more than the 16384-block
    cap.  The reference distance is built in chunks."""
    K = _k()
    N, HW, C, dt = 4, 262150, 16, F32
    g = _gen(77)
    y1 = torch.randn(N, HW, C, generator=g)
    y2 = y1 + 0.4 * torch.randn(N, HW, C, generator=g)
    mu1, mu2 = y1.mean(1), y2.mean(1)
    is1, is2 = 1.0 / y1.std(1), 1.0 / y2.std(1)
    drop1 = (torch.rand(N, C, generator=g) >= 0.3).float() / 0.7
    drop2 = (torch.rand(N, C, generator=g) >= 0.3).float() / 0.7
    chunks = [R.emask_dist(y1[:, s:s + 32768], y2[:, s:s + 32768], mu1, is1, mu2, is2).float()
              for s in range(0, HW, 32768)]
    dist32 = torch.cat(chunks, 1)
    thr = torch.tensor(dist32.flatten()[:200001].median().item() * (1 + 2.0 ** -12), dtype=torch.float32).item()
    res = _emask_run(K, dev, dt, N, HW, C, y1, y2, (mu1, is1, mu2, is2), thr, (drop1, drop2), 177)
    # float64 distance only where the float32 one is within 1e-4 thr of the threshold (it is within 1e-6 of
    # the float64 one); elsewhere the decision is the float32 one's
    band = (dist32 - thr).abs() <= 1e-4 * thr
    dist = dist32.double()
    idx = band.nonzero(as_tuple=True)
    ia = (y1[idx].double() - mu1[idx[0], idx[2]].double()) * is1[idx[0], idx[2]].double()
    ib = (y2[idx].double() - mu2[idx[0], idx[2]].double()) * is2[idx[0], idx[2]].double()
    dist[idx] = (ia - ib).abs()
    _emask_check(dt, N, HW, C, y1, y2, (drop1, drop2), dist, thr, res)


# ------------------------------------------------------------------------------ class maps, product
@pytest.mark.parametrize("N,h,w,s", [(2, 3, 5, 4), (1, 7, 9, 1), (1, 130, 127, 16)])
def test_cls_combine(dev, N, h, w, s):
    """Exact against the torch restatement; (1, 130, 127, 16) has more than 16384 x 256 outputs."""
    K = _k()
    g = _gen(60 + h)
    thr = 0.5
    c1, c2 = torch.rand(N, h, w, generator=g), torch.rand(N, h, w, generator=g)
    c1.view(-1)[::7] = thr  # values exactly at the threshold count as set
    c2.view(-1)[3::11] = thr
    cgt = (torch.rand(N, h, w, generator=g) > 0.6).float()
    c1d, c2d, gtd = c1.to(dev), c2.to(dev), cgt.to(dev)
    for two, gt, want_err in ((True, True, True), (True, False, True), (True, True, False), (False, True, False),
                              (False, False, False)):
        cres = torch.full((N, h * s, w * s), -1.0, device=dev)
        cerr = torch.full((N, h * s, w * s), -1.0, device=dev)
        K.call("dg_cls_combine", K.ptr(c1d), K.ptr(c2d) if two else None, K.ptr(gtd) if gt else None, N, h, w, s,
               thr, K.ptr(cres), K.ptr(cerr) if want_err else None, K.stream())
        torch.cuda.synchronize()
        rres, rerr = R.cls_combine(c1, c2 if two else None, cgt if gt else None, s, thr)
        assert torch.equal(cres.cpu(), rres), (two, gt)
        if want_err:
            assert torch.equal(cerr.cpu(), rerr), (two, gt)
        else:
            assert (cerr == -1).all()


@pytest.mark.parametrize("n", [1, 257, 4194307])
def test_mul_f32(dev, n):
    K = _k()
    g = _gen(n % 1000)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = a.to(dev), b.to(dev)
    out = torch.full((n + 1,), -1.0, device=dev)
    K.call("dg_mul_f32", K.ptr(ad), K.ptr(bd), n, K.ptr(out), K.stream())
    K.call("dg_mul_f32", K.ptr(ad), K.ptr(bd), n, K.ptr(ad), K.stream())  # out aliasing a, as the engine calls it
    torch.cuda.synchronize()
    assert torch.equal(out[:n].cpu(), a * b) and out[n].item() == -1.0
    assert torch.equal(ad.cpu(), a * b)


# ------------------------------------------------------------------------------ cat-combine -------
@pytest.mark.parametrize("dt,C", [(F32, 64), (BF16, 256), (F16, 8)], ids=["f32-C64", "bf16-C256", "f16-C8"])
@pytest.mark.parametrize("N,H,W", [(3, 8, 12), (1, 68, 964)])
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
def test_cat_combine(dev, dt, C, N, H, W, use_bias):
    """(3, 8, 12): 288 pixels in 5 blocks of 58, a short last block; (1, 68, 964): 65552 pixels, 65 per block
    under the 1024-block cap, so the last 15 blocks are empty and their partial rows must read n = 0."""
    K = _k()
    V, M = VEC[dt], N * H * W
    g = _gen(70 + C + H)
    z1 = torch.randn(N, H, W, C, generator=g).to(dt)
    z2 = torch.randn(N, H // 2, W // 2, C, generator=g).to(dt)
    z3 = torch.randn(N, H // 4, W // 4, C, generator=g).to(dt)
    bias = (torch.randn(C, generator=g) + 3.0) if use_bias else None  # |mean| >> std: the shift matters
    ld1, ld2, ld3 = C + V, C + 2 * V, C + V
    Z1 = _strided(z1.reshape(M, C), ld1, 0, 7.0).to(dev)
    Z2 = _strided(z2.reshape(-1, C), ld2, 0, 7.0).to(dev)
    Z3 = _strided(z3.reshape(-1, C), ld3, 0, 7.0).to(dev)
    bd = bias.to(dev) if use_bias else None
    rows = K.query("dg_cat_combine_part_rows", N, H, W)
    assert rows == min(1024, (M + 63) // 64)
    Zs = torch.full((M, C + 2 * V), 5.0, dtype=dt, device=dev)
    part_s = torch.full((rows, 3, C), -1.0, device=dev)
    K.call("dg_cat_combine", CODE[dt], K.ptr(Z1), ld1, K.ptr(Z2), ld2, K.ptr(Z3), ld3, N, H, W, C, K.ptr(bd),
           K.ptr(Zs), C + 2 * V, K.ptr(part_s), K.stream())
    part_a = torch.full((rows, 3, C), -1.0, device=dev)
    K.call("dg_cat_combine", CODE[dt], K.ptr(Z1), ld1, K.ptr(Z2), ld2, K.ptr(Z3), ld3, N, H, W, C, K.ptr(bd),
           K.ptr(Z1), ld1, K.ptr(part_a), K.stream())  # z aliasing z1, as the engine calls it
    torch.cuda.synchronize()
    zs, za = Zs[:, :C].cpu(), Z1[:, :C].cpu()
    assert torch.equal(zs, za) and torch.equal(part_s, part_a)
    assert (Zs[:, C:] == 5).all() and (Z1[:, C:] == 7).all() and (Z2[:, C:] == 7).all()
    # <= 16 f32 roundings of partial sums no larger than 2 max|z|: 16 * 2^-24 * 2 = 1.9e-6 of max|z|
    close(zs.reshape(N, H, W, C), R.cat_combine(z1, z2, z3, bias), dt, 2e-6, "z")
    ppb = -(-M // rows)
    counts = torch.tensor([max(0, min(M, (b + 1) * ppb) - b * ppb) for b in range(rows)], dtype=torch.float32)
    assert counts.sum().item() == M
    assert torch.equal(part_s[:, 0, :].cpu(), counts[:, None].expand(rows, C))
    assert (part_s.cpu()[counts == 0] == 0).all()
    gam, bet = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    st = K.bn_part_finalize(part_s, rows, C, gam, bet, rm, rv, 0.1, 1e-5)
    torch.cuda.synchronize()
    zf = zs.double()
    relerr = lambda a, b: ((a.double().cpu() - b).abs().max() / b.abs().max()).item()
    if use_bias:  # without it the means are ~0 and a bound relative to them says nothing
        assert relerr(st[0], zf.mean(0)) < 1e-6
    assert relerr(st[1], 1.0 / (zf.var(0, unbiased=False) + 1e-5).sqrt()) < 2e-6


# ------------------------------------------------------------------------------ BCE, unscale ------
@pytest.mark.parametrize("n", [1, 255, 257, 262149])
def test_bce_loss(dev, n):
    """Against F.binary_cross_entropy in float64 on the same f32 values; 262149 is beyond 1024 blocks."""
    K = _k()
    g = _gen(80 + n % 100)
    p, t = torch.rand(n, generator=g), torch.rand(n, generator=g)
    edge_p = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    edge_t = torch.tensor([0.0, 1.0, 0.3, 0.0, 1.0, 0.3])
    if n >= 6:
        p[:6], t[:6] = edge_p, edge_t
    else:
        p[0], t[0] = 0.0, 0.3
    pd_ = p.double().requires_grad_(True)
    want = F.binary_cross_entropy(pd_, t.double())
    (2.5 * want).backward()
    P, T = p.to(dev), t.to(dev)
    work = torch.empty(K.query("dg_reduce_workspace", n) // 4 + 1, device=dev)
    loss, loss2 = torch.full((), -1.0, device=dev), torch.full((), -1.0, device=dev)
    dp = torch.full((n + 1,), -1.0, device=dev)
    K.call("dg_bce_loss", K.ptr(P), K.ptr(T), n, K.ptr(loss), K.ptr(dp), 2.5, K.ptr(work), K.stream())
    K.call("dg_bce_loss", K.ptr(P), K.ptr(T), n, K.ptr(loss2), None, 2.5, K.ptr(work), K.stream())  # dpred = NULL
    torch.cuda.synchronize()
    close_scalar(loss, want, 1e-5, "loss")
    assert loss2.item() == loss.item()
    got, ref = dp[:n].double().cpu(), pd_.grad
    assert dp[n].item() == -1.0 and torch.isfinite(got).all()
    assert ((got - ref).abs() <= 1e-5 * ref.abs()).all(), ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max()
    rl, rg = R.bce(p, t, 2.5)
    close_scalar(loss, rl, 1e-5, "loss vs restatement")
    assert ((got - rg).abs() <= 1e-5 * rg.abs()).all()


@pytest.mark.parametrize("n", [1, 300, 2097155])
def test_grad_unscale(dev, n):
    """g *= inv_scale exactly; the flag is rewritten by every call.  2,097,155 is beyond the 8192-block grid."""
    K = _k()
    g = _gen(90 + n % 100)
    inv = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    x = torch.randn(n, generator=g) * 100.0
    bads = [(None, None), (0, float("inf")), (n - 1, float("nan"))]
    if n > 8192 * 256:
        bads.append((n - 2, float("-inf")))  # in the grid-stride tail
    for pos, val in bads:
        xi = x.clone()
        if pos is not None:
            xi[pos] = val
        xd = xi.to(dev)
        flag = torch.ones(1, dtype=torch.int32, device=dev)  # a stale 1 must not survive a finite input
        K.call("dg_grad_unscale", K.ptr(xd), n, inv.item(), K.ptr(flag), K.stream())
        torch.cuda.synchronize()
        assert flag.item() == (0 if pos is None else 1), (pos, val)
        assert torch.equal(xd.cpu().nan_to_num(nan=12345.0), (xi * inv).nan_to_num(nan=12345.0))
