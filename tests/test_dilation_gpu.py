"""Dilated 3x3 convolution by phase decomposition on the GPU:

* the two layout kernels, bitwise against the torch indexing restatement of the identity below;
* engine.ConvLayer with dilation against F.conv2d(padding=d, dilation=d) on the dtype-rounded
  operands, at the tolerances of test_kernels_gpu.test_conv_fwd_dgrad_wgrad (the same kernels do
  the arithmetic), with BatchNorm batch statistics and with a Dropout2d channel mask;
* the decomposition itself: bit-identical to the dense ConvLayer on phase batches formed and
  un-formed on the host;
* ChainPlan: a run of dilated layers kept in phase layout against the per-layer route, bit for bit.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _k():
    from dgvcc_amd import kernels as K
    return K


def relerr(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def to_nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---- the identity, restated with torch indexing (NHWC) --------------------------------------
def s2b_ref(x, d):
    """xs[(n*d + i)*d + j, hp, wp, c] = x[n, hp*d + i, wp*d + j, c], zero outside the image."""
    N, H, W, C = x.shape
    Hp, Wp = -(-H // d), -(-W // d)
    xp = x.new_zeros(N, Hp * d, Wp * d, C)
    xp[:, :H, :W] = x
    return xp.view(N, Hp, d, Wp, d, C).permute(0, 2, 4, 1, 3, 5).reshape(N * d * d, Hp, Wp, C).contiguous()


def b2s_ref(xs, d, H, W):
    """The inverse map, cropped to H x W."""
    Nd, Hp, Wp, C = xs.shape
    N = Nd // (d * d)
    x = xs.view(N, d, d, Hp, Wp, C).permute(0, 3, 1, 4, 2, 5).reshape(N, Hp * d, Wp * d, C)
    return x[:, :H, :W].contiguous()


def test_restatement_is_the_dilated_conv():
    """The restatement above does compute F.conv2d(dilation=d) (float64, ragged size, exact)."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 7, 9, 4, generator=g, dtype=torch.float64)
    w = torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64)
    for d in (2, 3):
        ys = F.conv2d(to_nchw(s2b_ref(x, d)), w, padding=1)
        y = b2s_ref(to_nhwc(ys), d, 7, 9)
        assert (to_nchw(y) - F.conv2d(to_nchw(x), w, padding=d, dilation=d)).abs().max().item() < 1e-13


# ---- layout kernels --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [(8, 12), (7, 9), (6, 5)])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_layout_kernels_bitwise(dev, dtype, HW, d):
    K = _k()
    N, C = 2, 64
    H, W = HW
    g = torch.Generator().manual_seed(d * 100 + H)
    x = torch.randn(N, H, W, C, generator=g).to(dtype)
    xd = K.Act(x.to(dev))
    xs = K.Act(torch.full(K.phase_shape(N, H, W, d) + (C,), float("nan"), dtype=dtype, device=dev))
    K.space_to_batch(xd, d, xs)
    assert torch.equal(xs.buf.cpu(), s2b_ref(x, d))
    ps = torch.randn(*K.phase_shape(N, H, W, d), C, generator=g).to(dtype)  # fill positions hold values
    y = K.Act(torch.full((N, H, W, C), float("nan"), dtype=dtype, device=dev))
    K.batch_to_space(K.Act(ps.to(dev)), d, y)
    assert torch.equal(y.buf.cpu(), b2s_ref(ps, d, H, W))
    # round trip
    back = K.Act(torch.full((N, H, W, C), float("nan"), dtype=dtype, device=dev))
    K.batch_to_space(xs, d, back)
    assert torch.equal(back.buf.cpu(), x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_kernels_channel_slices(dev, dtype):
    """Source and destination are the 64-channel slice at offset 64 of 192-channel buffers; the
    other channels of the destination stay untouched."""
    K = _k()
    N, H, W, d = 2, 7, 9, 2
    g = torch.Generator().manual_seed(5)
    big = torch.randn(N, H, W, 192, generator=g).to(dtype)
    Np, Hp, Wp = K.phase_shape(N, H, W, d)
    dst0 = torch.randn(Np, Hp, Wp, 192, generator=g).to(dtype)
    dst = dst0.to(dev)
    K.space_to_batch(K.Act(big.to(dev), 64, 64), d, K.Act(dst, 64, 64))
    want = dst0.clone()
    want[..., 64:128] = s2b_ref(big[..., 64:128].contiguous(), d)
    assert torch.equal(dst.cpu(), want)
    img0 = torch.randn(N, H, W, 192, generator=g).to(dtype)
    img = img0.to(dev)
    K.batch_to_space(K.Act(dst0.to(dev), 64, 64), d, K.Act(img, 64, 64))
    want = img0.clone()
    want[..., 64:128] = b2s_ref(dst0[..., 64:128].contiguous(), d, H, W)
    assert torch.equal(img.cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_kernels_accumulate(dev, dtype):
    K = _k()
    N, H, W, C, d = 2, 7, 9, 64, 2
    g = torch.Generator().manual_seed(6)
    x = torch.randn(N, H, W, C, generator=g).to(dtype)
    y0 = torch.randn(*K.phase_shape(N, H, W, d), C, generator=g).to(dtype)
    y = K.Act(y0.to(dev))
    K.space_to_batch(K.Act(x.to(dev)), d, y, accumulate=True)
    assert torch.equal(y.buf.cpu(), y0 + s2b_ref(x, d))
    assert y.amax is None  # a sum is not bounded by the source's maxima
    i0 = torch.randn(N, H, W, C, generator=g).to(dtype)
    img = K.Act(i0.to(dev))
    K.batch_to_space(K.Act(y0.to(dev)), d, img, accumulate=True)
    assert torch.equal(img.buf.cpu(), i0 + b2s_ref(y0, d, H, W))


def test_layout_kernels_carry_amax(dev):
    K = _k()
    N, H, W, C, d = 2, 7, 9, 64, 2
    x = K.Act(torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(7)).to(dev))
    x.amax = K.amax(x)
    xs = K.Act(K.nhwc(*K.phase_shape(N, H, W, d), C, torch.float32, dev))
    K.space_to_batch(x, d, xs)
    assert xs.amax is x.amax
    K.check_amax(xs, "space_to_batch")
    y = K.Act(K.nhwc(N, H, W, C, torch.float32, dev))
    K.batch_to_space(xs, d, y)
    assert y.amax is x.amax
    K.check_amax(y, "batch_to_space")


# ---- the dilated layer -----------------------------------------------------------------------
LAYER_CASES = [
    # N, H, W, C, Cout, d
    (2, 12, 16, 64, 128, 2),
    (1, 9, 13, 128, 64, 2),     # ragged in both axes
    (1, 12, 18, 64, 64, 3),
    (1, 4, 512, 64, 64, 2),     # phase width 256: the fused 3-tap forward
]


def _operands(case, dtype, seed=0):
    N, H, W, C, Cout, d = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    gy = torch.randn(N, Cout, H, W, generator=g)
    if dtype != torch.float32:  # reference on the rounded operands
        x, w, gy = x.to(dtype).float(), w.to(dtype).float(), gy.to(dtype).float()
    return x, w, b, gy


def _layer(w, b, d, dev, bn=None, act=0):
    from dgvcc_amd import engine as E
    conv = nn.Conv2d(w.shape[1], w.shape[0], 3, padding=d, dilation=d)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    conv.to(dev)
    return E.ConvLayer(conv, bn, act)


def _run_layer(layer, x, gy, dtype, dev, drop=None, want_gx=True):
    """forward + backward of a ConvLayer on NCHW host operands -> (y, gx, grads) (y, gx NCHW f32 on host)."""
    K = _k()
    from dgvcc_amd import engine as E
    from dgvcc_amd import syncbn as SB
    E.invalidate_frozen()
    xd = K.Act(to_nhwc(x).to(dev, dtype))
    N, H, W = xd.N, xd.H, xd.W
    y = K.Act(torch.full((N, H, W, layer.Cout), float("nan"), dtype=dtype, device=dev))
    tape = {}
    layer.forward(xd, y, True, tape, drop=drop)
    SB.flush_batches()
    saved = tape[layer]
    gx = K.Act(torch.full((N, H, W, layer.Cin), float("nan"), dtype=dtype, device=dev)) if want_gx else None
    grads = layer.backward(tape, K.Act(to_nhwc(gy).to(dev, dtype)), gx)
    torch.cuda.synchronize()
    assert not tape  # everything the forward saved was consumed
    return to_nchw(y.buf.float()).cpu(), to_nchw(gx.buf.float()).cpu() if want_gx else None, grads, saved


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", LAYER_CASES)
def test_dilated_layer_matches_torch(dev, dtype, case):
    d = case[5]
    x, w, b, gy = _operands(case, dtype)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, padding=d, dilation=d)
    yr.backward(gy)
    layer = _layer(w, b, d, dev)
    y, gx, grads, _ = _run_layer(layer, x, gy, dtype, dev)
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    wtol = 2e-5 if dtype == torch.float32 else 2e-3  # f32 accumulation of 16-bit products
    errs = (relerr(y, yr.detach()), relerr(gx, xr.grad), relerr(grads[layer.conv.weight], wr.grad),
            relerr(grads[layer.conv.bias], br.grad))
    print(f"{case} {dtype}: fwd {errs[0]:.2e} dgrad {errs[1]:.2e} wgrad {errs[2]:.2e} bias {errs[3]:.2e}")
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    assert errs[0] < tol and errs[1] < tol
    assert errs[2] < wtol
    assert errs[3] < wtol  # a plain f32 sum of the (rounded) output gradient


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [LAYER_CASES[0], LAYER_CASES[1], LAYER_CASES[2]])
def test_dilated_layer_is_the_dense_layer_on_phases(dev, dtype, case):
    """Output and gradients are bit-identical to the dense ConvLayer (same weights) run on phase
    batches formed and un-formed on the host with torch indexing."""
    K = _k()
    from dgvcc_amd import engine as E
    N, H, W, C, Cout, d = case
    x, w, b, gy = _operands(case, dtype, seed=1)
    layer = _layer(w, b, d, dev, act=E.ACT_RELU)
    y, gx, grads, _ = _run_layer(layer, x, gy, dtype, dev)
    dense_conv = nn.Conv2d(C, Cout, 3, padding=1).to(dev)
    dense_conv.weight, dense_conv.bias = layer.conv.weight, layer.conv.bias
    dense = E.ConvLayer(dense_conv, None, E.ACT_RELU)
    xs = to_nchw(s2b_ref(to_nhwc(x), d))
    gs = to_nchw(s2b_ref(to_nhwc(gy), d))
    ys, gxs, grads0, _ = _run_layer(dense, xs, gs, dtype, dev)
    assert torch.equal(y, to_nchw(b2s_ref(to_nhwc(ys), d, H, W)))
    assert torch.equal(gx, to_nchw(b2s_ref(to_nhwc(gxs), d, H, W)))
    assert torch.equal(grads[layer.conv.weight], grads0[layer.conv.weight])
    assert torch.equal(grads[layer.conv.bias], grads0[layer.conv.bias])


def test_dilated_layer_accumulates_input_gradient(dev):
    K = _k()
    case = LAYER_CASES[1]
    N, H, W, C, Cout, d = case
    x, w, b, gy = _operands(case, torch.float32, seed=2)
    layer = _layer(w, b, d, dev)
    _, gx, _, _ = _run_layer(layer, x, gy, torch.float32, dev)
    g0 = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(3))
    acc = K.Act(g0.to(dev))
    tape = {}
    layer.forward(K.Act(to_nhwc(x).to(dev)), K.Act(K.nhwc(N, H, W, Cout, torch.float32, dev)), True, tape)
    layer.backward(tape, K.Act(to_nhwc(gy).to(dev)), acc, accumulate_gx=True)
    assert torch.equal(acc.buf.cpu(), g0 + to_nhwc(gx))


def test_dilated_layer_batchnorm_train(dev):
    """Conv(d=2) + BatchNorm2d(train) + ReLU in fp32 against float64 torch on the dilated conv, at
    the tolerances of test_fused_gpu: batch statistics of the stored z 1e-6 (mean) / 1e-5 (invstd,
    running variance), outputs 1e-5 given z -- here 2e-5, the conv's own bar, as z comes from the
    conv under test -- and gradients 1e-4."""
    from dgvcc_amd import engine as E
    case = LAYER_CASES[0]
    N, H, W, C, Cout, d = case
    x, w, b, gy = _operands(case, torch.float32, seed=24)
    g = torch.Generator().manual_seed(40)
    gam, bet = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    bn = nn.BatchNorm2d(Cout)
    with torch.no_grad():
        bn.weight.copy_(gam)
        bn.bias.copy_(bet)
    bn.to(dev).train()
    layer = _layer(w, b, d, dev, bn=bn, act=E.ACT_RELU)
    y, gx, grads, saved = _run_layer(layer, x, gy, torch.float32, dev)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    gr, btr = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    zr = F.conv2d(xr, wr, b.double(), padding=d, dilation=d)
    pre = F.batch_norm(zr, None, None, gr, btr, training=True, eps=bn.eps)
    # the reference is well conditioned: no pre-activation within the fp32 conv's error of the ReLU's kink
    assert pre.detach().abs().min().item() > 1e-5
    yr = F.relu(pre)
    yr.backward(gy.double())
    # the tape holds the phase batch of z; statistics do not depend on the order of the pixels
    _, z, stats, _, _, _ = saved
    assert (z.N, z.H, z.W) == (N * d * d, H // d, W // d)
    zf = z.buf.double().cpu().reshape(-1, Cout)
    assert relerr(stats[0], zf.mean(0)) < 1e-6
    assert relerr(stats[1], 1.0 / (zf.var(0, unbiased=False) + bn.eps).sqrt()) < 1e-5
    assert relerr(bn.running_var, 0.9 + 0.1 * zf.var(0, unbiased=True)) < 1e-5
    assert relerr(to_nchw(b2s_ref(z.buf.cpu(), d, H, W)), zr.detach()) < 2e-5
    assert relerr(y, yr.detach()) < 2e-5
    assert relerr(gx, xr.grad) < 1e-4
    assert relerr(grads[layer.conv.weight], wr.grad) < 1e-4
    assert relerr(grads[bn.weight], gr.grad) < 1e-4 and relerr(grads[bn.bias], btr.grad) < 1e-4


def test_dilated_layer_batchnorm_ragged_raises(dev):
    K = _k()
    case = LAYER_CASES[1]
    N, H, W, C, Cout, d = case
    x, w, b, _ = _operands(case, torch.float32)
    layer = _layer(w, b, d, dev, bn=nn.BatchNorm2d(Cout).to(dev).train(), act=1)
    with pytest.raises(ValueError, match="divisible"):
        layer.forward(K.Act(to_nhwc(x).to(dev)), K.Act(K.nhwc(N, H, W, Cout, torch.float32, dev)), True, {})


@pytest.mark.parametrize("case", [LAYER_CASES[0], LAYER_CASES[1]])
def test_dilated_layer_dropout_mask(dev, case):
    """The [N, C] Dropout2d channel mask is per image: every phase of an image takes its row."""
    N, H, W, C, Cout, d = case
    x, w, b, gy = _operands(case, torch.float32, seed=5)
    g = torch.Generator().manual_seed(50)
    mask = torch.empty(N, Cout).bernoulli_(0.5, generator=g) * 2.0
    mask[0, 0], mask[N - 1, 1] = 0.0, 2.0  # both values occur
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, b, padding=d, dilation=d) * mask[:, :, None, None]
    yr.backward(gy)
    layer = _layer(w, b, d, dev)
    y, gx, grads, _ = _run_layer(layer, x, gy, torch.float32, dev, drop=mask.to(dev))
    assert relerr(y, yr.detach()) < 2e-5 and relerr(gx, xr.grad) < 2e-5
    assert relerr(grads[layer.conv.weight], wr.grad) < 2e-5
    assert torch.equal(y[0, 0], torch.zeros(H, W))


# ---- ChainPlan: resident runs ------------------------------------------------------------------
def _chain(dev, seed=0, C=64, d=2, layers=3):
    from dgvcc_amd.models import plans2 as P2
    g = torch.Generator().manual_seed(seed)
    mods = []
    for _ in range(layers):
        conv = nn.Conv2d(C, C, 3, padding=d, dilation=d)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5)
            conv.bias.copy_(torch.randn(C, generator=g) * 0.1)
        mods += [conv, nn.ReLU(inplace=True)]
    seq = nn.Sequential(*mods).to(dev)
    return seq, P2.ChainPlan(seq)


def _run_chain(plan, x, gy, dev, counts=None):
    K = _k()
    from dgvcc_amd import engine as E
    E.invalidate_frozen()
    tape = {}
    y = plan.run(K.Act(x.to(dev)), torch.float32, True, tape)
    fwd = dict(counts) if counts is not None else None
    grads, gx = plan.back(tape, K.Act(gy.to(dev)))
    torch.cuda.synchronize()
    return y.buf.cpu(), gx.buf.cpu(), {p: v.cpu() for p, v in grads.items()}, fwd


@pytest.fixture
def launch_counts(monkeypatch):
    K = _k()
    counts = {}
    real = K.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(K, "call", counting)
    return counts


def test_chain_resident_equals_per_layer(dev, launch_counts):
    N, H, W, C = 2, 8, 12, 64
    g = torch.Generator().manual_seed(11)
    x, gy = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    seq, plan = _chain(dev)
    assert plan.resident
    y1, gx1, gr1, _ = _run_chain(plan, x, gy, dev)
    assert launch_counts["dg_space_to_batch"] == 2 and launch_counts["dg_batch_to_space"] == 2
    launch_counts.clear()
    plan.resident = False  # every layer converts by itself
    y0, gx0, gr0, _ = _run_chain(plan, x, gy, dev)
    assert launch_counts["dg_space_to_batch"] == 6 and launch_counts["dg_batch_to_space"] == 6
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0)
    assert set(gr1) == set(gr0) == set(seq.parameters())
    for p in gr1:
        assert torch.equal(gr1[p], gr0[p])
    # and both are the dilated chain
    ref = seq.double()(to_nchw(x.double().to(dev)))
    assert relerr(to_nchw(y1), ref.detach()) < 2e-5


def test_chain_ragged_takes_per_layer_path(dev, launch_counts):
    N, H, W, C = 2, 7, 9, 64
    g = torch.Generator().manual_seed(12)
    x, gy = torch.randn(N, H, W, C, generator=g), torch.randn(N, H, W, C, generator=g)
    seq, plan = _chain(dev, seed=3)
    y, gx, grads, fwd = _run_chain(plan, x, gy, dev, counts=launch_counts)
    assert fwd["dg_space_to_batch"] == 3 and fwd["dg_batch_to_space"] == 3  # by itself: 7x9 is ragged
    ref_seq = nn.Sequential(*[m for m in seq]).double()
    xr = to_nchw(x.double().to(dev)).requires_grad_(True)
    pre = []
    h = xr
    for m in ref_seq:
        h = m(h) if not isinstance(m, nn.ReLU) else F.relu(h)
        if isinstance(m, nn.Conv2d):
            pre.append(h.detach().abs().min().item())
    # no pre-activation within the fp32 error of the ReLU's kink (else a flipped decision, not an
    # arithmetic error, would decide the gradient comparison)
    assert min(pre) > 1e-5, pre
    h.backward(to_nchw(gy.double().to(dev)))
    assert relerr(to_nchw(y), h.detach()) < 2e-5
    assert relerr(to_nchw(gx), xr.grad) < 2e-5
    for p in seq.parameters():
        assert relerr(grads[p], p.grad) < 2e-5
