"""Small-channel k x k convolution on the GPU: engine.SmallConvLayer against
F.conv2d in float64 on the host, on the dtype-rounded operands, for the twelve MCNN forms and the
edges of the family, at the tolerances of test_dilation_gpu.test_dilated_layer_matches_torch.

Sizes: 8x8 (smaller than a 9x9 footprint, one partial tile), 9x11 (odd in both axes) and 19x69: the
tile is 8 rows x 32 columns (fewer rows where the LDS budget asks for it), so 19x69 has two full
tiles plus a ragged remainder in both axes and a weight-gradient strip crosses the image boundary.
Output buffers are pre-filled with NaN; the padded channels of y and dx must come back exactly zero.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_dilation_gpu import relerr, to_nchw, to_nhwc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MCNN_FORMS = [(3, 16, 9), (16, 32, 7), (32, 16, 7), (16, 8, 7),
              (3, 20, 7), (20, 40, 5), (40, 20, 5), (20, 10, 5),
              (3, 24, 5), (24, 48, 3), (48, 24, 3), (24, 12, 3)]
FORMS = MCNN_FORMS + [(64, 64, 9), (1, 1, 1), (30, 8, 1)]
SIZES = [(8, 8), (9, 11), (19, 69)]
N = 2


def _k():
    from dgvcc_amd import kernels as K
    return K


def _operands(form, size, dtype, seed=0):
    C, Cout, k = form
    H, W = size
    g = torch.Generator().manual_seed(seed + 17 * C + 31 * Cout + k + 7 * H)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    rd = lambda t: t.to(dtype).double()  # noqa: E731  (the value the kernels read)
    x, gy = rd(r(N, C, H, W)), rd(r(N, Cout, H, W))
    w = rd(r(Cout, C, k, k) / (C * k * k) ** 0.5)
    b = r(Cout).double()
    return x, w, b, gy


def _layer(w, b, dev, act):
    from dgvcc_amd import engine as E
    Cout, C, k, _ = w.shape
    conv = nn.Conv2d(C, Cout, k, padding=k // 2).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.copy_(b.float())
    return E.SmallConvLayer(conv, None, act)


def _padded(t, Cp, dtype, dev):
    """NCHW host tensor -> NHWC Act with the channels zero-padded to Cp."""
    K = _k()
    n, c, h, w = t.shape
    buf = torch.zeros((n, h, w, Cp), dtype=dtype, device=dev)
    buf[..., :c] = to_nhwc(t).to(dev, dtype)
    return K.Act(buf)


def _nan(n, h, w, c, dtype, dev):
    return _k().Act(torch.full((n, h, w, c), float("nan"), dtype=dtype, device=dev))


def _run_layer(layer, x, gy, dtype, dev, want_gx=True):
    """forward + backward on NCHW host operands -> (y, gx, grads, the padded lanes of y and gx)."""
    from dgvcc_amd import engine as E
    E.invalidate_frozen()
    n, _, h, w = x.shape
    xd = _padded(x, layer.Cp_in, dtype, dev)
    y = _nan(n, h, w, layer.Cp_out, dtype, dev)
    tape = {}
    layer.forward(xd, y, True, tape)
    gx = _nan(n, h, w, layer.Cp_in, dtype, dev) if want_gx else None
    grads = layer.backward(tape, _padded(gy, layer.Cp_out, dtype, dev), gx)
    torch.cuda.synchronize()
    assert not tape  # everything the forward saved was consumed
    pads = [y.buf[..., layer.Cout:]] + ([gx.buf[..., layer.Cin:]] if want_gx else [])
    return (to_nchw(y.buf[..., :layer.Cout].float()).cpu(),
            to_nchw(gx.buf[..., :layer.Cin].float()).cpu() if want_gx else None, grads, pads)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{f[0]}-{f[1]}-k{f[2]}")
def test_small_layer_matches_torch(dev, form, size, dtype):
    from dgvcc_amd import engine as E
    C, Cout, k = form
    x, w, b, gy = _operands(form, size, dtype)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, padding=k // 2)
    yr.backward(gy)
    layer = _layer(w, b, dev, E.ACT_NONE)
    y, gx, grads, pads = _run_layer(layer, x, gy, dtype, dev)
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    wtol = 2e-5 if dtype == torch.float32 else 2e-3  # f32 accumulation of 16-bit products
    gw, gb = grads[layer.conv.weight], grads[layer.conv.bias]
    assert gw.dtype == torch.float32 and tuple(gw.shape) == (Cout, C, k, k) and tuple(gb.shape) == (Cout,)
    errs = (relerr(y, yr.detach()), relerr(gx, xr.grad), relerr(gw, wr.grad), relerr(gb, br.grad))
    print(f"{form} {size} {dtype}: fwd {errs[0]:.2e} dgrad {errs[1]:.2e} wgrad {errs[2]:.2e} bias {errs[3]:.2e}")
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    for p in pads:  # the padded channels hold exact zeros, whatever the buffers held before
        assert p.numel() == 0 or bool((p == 0).all())
    assert errs[0] < tol and errs[1] < tol
    assert errs[2] < wtol
    assert errs[3] < wtol


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("form", [(3, 16, 9), (40, 20, 5), (24, 12, 3)], ids=lambda f: f"{f[0]}-{f[1]}-k{f[2]}")
def test_small_layer_relu(dev, form, dtype):
    """With the ReLU: y = relu(conv), and the backward is the linear backward of the gradient masked
    by the layer's own output (so a near-zero pre-activation cannot disagree on its sign)."""
    from dgvcc_amd import engine as E
    C, Cout, k = form
    x, w, b, gy = _operands(form, (9, 11), dtype, seed=3)
    layer = _layer(w, b, dev, E.ACT_RELU)
    y, gx, grads, pads = _run_layer(layer, x, gy, dtype, dev)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    zr = F.conv2d(xr, wr, br, padding=k // 2)
    zr.backward(gy * (y > 0).double())
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    wtol = 2e-5 if dtype == torch.float32 else 2e-3
    assert relerr(y, zr.detach().clamp_min(0)) < tol and bool((y >= 0).all())
    assert relerr(gx, xr.grad) < tol
    assert relerr(grads[layer.conv.weight], wr.grad) < wtol and relerr(grads[layer.conv.bias], br.grad) < wtol
    for p in pads:
        assert p.numel() == 0 or bool((p == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("form", [(16, 32, 7), (3, 24, 5), (64, 64, 9)], ids=lambda f: f"{f[0]}-{f[1]}-k{f[2]}")
def test_weight_gradient_is_bit_identical_from_run_to_run(dev, form, dtype):
    K = _k()
    C, Cout, k = form
    x, _, _, gy = _operands(form, (19, 69), dtype, seed=5)
    xd, gd = _padded(x, K.cpad8(C), dtype, dev), _padded(gy, K.cpad8(Cout), dtype, dev)
    out = []
    for _ in range(2):
        dw = torch.full((Cout, C, k, k), float("nan"), dtype=torch.float32, device=dev)
        db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=dev)
        K.smallconv_wgrad(xd, gd, C, Cout, k, dw, db)
        out.append((dw, db))
    torch.cuda.synchronize()
    assert torch.isfinite(out[0][0]).all() and torch.isfinite(out[0][1]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_small_layer_without_input_gradient_or_bias(dev):
    """The Cin = 3 layers take no input gradient; a bias-free convolution returns no bias gradient."""
    from dgvcc_amd import engine as E
    form, dtype = (3, 16, 9), torch.float32
    x, w, b, gy = _operands(form, (9, 11), dtype, seed=9)
    conv = nn.Conv2d(3, 16, 9, padding=4, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.float())
    layer = E.SmallConvLayer(conv, None, E.ACT_NONE)
    wr = w.clone().requires_grad_(True)
    F.conv2d(x, wr, None, padding=4).backward(gy)
    y, gx, grads, _ = _run_layer(layer, x, gy, dtype, dev, want_gx=False)
    assert gx is None and list(grads) == [conv.weight]
    assert relerr(y, F.conv2d(x, w, None, padding=4)) < 2e-5
    assert relerr(grads[conv.weight], wr.grad) < 2e-5


def test_image_layout_pass(dev):
    K = _k()
    img = torch.randn(2, 3, 9, 11, generator=torch.Generator().manual_seed(1))
    for dtype in DTYPES:
        y = K.image_nhwc_pad(img.to(dev), dtype)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (2, 9, 11, 8) and y.dtype == dtype
        assert torch.equal(y[..., :3].cpu(), to_nhwc(img).to(dtype)) and bool((y[..., 3:] == 0).all())


@pytest.mark.parametrize("conv", [nn.Conv2d(3, 8, 11, padding=5), nn.Conv2d(65, 8, 3, padding=1),
                                  nn.Conv2d(8, 8, 3, stride=2, padding=1)], ids=["k11", "C65", "stride2"])
def test_outside_the_family_raises_before_any_launch(dev, conv, monkeypatch):
    from dgvcc_amd import engine as E
    K = _k()
    calls = []
    monkeypatch.setattr(K, "call", lambda name, *a: calls.append(name))
    with pytest.raises(ValueError, match="in_channels="):
        E.SmallConvLayer(conv.to(dev), None, E.ACT_RELU)
    with pytest.raises(ValueError, match="BatchNorm"):
        E.SmallConvLayer(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), E.ACT_RELU)
    assert not calls
    # the C-ABI itself refuses the form too, before any launch (-2 = DG_ERR_UNSUPPORTED)
    k, s = conv.kernel_size[0], conv.stride[0]
    buf = torch.zeros(2, 8, 8, 72, device=dev)
    st = K.lib_call_status("dg_smallconv_fwd", 0, buf.data_ptr(), 72, 2, 8, 8, conv.in_channels, buf.data_ptr(),
                           conv.out_channels, k, k, s, conv.padding[0], 1, None, 0, buf.data_ptr(), 72, K.stream())
    assert st == -2
