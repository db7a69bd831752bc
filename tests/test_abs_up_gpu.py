"""The two kernels under BL_VGG's tail on the GPU: dg_abs_fwd / dg_abs_bwd bit for bit against
torch.abs and g * torch.sign(z) (signed zeros, denormals, one element, sizes around a block and
beyond 1024 blocks, the accumulate flag), and the align-corners x2 upsampling at the 512 channels and
the 1x3 / 3x5 feature maps that BL_VGG's fixtures run, against F.interpolate in float64 at
test_kernels_gpu.py::test_upsample's tolerances.  The upsampling cases pin the existing kernel at
BL's shapes; the abs cases need the new entry points."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _abs_inputs(n, seed):
    """Mixed signs with +0.0, -0.0, denormals of both signs, the smallest normal and large values
    placed over a seeded normal draw (all of them as far as n reaches)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=g)
    gy = torch.randn(n, generator=g)
    special = torch.tensor([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 3e38, -3e38])
    k = min(n, len(special))
    z[:k] = special[:k]
    if n > 2 * len(special):  # special values in the last block's tail too, and denormal gradients
        z[-k:] = special.flip(0)
        gy[3], gy[4] = 1e-41, -1e-41
    return z, gy


@pytest.mark.parametrize("n", [1, 255, 257, 262149])
def test_abs_fwd_bwd_bit_equal(dev, n):
    from dgvcc_amd import kernels as K
    z, gy = _abs_inputs(n, seed=n)
    zd, gd = z.to(dev), gy.to(dev)
    y = K.abs_fwd(zd)
    gz = K.abs_bwd(zd, gd)
    torch.cuda.synchronize()
    want_y, want_g = torch.abs(z), gy * torch.sign(z)
    assert y.dtype == torch.float32 and y.shape == z.shape
    # bit patterns: -0.0 vs +0.0 and denormals count
    assert torch.equal(y.cpu().view(torch.int32), want_y.view(torch.int32))
    assert torch.equal(gz.cpu().view(torch.int32), want_g.view(torch.int32))
    assert torch.equal(zd.cpu().view(torch.int32), z.view(torch.int32))  # the input is left alone
    if n >= 2:
        assert gz[0].item() == 0.0 and gz[1].item() == 0.0  # sign(+-0) = 0


@pytest.mark.parametrize("n", [1, 257, 262149])
def test_abs_bwd_accumulates(dev, n):
    from dgvcc_amd import kernels as K
    z, gy = _abs_inputs(n, seed=n + 1)
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    acc = g0.clone().to(dev)
    out = K.abs_bwd(z.to(dev), gy.to(dev), acc, accumulate=True)
    assert out is acc
    want = g0 + gy * torch.sign(z)
    assert torch.equal(acc.cpu().view(torch.int32), want.view(torch.int32))
    # accumulate=0 overwrites whatever was there
    K.abs_bwd(z.to(dev), gy.to(dev), acc, accumulate=False)
    assert torch.equal(acc.cpu().view(torch.int32), (gy * torch.sign(z)).view(torch.int32))


def test_abs_matches_autograd_of_torch_abs(dev):
    """The pair is torch.abs's forward and gradient, zeros included (subgradient 0)."""
    from dgvcc_amd import kernels as K
    z, gy = _abs_inputs(1000, seed=3)
    zr = z.clone().requires_grad_(True)
    torch.abs(zr).backward(gy)
    gz = K.abs_bwd(z.to(dev), gy.to(dev))
    assert torch.equal(gz.cpu(), zr.grad)


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(1, 3), (3, 5)])
def test_align_corners_up2_at_512_channels(dev, dtype, H, W):
    from dgvcc_amd import kernels as K
    N, C, s = 2, 512, 2
    g = torch.Generator().manual_seed(17)
    x = torch.randn(N, C, H, W, generator=g).to(dtype)
    gy = torch.randn(N, C, H * s, W * s, generator=g).to(dtype)
    xr = x.double().requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=s, mode="bilinear", align_corners=True)
    yr.backward(gy.double())
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    y = K.Act(K.nhwc(N, H * s, W * s, C, dtype, dev))
    K.upsample_fwd(K.Act(nhwc(x).to(dev)), s, K.UP_BILINEAR_AC, y)
    gx = K.Act(K.nhwc(N, H, W, C, dtype, dev))
    K.upsample_bwd(K.Act(nhwc(gy).to(dev)), s, K.UP_BILINEAR_AC, gx)
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    e_f = _relerr(y.buf.float().permute(0, 3, 1, 2), yr.detach())
    e_b = _relerr(gx.buf.float().permute(0, 3, 1, 2), xr.grad)
    print(f"up2 align-corners C=512 {H}x{W} {dtype}: fwd {e_f:.2e} bwd {e_b:.2e} tol {tol:.0e}")
    assert e_f < tol and e_b < tol
    if H == 1:  # one source row: every output row is that row's interpolation along W
        assert torch.equal(y.buf[:, 0], y.buf[:, 1])
