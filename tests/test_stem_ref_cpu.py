"""The float64 restatements of tests/stem_ref.py against F.conv2d and torch.nn.grad.conv2d_weight in float64, and
the conditions the case builders promise for every shape of tests/test_stem_kernels_gpu.py (segment walk, part
counts, planted borders, ReLU margin), so that a failure there cannot be blamed on its inputs.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
import stem_ref as SR

TOL = 1e-10
E = 2.0 ** -24
SHAPE_IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def _close(a, b, what=""):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), (what, err)


@pytest.mark.parametrize("shape", SR.SMALL + SR.BWD_ONLY, ids=SHAPE_IDS)
def test_conv_and_wgrad_against_torch(shape):
    i = SR.make_case(*shape)
    img, w, b = i["img"].double(), i["w"].double(), i["bias"].double()
    z, a = SR.conv(img, w, b)
    _close(z, F.conv2d(img, w, b, padding=1).permute(0, 2, 3, 1), "conv")
    _close(a, F.conv2d(img.abs(), w.abs(), b.abs(), padding=1).permute(0, 2, 3, 1), "conv |terms|")
    z0, a0 = SR.conv(img, w, None)
    _close(z0, z - b, "conv without bias")
    dz = i["g"].double()
    dw, da = SR.wgrad(img, dz)
    _close(dw, torch.nn.grad.conv2d_weight(img, (64, 3, 3, 3), dz.permute(0, 3, 1, 2), padding=1), "wgrad")
    _close(da, torch.nn.grad.conv2d_weight(img.abs(), (64, 3, 3, 3), dz.abs().permute(0, 3, 1, 2), padding=1),
           "wgrad |terms|")
    assert (a >= z.abs() - 1e-12).all() and (da >= dw.abs() - 1e-9).all()


@pytest.mark.parametrize("shape,width", [((2, 3, 128), 64), ((1, 4, 96), 32), ((2, 3, 32), 32)], ids=str)
def test_segments_tile_the_pixels_and_localise_wgrad(shape, width):
    N, H, W = shape
    nseg = N * H * (W // width)
    pix = torch.cat([SR.segment_pixels(N, H, W, s, width) for s in range(nseg)])
    assert torch.equal(pix, torch.arange(N * H * W)), "segments in order cover every pixel once"
    i = SR.make_case(*shape)
    seg = nseg - 2
    p = SR.segment_pixels(N, H, W, seg, width)
    dz = torch.zeros(N * H * W, 64, dtype=torch.float64)
    dz[p] = i["g"].double().reshape(-1, 64)[p]
    dw, da = SR.wgrad(i["img"], dz.reshape(N, H, W, 64))
    dw2, da2 = SR.wgrad_pixels(i["img"], p, dz[p])
    _close(dw2, dw, "wgrad_pixels")
    _close(da2, da, "wgrad_pixels |terms|")


@pytest.mark.parametrize("shape", SR.FWD_SHAPES, ids=SHAPE_IDS)
def test_part_counts(shape):
    N, H, W = shape
    n = SR.part_counts(N, H, W)
    nseg = N * H * (W // 64)
    assert n.sum().item() == N * H * W
    assert n.numel() == SR.fwd_grid(nseg) and (n % 64 == 0).all()
    walked = sorted(s for b in range(n.numel()) for w in range(4) for s in SR.wave_segments(nseg, b, w))
    assert walked == list(range(nseg))
    for b in (0, n.numel() - 1):
        assert n[b].item() == 64 * sum(len(SR.wave_segments(nseg, b, w)) for w in range(4))


def test_long_shape_takes_the_paths_it_is_there_for():
    N, H, W = SR.LONG
    fseg, bseg = N * H * (W // 64), N * H * (W // 32)
    per_f = {len(SR.wave_segments(fseg, b, w)) for b in range(512) for w in range(4)}
    per_b = {len(SR.wave_segments(bseg, b, w)) for b in range(512) for w in range(4)}
    per_a = {len(SR.wave_segments(fseg, b, w, 1024)) for b in range(1024) for w in range(4)}
    assert per_f == {2, 3} and per_b == {4, 5} and per_a == {1, 2}
    assert 0 < (H * (W // 64)) % (4 * 512) and 0 < (H * (W // 32)) % (4 * 512)  # the image boundary falls mid-grid
    for shape in SR.SMALL[:1]:  # (1, 1, 64): one segment, three waves of block 0 without work
        assert SR.part_counts(*shape).tolist() == [64.0]


@pytest.mark.parametrize("dt", [SR.F32, SR.BF16], ids=lambda d: R.IDS[d])
@pytest.mark.parametrize("shape", SR.SMALL + SR.BWD_ONLY, ids=SHAPE_IDS)
def test_planted_borders_dominate_the_bound(shape, dt):
    """Every wrong halo rule moves z, at the pixels it touches, by more than k times the per-element bound in at
    least 90% of the ordinary channels' elements (a channel whose filter taps happen to cancel on a border stays
    below) and by 10 k in the median (k = 100 in f32, 10 in bf16, whose
    bound holds an ulp of |z|): rows / columns taken for padding, and the neighbouring image's rows read where
    the padding belongs."""
    i = SR.make_case(*shape)
    N, H, W = shape
    img, w, b = SR.rounded(i["img"], dt), SR.rounded(i["w"], dt), i["bias"].double()
    z, a = SR.conv(img, w, b)
    bound = 32 * E * a + (E if dt == SR.F32 else 2.0 ** -8) * z.abs()
    ordinary = [c for c in range(64) if c not in (SR.CH_ZERO, SR.CH_BIAS100)]
    k = 100 if dt == SR.F32 else 10

    def dominated(zv, rows, cols, what):
        d = ((zv - z).abs() / bound)[..., ordinary]
        if rows is not None:
            d = d[:, rows]
        if cols is not None:
            d = d[:, :, cols]
        frac = (d > k).double().mean().item()
        assert frac >= 0.9 and d.median().item() > 10 * k, (what, frac, d.median().item())

    for v in SR.wrong_halo_variants(img):
        dominated(SR.conv(v.img, w, b)[0], v.rows, v.cols, v.name)
    if N > 1:  # the images stacked into one tall image: no padding between them
        tall = img.permute(1, 0, 2, 3).reshape(1, 3, N * H, W)
        zt = SR.conv(tall, w, b)[0].reshape(N, H, W, 64)
        d = ((zt - z).abs() / bound)[..., ordinary]
        inner = torch.cat([d[1:, 0].reshape(-1), d[:-1, H - 1].reshape(-1)])
        assert (inner > k).double().mean().item() >= 0.9, "neighbouring image"


@pytest.mark.parametrize("dt", [SR.F32, SR.BF16], ids=lambda d: R.IDS[d])
@pytest.mark.parametrize("shape", SR.BWD_SHAPES, ids=SHAPE_IDS)
def test_relu_margin(shape, dt):
    """At most 1 in 10^5 of the (pixel, channel) elements of a case within 2^-23 (|z scale| + |shift|) of the
    ReLU's zero (the zero-filter channel: constant, at least 0.5 away), on float64 z rounded to the storage
    type and its float64 statistics; the synthetic rows of the localisation tests keep every element active."""
    z, st, scale, shift = SR.ref_stats(shape, dt)
    ok, n, total = SR.margin_ok(z, scale, shift)
    print(f"  {shape} {R.IDS[dt]}: {n} uncertain of {total}")
    assert ok, (n, total)
    zs, sf = R.pre(z, scale, shift)
    assert ((zs + sf)[:, SR.CH_ZERO].abs() >= 0.5).all()
    assert st["var"][SR.CH_ZERO].item() == 0.0
    active = z.double() + 1000.0  # scale 1, shift 1000 of the localisation tests
    assert (active > 500).all()
    # the planted channels are what they claim
    i = SR.make_case(*shape)
    assert not i["w"][SR.CH_ZERO].any() and i["bias"][SR.CH_BIAS100] == 100 and i["bias"][SR.CH_NOBIAS] == 0
    assert i["gamma"][SR.CH_NEGGAMMA] < 0 and (i["gamma"].abs() >= 0.5).all()
