"""The restatements of tests/resize_ref.py against their yardsticks: (a) PIL `Image.resize` bit for
bit, (b) `F.interpolate(mode='bilinear', antialias=True)` in float64 within 1e-12, the sum identity
behind the renormalisation scalar, and the host's vectorised tap tables against both."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import resize_ref as R


def _sizes(H, W, f):
    return int(H * f), int(W * f)


def _dmap(H, W, seed):
    rng = np.random.default_rng(seed)
    d = rng.random((H, W)) ** 4
    d[H // 3:H // 2, W // 4:W // 2] = 0.0
    return d


@pytest.mark.parametrize("H,W,f", R.CASES)
def test_pil_bicubic_bit_exact(H, W, f):
    img = R.test_image(H, W, seed=H * 1000 + W)
    assert (img == 255).any() and (img == 0).any()
    nh, nw = _sizes(H, W, f)
    want = np.asarray(Image.fromarray(img).resize((nw, nh)))
    got = R.pil_bicubic_resize(img, nh, nw)
    assert got.shape == want.shape
    assert int((got != want).sum()) == 0
    if (nh, nw) == (H, W):
        assert np.array_equal(got, img)  # no pass


@pytest.mark.parametrize("H,W,f", R.CASES)
def test_aa_bilinear_float64(H, W, f):
    d = _dmap(H, W, seed=H + W)
    nh, nw = _sizes(H, W, f)
    want = F.interpolate(torch.from_numpy(d)[None, None], size=(nh, nw), mode="bilinear", align_corners=False,
                         antialias=True)[0, 0].numpy()
    got = R.aa_bilinear_resize(d, nh, nw)
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("H,W,f", R.CASES)
def test_sum_identity(H, W, f):
    d = _dmap(H, W, seed=3 * H + W)
    nh, nw = _sizes(H, W, f)
    total = R.aa_bilinear_resize(d, nh, nw).sum()
    ident = R.axis_sums(H, nh) @ d @ R.axis_sums(W, nw)
    assert abs(ident - total) <= 1e-12 * abs(total)


@pytest.mark.parametrize("H,W,f", R.CASES)
def test_host_tap_tables(H, W, f):
    """dgvcc_amd.datasets.den_dataset's vectorised tables equal the per-sample loops: the fixed-point
    bicubic weights exactly, the triangle weights exactly, the tap sums within rounding."""
    from dgvcc_amd.datasets import den_dataset as DD
    for n_in, n_out in ((H, int(H * f)), (W, int(W * f))):
        for kind, filt, sup in (("bicubic", R.bicubic, 2.0), ("triangle", R.triangle, 1.0)):
            start, count, w = DD.tap_table(n_in, n_out, 0, n_out, kind)
            if n_in == n_out:
                assert np.array_equal(start, np.arange(n_out)) and (count == 1).all() and (w == 1.0).all()
                continue
            ref = R.coeffs(n_in, n_out, filt, sup)
            assert [int(s) for s in start] == [m for m, _ in ref]
            assert [int(c) for c in count] == [len(k) for _, k in ref]
            for n, (_, k) in enumerate(ref):
                assert np.array_equal(w[n, :len(k)], np.array(k)) and (w[n, len(k):] == 0).all()
                if kind == "bicubic":
                    assert DD.fixed_point(w[n, :len(k)]).tolist() == [R.to_fixed(x) for x in k]
        assert np.abs(DD.tap_sums(n_in, n_out, "triangle") - R.axis_sums(n_in, n_out)).max() <= 1e-14
