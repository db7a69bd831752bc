"""dg_resize_crop_u8 / dg_resize_crop_f32 on one ragged batch of six samples (all source sizes
different): factors 0.75, 1.2499, 0.6 and 1.4, one axis unchanged, pre_resize 0.31 (15 bicubic taps
per output), a padded sample, grey on two samples, flip on three; downsample 1, 2 and 8; crops
(32, 48) and (64, 64), and (24, 304) with downsample 4, wider than one block's 256 columns.  Output
buffers are pre-filled with NaN.

* image: torch.equal against PIL resize -> pad -> crop -> hflip -> ToTensor/Normalize;
* density map: against restatement (b) of tests/resize_ref.py in float64, per sample within
  (2 (K + 2) + 2 + ds^2) * 2^-24 * max|d|, d the sample's source map and K its largest tap count.
  Derivation: the f32 weights (non-negative, summing to 1: no cancellation, every partial sum is
  bounded by max|d|) carry one rounding each, a pass adds K products and K - 1 sums, so a pass costs
  at most (K + 2) roundings of a value <= max|d|; two passes; two more for the f32 scalar and its
  product; one per term of the block sum.  Derived, not measured;
* the sum of each output map equals the source map's sum times the crop's share, within the same
  bound times the number of output pixels;
* two runs are bit-identical.
"""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as R

pytestmark = pytest.mark.gpu

F31 = 0.31 * 0.92  # a factor drawn under pre_resize 0.31: scale 3.5, 15 bicubic taps
# (24, 304): more than one 256-column tile per row, with a remainder, in both passes
CONFIGS = [((32, 48), 1), ((32, 48), 2), ((64, 64), 8), ((64, 64), 2), ((24, 304), 4)]


def _blobs(H, W, seed):
    """A sparse density map: unit-mass Gaussian blobs (f32), about one per 150 pixels."""
    rng = np.random.default_rng(seed)
    d = np.zeros((H, W), dtype=np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(max(3, H * W // 150)):
        x, y, s = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.8, 2.5)
        g = np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
        d += g / g.sum()
    return d.astype(np.float32)


def _specs(ch, cw):
    """(source h, w, resized nh, nw, crop corner rule, grey, flip) of the six samples."""
    up = lambda n, f: int(np.ceil(n / f)) + 1  # noqa: E731  a source size whose resize covers n
    return [
        dict(h=up(ch + 5, 0.75), w=up(cw + 9, 0.75), f=0.75, at="inside", grey=False, flip=True),
        dict(h=up(ch + 3, 1.2499), w=up(cw + 2, 1.2499), f=1.2499, at="topleft", grey=True, flip=False),
        dict(h=up(ch + 8, 0.6), w=up(cw + 1, 0.6), f=0.6, at="bottomright", grey=True, flip=True),
        dict(h=up(ch + 6, 1.4), w=cw + 7, f=1.4, keep_w=True, at="inside", grey=False, flip=False),
        dict(h=up(ch + 4, F31), w=up(cw + 3, F31), f=F31, at="inside", grey=False, flip=False),
        dict(h=up(ch - 7, 0.75), w=up(cw - 10, 0.75), f=0.75, at="padded", grey=False, flip=True),
    ]


@functools.lru_cache(maxsize=None)
def _case(crop, ds):
    """The batch (RawDenBatch) and its references, computed once: per sample the expected image
    [3,ch,cw] f32, the expected map float64 [ch/ds, cw/ds], the bound's K and max|d|, and the
    source sum times the crop's share."""
    from dgvcc_amd.datasets.den_dataset import collate_rescaled, make_sample
    from dgvcc_amd.utils.misc import get_padding
    ch, cw = crop
    samples, refs = [], []
    for n, sp in enumerate(_specs(ch, cw)):
        h, w, f = sp["h"], sp["w"], sp["f"]
        img = R.test_image(h, w, seed=100 * ch + n)
        dmap = _blobs(h, w, seed=200 * ch + n)
        nh, nw = int(h * f), (w if sp.get("keep_w") else int(w * f))
        left = top = 0
        ph, pw = nh, nw
        if sp["at"] == "padded":
            assert nh < ch and nw < cw
            (left, top, right, bottom), ph, pw = get_padding(nh, nw, ch, cw)
        else:
            assert nh > ch and nw > cw
        i, j = {"inside": ((ph - ch) // 2, (pw - cw) // 3), "topleft": (0, 0), "bottomright": (ph - ch, pw - cw),
                "padded": (0, 0)}[sp["at"]]
        samples.append(make_sample(img, dmap, nh, nw, left, top, i, j, crop, ds, sp["grey"], sp["flip"], True,
                                   torch.zeros(0, 2)))
        # whole-frame references
        pil = Image.fromarray(img)
        if sp["grey"]:
            pil = pil.convert("L").convert("RGB")
        arr = np.asarray(pil.resize((nw, nh)))
        d64 = dmap.astype(np.float64)
        res = R.aa_bilinear_resize(d64, nh, nw)
        res = res * (d64.sum() / res.sum())
        if sp["at"] == "padded":
            arr = np.pad(arr, ((top, bottom), (left, right), (0, 0)))
            res = np.pad(res, ((top, bottom), (left, right)))
        arr, res = arr[i:i + ch, j:j + cw], res[i:i + ch, j:j + cw]
        share = res.sum() / d64.sum()
        if sp["flip"]:
            arr = arr[:, ::-1]
        K = max(samples[-1].map_hw.shape[1], samples[-1].map_vw.shape[1])
        refs.append(dict(img=R.normalise(arr), map=R.block_sum_flip(res, ds, sp["flip"]), K=K,
                         dmax=float(np.abs(d64).max()), mass=float(d64.sum() * share),
                         taps=max(samples[-1].img_hw.shape[1], samples[-1].img_vw.shape[1])))
    return collate_rescaled(samples), refs


def _run(raw, dev):
    """Both kernels into NaN-filled outputs."""
    from dgvcc_amd.datasets.augment import resize_crop_f32, resize_crop_u8
    B, (ch, cw), ds = raw.img_desc.shape[0], raw.crop_size, raw.downsample
    imgs = torch.full((B, 3, ch, cw), float("nan"), device=dev)
    dmaps = torch.full((B, 1, ch // ds, cw // ds), float("nan"), device=dev)
    resize_crop_u8(raw.img_src, raw.img_desc, raw.img_bounds, raw.img_weights, raw.crop_size, dev, out=imgs)
    resize_crop_f32(raw.map_src, raw.map_desc, raw.map_bounds, raw.map_weights, raw.scales, raw.crop_size, ds, dev,
                    out=dmaps)
    torch.cuda.synchronize()
    return imgs, dmaps


def test_batch_is_ragged_and_covers_the_cases():
    raw, refs = _case((64, 64), 8)
    d = raw.img_desc
    sizes = {(int(r[1]), int(r[2])) for r in d}
    assert len(sizes) == 6
    assert int(d[:, 13].sum()) == 2 and int(d[:, 14].sum()) == 3  # grey on two, flip on three
    assert refs[4]["taps"] == 15 and refs[3]["taps"] > 1
    assert int(d[3, 9]) == 1  # the unchanged axis: identity taps
    assert int(d[5, 5]) > 0 and int(d[5, 6]) > 0  # the padded sample starts inside the crop


@pytest.mark.parametrize("crop,ds", CONFIGS)
def test_image_bit_exact(dev, crop, ds):
    raw, refs = _case(crop, ds)
    imgs, _ = _run(raw, dev)
    imgs = imgs.cpu()
    assert not torch.isnan(imgs).any()
    for n, ref in enumerate(refs):
        assert torch.equal(imgs[n], ref["img"]), f"sample {n}: {(imgs[n] != ref['img']).sum().item()} pixels differ"


@pytest.mark.parametrize("crop,ds", CONFIGS)
def test_density_map_within_derived_bound(dev, crop, ds):
    raw, refs = _case(crop, ds)
    _, dmaps = _run(raw, dev)
    dmaps = dmaps.cpu().double().numpy()
    assert dmaps.shape == (6, 1, crop[0] // ds, crop[1] // ds) and np.isfinite(dmaps).all()
    for n, ref in enumerate(refs):
        bound = (2 * (ref["K"] + 2) + 2 + ds * ds) * 2.0 ** -24 * ref["dmax"]
        err = np.abs(dmaps[n, 0] - ref["map"]).max()
        serr = abs(dmaps[n, 0].sum() - ref["mass"])
        print(f"crop {crop} ds {ds} sample {n}: K {ref['K']} err {err:.3e} bound {bound:.3e} "
              f"sum err {serr:.3e} bound {bound * dmaps[n, 0].size:.3e}")
        assert err <= bound
        assert serr <= bound * dmaps[n, 0].size


def test_two_runs_bit_identical(dev):
    raw, _ = _case((64, 64), 2)
    a = _run(raw, dev)
    b = _run(raw, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refuses_inconsistent_descriptors(dev):
    """The library checks every descriptor against the buffer extents before any launch."""
    import dataclasses
    from dgvcc_amd._capi import DGError
    from dgvcc_amd.datasets.augment import resize_crop_u8
    raw, _ = _case((32, 48), 1)
    for col, val in ((1, 10 ** 6), (4, 10 ** 6), (7, 10 ** 7), (9, 49), (5, 40)):
        desc = raw.img_desc.clone()
        desc[2, col] = val
        bad = dataclasses.replace(raw, img_desc=desc)
        with pytest.raises(DGError):
            resize_crop_u8(bad.img_src, bad.img_desc, bad.img_bounds, bad.img_weights, bad.crop_size, dev)
