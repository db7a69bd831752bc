"""Drop-in `datasets.den_dataset.DensityMapDataset` (reference datasets/den_dataset.py over
datasets/base_dataset.py), the training set of the baseline counters, with its random rescale
moved to the GPU (resize.hip).

What sets it apart from DenClsDataset is the rescale (den_dataset.py:65-79): per sample a factor
`pre_resize * (random() * 0.5 + 0.75)` is drawn, the image is resized with PIL's `resize`
(bicubic), the density map with torchvision's tensor `resize` and renormalised to its sum, and
the result is padded, cropped, block-summed and flipped.  Both resamplers are separable: an output
column (row) is a short weighted sum of input columns (rows).  So the host half

* makes the reference's Python-`random` draws in the reference's order (grey, factor,
  `get_padding`, `random_crop`, flip);
* builds the tap tables in float64 for the rows and columns of the crop only (`tap_table`):
  PIL's bicubic with its 22-bit fixed-point weights for the image, the antialiased triangle of
  `interpolate(mode='bilinear', align_corners=False, antialias=True)` (current torchvision's
  tensor `resize`) for the density map;
* slices the source windows those taps touch out of the decoded image and the density map;
* transforms the points;
* computes the renormalisation scalar `dmap_sum / resized_sum` in float64 without resizing the
  map: with cx / cy the column / row sums of the full tap tables, the resized map sums to
  `cy @ d @ cx`.  Where that sum is 0 (a frame with no people) the reference computes
  0 * 0 / 0 = NaN; here the scalar is 0 and the map stays zero.

Per-pixel work is left to `dg_resize_crop_u8` / `dg_resize_crop_f32`: `collate` packs the samples
into a `RawDenBatch`, which `DGTrainer.train_step` (mode 'simple') or `DeviceAugment` turns into
`(imgs, imgs, (points, dmaps, <empty>))` on the device.

Train files: `<name>_dmap2.npy` unless `gt_dir` is given.  Val/test samples are
DenClsDataset._val_transform's.
"""
from __future__ import annotations

import random
from typing import NamedTuple

import numpy as np
import torch

from ..utils.misc import get_padding, random_crop
from .augment import RESIZE_DESC, RawDenBatch
from .den_cls_dataset import DenClsDataset

PRECISION_BITS = 22  # PIL Resample.c: 32 - 8 - 2


def _bicubic(x):
    """PIL bicubic_filter (a = -0.5)."""
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _triangle(x):
    """ATen's antialias bilinear filter."""
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


_FILTERS = {"bicubic": (_bicubic, 2.0), "triangle": (_triangle, 1.0)}


def tap_table(n_in: int, n_out: int, lo: int, hi: int, kind: str):
    """Taps of output indices [lo, hi) of a resize from n_in to n_out samples along one axis:
    (start int64 [n], count int64 [n], weights float64 [n, K], zero past each count).  PIL's
    precompute_coeffs and ATen's _compute_indices_weights_aa share the window arithmetic; the
    weights are normalised in double in tap order.  An axis that keeps its size is not resampled
    (PIL skips the pass, torchvision returns its input; the triangle's own taps there are 1 and 0):
    identity taps."""
    if n_out <= 0 or n_in <= 0:
        raise ValueError(f"cannot resize {n_in} samples to {n_out}")
    xx = np.arange(lo, hi, dtype=np.int64)
    if n_in == n_out:
        return xx.copy(), np.ones(len(xx), np.int64), np.ones((len(xx), 1), np.float64)
    filt, support = _FILTERS[kind]
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ss = 1.0 / filterscale
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # C casts truncate
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    count = xmax - xmin
    K = int(count.max()) if len(xx) else 1
    k = np.arange(K, dtype=np.int64)
    w = filt(((k[None, :] + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where(k[None, :] < count[:, None], w, 0.0)
    ww = np.zeros(len(xx), np.float64)
    for j in range(K):  # the C loops add in tap order
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    return xmin, count, w


def fixed_point(w: np.ndarray) -> np.ndarray:
    """PIL normalize_coeffs_8bpc: round half away from zero to 22 fractional bits."""
    s = w * (1 << PRECISION_BITS)
    return np.where(w < 0, np.trunc(-0.5 + s), np.trunc(0.5 + s)).astype(np.int32)


def tap_sums(n_in: int, n_out: int, kind: str) -> np.ndarray:
    """[n_in] float64: how much each input sample contributes to the sum over all n_out outputs."""
    start, count, w = tap_table(n_in, n_out, 0, n_out, kind)
    idx = np.minimum(start[:, None] + np.arange(w.shape[1])[None, :], n_in - 1)
    return np.bincount(idx.ravel(), weights=w.ravel(), minlength=n_in)


class AxisTaps(NamedTuple):
    lo: int               # first source index the taps touch
    hi: int               # one past the last
    bounds: np.ndarray    # int32 [n, 2]: (start relative to lo, count)
    weights: np.ndarray   # float64 [n, K]


def axis_taps(n_in, n_out, lo, hi, kind) -> AxisTaps:
    start, count, w = tap_table(n_in, n_out, lo, hi, kind)
    a, b = int(start.min()), int((start + count).max())
    return AxisTaps(a, b, np.stack([start - a, count], 1).astype(np.int32), w)


class DenSample(NamedTuple):
    """One training sample before its pixel work.  geom = (r0, c0, oh, ow, grey, flip, ch, cw,
    downsample): the oh x ow pixels of the ch x cw crop from (r0, c0) lie inside the resized frame,
    the rest is padding."""
    img_win: torch.Tensor      # uint8 [sh, sw, 3]
    img_hb: torch.Tensor       # int32 [ow, 2]
    img_hw: torch.Tensor       # int32 [ow, kh]
    img_vb: torch.Tensor       # int32 [oh, 2]
    img_vw: torch.Tensor       # int32 [oh, kv]
    map_win: torch.Tensor      # [mh, mw] in the file's dtype
    map_hb: torch.Tensor
    map_hw: torch.Tensor       # f64
    map_vb: torch.Tensor
    map_vw: torch.Tensor       # f64
    geom: torch.Tensor         # int32 [9]
    scale: float
    points: torch.Tensor       # f32 [n, 2]


def _t(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C"))  # a copy: the decoded image is read-only


def rescale_train_transform(ds, img, gt, dmap) -> DenSample:
    """Host half of the reference's _train_transform (den_dataset.py:55-128): the same
    Python-`random` calls in the same order, O(points) and O(window) work."""
    h, w = img.shape[:2]
    ch, cw = ds.crop_size
    grey = random.random() > 0.88
    factor = ds.pre_resize * (random.random() * 0.5 + 0.75)
    nh, nw = h, w
    if factor != 1.0:  # no minimum-size check in these two datasets
        nw, nh = int(w * factor), int(h * factor)
        gt = gt * factor
    ph, pw, left, top = nh, nw, 0, 0
    if 1.0 * min(nw, nh) < min(ch, cw):
        (left, top, _, _), ph, pw = get_padding(nh, nw, ch, cw)
        if len(gt) > 0:
            gt = gt + [left, top]
    i, j = random_crop(ph, pw, ch, cw)
    if len(gt) > 0:
        gt = gt - [j, i]
        gt = gt[(gt[:, 0] >= 0) * (gt[:, 0] <= cw) * (gt[:, 1] >= 0) * (gt[:, 1] <= ch)]
    else:
        gt = np.empty([0, 2])
    if len(gt) > 0:
        gt = gt / ds.downsample
    flip = random.random() > 0.5
    if flip and len(gt) > 0:
        gt[:, 0] = cw - gt[:, 0]

    return make_sample(img, dmap, nh, nw, left, top, i, j, (ch, cw), ds.downsample, grey, flip, factor != 1.0,
                       torch.from_numpy(gt.copy()).float())


def make_sample(img, dmap, nh, nw, left, top, i, j, crop_size, downsample, grey, flip, renorm, points) -> DenSample:
    """The sample of one geometry: the frame (img uint8 [h,w,3], dmap [h,w]) resized to nh x nw, set
    at (top, left) of the padded frame, cropped at (i, j).  renorm: the reference resized (the
    density map is renormalised to its sum)."""
    h, w = img.shape[:2]
    ch, cw = crop_size
    # the part of the crop inside the resized frame: crop rows [r0, r0 + oh) = resized rows [y0, y0 + oh)
    r0, c0 = max(0, top - i), max(0, left - j)
    y0, x0 = i + r0 - top, j + c0 - left
    oh, ow = min(ch, top - i + nh) - r0, min(cw, left - j + nw) - c0
    fields = []
    # the density map's window and weights stay in double here; collate rounds them to f32 once
    for arr, kind, wconv in ((img, "bicubic", fixed_point), (dmap, "triangle", np.asarray)):
        hx = axis_taps(w, nw, x0, x0 + ow, kind)
        vy = axis_taps(h, nh, y0, y0 + oh, kind)
        fields += [_t(arr[vy.lo:vy.hi, hx.lo:hx.hi], None), _t(hx.bounds, np.int32), _t(wconv(hx.weights), None),
                   _t(vy.bounds, np.int32), _t(wconv(vy.weights), None)]
    scale = 1.0
    if renorm:
        d = np.asarray(dmap, dtype=np.float64)
        new_sum = float(tap_sums(h, nh, "triangle") @ d @ tap_sums(w, nw, "triangle"))
        scale = float(d.sum()) / new_sum if new_sum != 0.0 else 0.0
    geom = np.array([r0, c0, oh, ow, grey, flip, ch, cw, downsample], dtype=np.int32)
    return DenSample(*fields, _t(geom, np.int32), scale, points)


def collate_rescaled(batch) -> RawDenBatch:
    """DenSamples -> RawDenBatch: windows and tables packed end to end, one descriptor per sample."""
    D = {k: n for n, k in enumerate(RESIZE_DESC)}

    def pack(win, hb, hw, vb, vw, px, dtype, wdtype):
        desc = np.zeros((len(batch), len(RESIZE_DESC)), dtype=np.int32)
        src, bounds, weights = [], [], []
        n_src = n_b = n_w = 0
        for n, s in enumerate(batch):
            wi, a, b, c, d_ = (getattr(s, f) for f in (win, hb, hw, vb, vw))
            g = s.geom.tolist()
            r = desc[n]
            r[D["src"]], r[D["sh"]], r[D["sw"]] = n_src, wi.shape[0], wi.shape[1]
            r[D["r0"]], r[D["c0"]], r[D["oh"]], r[D["ow"]], r[D["grey"]], r[D["flip"]] = g[:6]
            r[D["hb"]], r[D["hw"]], r[D["kh"]] = n_b, n_w, b.shape[1]
            r[D["vb"]], r[D["vw"]], r[D["kv"]] = n_b + a.shape[0], n_w + b.numel(), d_.shape[1]
            src.append(wi.reshape(-1, px) if px > 1 else wi.reshape(-1))
            bounds += [a, c]
            weights += [b.reshape(-1), d_.reshape(-1)]
            n_src += wi.shape[0] * wi.shape[1]
            n_b += a.shape[0] + c.shape[0]
            n_w += b.numel() + d_.numel()
        return (torch.cat(src).to(dtype), torch.from_numpy(desc), torch.cat(bounds), torch.cat(weights).to(wdtype))

    img = pack("img_win", "img_hb", "img_hw", "img_vb", "img_vw", 3, torch.uint8, torch.int32)
    dmap = pack("map_win", "map_hb", "map_hw", "map_vb", "map_vw", 1, torch.float32, torch.float32)
    ch, cw, down = batch[0].geom[6:].tolist()
    return RawDenBatch(*img, *dmap, torch.tensor([s.scale for s in batch], dtype=torch.float32),
                       tuple(s.points for s in batch), (ch, cw), down)


class DensityMapDataset(DenClsDataset):
    """reference datasets/den_dataset.py:15-128 (constructor arguments as the reference)."""
    dmap_suffix = "_dmap2"

    def __init__(self, root, crop_size, downsample, method, is_grey, unit_size, pre_resize=1, roi_map_path=None,
                 gt_dir=None, gen_root=None):
        super().__init__(root, crop_size, downsample, method, is_grey=is_grey, unit_size=unit_size,
                         pre_resize=pre_resize, roi_map_path=roi_map_path, gt_dir=gt_dir, gen_root=gen_root)
        _check_crop(self)

    def _train_transform(self, img, gt, dmap):
        return rescale_train_transform(self, img, gt, dmap)

    collate = staticmethod(collate_rescaled)


def _check_crop(ds):
    ch, cw = ds.crop_size
    if ch % ds.downsample or cw % ds.downsample:
        raise ValueError(f"crop {ds.crop_size} is not a multiple of downsample {ds.downsample}")


__all__ = ["DensityMapDataset", "DenSample", "AxisTaps", "tap_table", "tap_sums", "axis_taps", "fixed_point",
           "rescale_train_transform", "make_sample", "collate_rescaled", "PRECISION_BITS"]
