"""Device-side training augmentation of the reference's DenClsDataset
(datasets/den_cls_dataset.py:29-35, 77-158).

The reference applies grey-scale, horizontal flip, ToTensor/Normalize (view 1) and
`more_transform` = RandomApply(ColorJitter(0.5, 0.2, 0.2, 0.1), p=0.8),
RandomApply(GaussianBlur(3, sigma=1), p=0.5), RandomAdjustSharpness(5, p=0.5),
ToTensor/Normalize (view 2) to PIL images in host worker processes.  Here:

* the random decisions are drawn on the host with the same generators and in the
  same order as the reference (Python `random` for grey/crop/flip, torch's global RNG
  for the torchvision transforms: `draw_more_transform`), packed into a per-sample
  parameter record (`AUG_PARAMS`);
* the pixel work runs on the GPU (`dg_augment_den_cls`, augment.hip) on uint8 crops
  already in HBM, keeping PIL's integer semantics, and the block map (`dg_block_map`).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import kernels as K
from .._capi import call, ptr, query, stream

AUG_PARAMS = ("grey", "flip", "jitter", "order0", "order1", "order2", "order3", "brightness", "contrast",
              "saturation", "hue_shift", "blur", "k0", "k1", "sharp", "sharp_factor")
P = {k: i for i, k in enumerate(AUG_PARAMS)}

# torchvision ColorJitter(brightness=0.5, contrast=0.2, saturation=0.2, hue=0.1) ranges
JITTER_RANGES = ((0.5, 1.5), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))
BLUR_SIGMA = (1.0, 1.0)   # GaussianBlur(kernel_size=3, sigma=1)
SHARPNESS = 5.0


def hue_shift(hue_factor: float) -> int:
    """torchvision F_pil.adjust_hue: np.array(hue_factor * 255).astype(np.uint8)."""
    return int(np.array(hue_factor * 255).astype(np.uint8))


def gaussian_weights(sigma: float) -> tuple[float, float]:
    """torchvision _get_gaussian_kernel1d(3, sigma) in float32: (edge, centre)."""
    x = torch.linspace(-1.0, 1.0, steps=3, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k = pdf / pdf.sum()
    return float(k[0]), float(k[1])


def draw_more_transform(rec: np.ndarray) -> None:
    """Consume torch's RNG exactly as `more_transform(img)` does and record the decisions:
    RandomApply (`p < torch.rand(1)` skips), ColorJitter.get_params (randperm(4), then one
    uniform_ per factor), GaussianBlur.get_params (uniform_), RandomAdjustSharpness (rand < p)."""
    if not (0.8 < torch.rand(1)):
        fn_idx = torch.randperm(4)
        b, c, s, h = (float(torch.empty(1).uniform_(lo, hi)) for lo, hi in JITTER_RANGES)
        rec[P["jitter"]] = 1.0
        rec[P["order0"]:P["order0"] + 4] = fn_idx.numpy().astype(np.float32)
        rec[P["brightness"]], rec[P["contrast"]], rec[P["saturation"]] = b, c, s
        rec[P["hue_shift"]] = hue_shift(h)
    if not (0.5 < torch.rand(1)):
        sigma = torch.empty(1).uniform_(BLUR_SIGMA[0], BLUR_SIGMA[1]).item()
        rec[P["blur"]] = 1.0
        rec[P["k0"]], rec[P["k1"]] = gaussian_weights(sigma)
    if torch.rand(1).item() < 0.5:
        rec[P["sharp"]] = 1.0
        rec[P["sharp_factor"]] = SHARPNESS


def new_record(grey: bool = False, flip: bool = False) -> np.ndarray:
    rec = np.zeros(len(AUG_PARAMS), dtype=np.float32)
    rec[P["grey"]] = float(grey)
    rec[P["flip"]] = float(flip)
    return rec


@dataclass
class RawDenClsBatch:
    """A collated training batch before its pixel augmentation: uint8 crops [B,H,W,3],
    parameter records [B,16], point sets, density maps [B,1,h,w] (already cropped,
    downsampled and flipped on the host, as in the reference)."""
    imgs: torch.Tensor
    params: torch.Tensor
    points: tuple
    dmaps: torch.Tensor | None = None
    # DenClsDataset(bl_targets=True): per image, every annotation in crop coordinates before the
    # in-crop mask and the flip (f32 [n, 2]), and st_size [B] (datasets/bay_dataset.py:69-71)
    all_points: tuple | None = None
    st_sizes: torch.Tensor | None = None


# per-sample descriptor of dg_resize_crop_u8 / dg_resize_crop_f32 (resize.hip), int32 x 16
RESIZE_DESC = ("src", "sh", "sw", "oh", "ow", "r0", "c0", "hb", "hw", "kh", "vb", "vw", "kv", "grey", "flip", "tmp")


@dataclass
class RawDenBatch:
    """A collated DensityMapDataset / JHUDomainDataset training batch before its pixel work (CPU
    tensors only): per sample the source windows of the image and of the density map that the
    crop's resampling taps touch, packed end to end, the tap tables (built on the host in float64,
    datasets/den_dataset.py) and a descriptor [B,16] (RESIZE_DESC); the renormalisation scalars
    [B]; the point sets; the crop size and the density map's downsample."""
    img_src: torch.Tensor       # uint8 [pixels, 3]
    img_desc: torch.Tensor      # int32 [B, 16]
    img_bounds: torch.Tensor    # int32 [n, 2]: (start in the window, count) per output column / row
    img_weights: torch.Tensor   # int32, 22 fractional bits
    map_src: torch.Tensor       # f32 [elements]
    map_desc: torch.Tensor
    map_bounds: torch.Tensor
    map_weights: torch.Tensor   # f32
    scales: torch.Tensor        # f32 [B]
    points: tuple
    crop_size: tuple
    downsample: int


def _resize_args(src, desc, bounds, weights, dev):
    if desc.device.type != "cpu" or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != len(RESIZE_DESC):
        raise ValueError("desc must be a CPU int32 [B, 16] tensor")
    return (src.to(dev, non_blocking=True).contiguous(), desc.contiguous(),
            bounds.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous(),
            weights.to(dev, non_blocking=True).contiguous())


def _resize_out(out, shape, dev):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {shape} tensor on {dev}")
    return out


def resize_crop_u8(src, desc, bounds, weights, crop_size, device, out=None):
    """[B,3,ch,cw] f32 normalised crops of the PIL-bicubic-resized frames (dg_resize_crop_u8)."""
    dev = torch.device(device)
    if src.dtype != torch.uint8 or weights.dtype != torch.int32:
        raise ValueError("src must be uint8 and weights int32")
    src, desc, bounds, weights = _resize_args(src, desc, bounds, weights, dev)
    B, (ch, cw) = desc.shape[0], crop_size
    out = _resize_out(out, (B, 3, ch, cw), dev)
    ws = query("dg_resize_crop_workspace", ptr(desc), B, 3)
    work = torch.empty(ws, dtype=torch.uint8, device=dev)
    call("dg_resize_crop_u8", ptr(src), src.numel() // 3, ptr(desc), B, ptr(bounds), bounds.numel() // 2,
         ptr(weights), weights.numel(), ch, cw, ptr(out), ptr(work), ws, stream())
    return out


def resize_crop_f32(src, desc, bounds, weights, scales, crop_size, downsample, device, out=None):
    """[B,1,ch/ds,cw/ds] f32 block sums of the crops of the resized, renormalised density maps
    (dg_resize_crop_f32)."""
    dev = torch.device(device)
    if src.dtype != torch.float32 or weights.dtype != torch.float32:
        raise ValueError("src and weights must be float32")
    src, desc, bounds, weights = _resize_args(src, desc, bounds, weights, dev)
    B, (ch, cw), ds = desc.shape[0], crop_size, int(downsample)
    if ds <= 0 or ch % ds or cw % ds:
        raise ValueError(f"crop {crop_size} is not a multiple of downsample {downsample}")
    scales = scales.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
    if scales.numel() != B:
        raise ValueError("one scale per sample")
    out = _resize_out(out, (B, 1, ch // ds, cw // ds), dev)
    ws = query("dg_resize_crop_workspace", ptr(desc), B, 4)
    work = torch.empty(ws, dtype=torch.uint8, device=dev)
    call("dg_resize_crop_f32", ptr(src), src.numel(), ptr(desc), B, ptr(bounds), bounds.numel() // 2, ptr(weights),
         weights.numel(), ptr(scales), ch, cw, ds, ptr(out), ptr(work), ws, stream())
    return out


def resize_crop(raw: RawDenBatch, device):
    """(imgs [B,3,ch,cw], dmaps [B,1,ch/ds,cw/ds]) of a RawDenBatch, all pixel work on `device`."""
    imgs = resize_crop_u8(raw.img_src, raw.img_desc, raw.img_bounds, raw.img_weights, raw.crop_size, device)
    dmaps = resize_crop_f32(raw.map_src, raw.map_desc, raw.map_bounds, raw.map_weights, raw.scales, raw.crop_size,
                            raw.downsample, device)
    return imgs, dmaps


class GtDatas(tuple):
    """The reference's `(points, dmaps, bmaps)` (indexing, [-1] and 3-way unpacking as a plain
    tuple) that also carries the Bayesian-loss batch: `bl = (points_kept, targets, st_sizes)`."""
    bl = None

    def __new__(cls, items, bl=None):
        self = super().__new__(cls, items)
        self.bl = bl
        return self


def bl_batch(all_points, st_sizes, params: torch.Tensor, h: int, w: int, device):
    """(points_kept, targets, st_sizes) of a batch for losses.bl.BL: the per-point targets of
    the reference's BayesianDataset computed on `device` (dg_bl_targets) from the unfiltered
    annotations; x is mirrored where the record's flip flag is set.  params: the [B,16] records
    on `device`.  One device-to-host copy (the B+1 offsets of the kept points) splits the lists."""
    counts = [int(p.shape[0]) for p in all_points]
    B = len(counts)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64).to(device, non_blocking=True)
    if sum(counts):
        pts = torch.cat([p.reshape(-1, 2) for p in all_points]).to(device=device, dtype=torch.float32,
                                                                  non_blocking=True).contiguous()
    else:
        pts = torch.empty((0, 2), dtype=torch.float32, device=device)
    kept, targets, koffs = K.bl_targets(pts, offs, h, w, params[:, P["flip"]:P["flip"] + 1])
    ko = koffs.cpu().tolist()
    points_kept = tuple(kept[ko[b]:ko[b + 1]] for b in range(B))
    targets = tuple(targets[ko[b]:ko[b + 1]] for b in range(B))
    return points_kept, targets, torch.as_tensor(st_sizes, dtype=torch.float32).to(device, non_blocking=True)


def augment_den_cls(imgs: torch.Tensor, params: torch.Tensor):
    """(img1, img2) NCHW f32 from uint8 crops [B,H,W,3] resident on the GPU."""
    if imgs.dtype != torch.uint8 or imgs.dim() != 4 or imgs.shape[3] != 3:
        raise ValueError("imgs must be uint8 [B, H, W, 3]")
    B, H, W, _ = imgs.shape
    dev = imgs.device
    imgs = imgs.contiguous()
    params = params.to(device=dev, dtype=torch.float32).contiguous()
    img1 = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    img2 = torch.empty_like(img1)
    ws = query("dg_augment_workspace", B, H, W)
    work = torch.empty(ws, dtype=torch.uint8, device=dev)
    call("dg_augment_den_cls", ptr(imgs), B, H, W, ptr(params), ptr(img1), ptr(img2), ptr(work), ws, stream())
    return img1, img2


def block_map(dmaps: torch.Tensor) -> torch.Tensor:
    """bmap = (16x16 block sums of dmap > 0) (datasets/den_cls_dataset.py:62-63)."""
    B, _, h, w = dmaps.shape
    d = dmaps.float().contiguous()
    out = torch.empty((B, 1, h // 16, w // 16), dtype=torch.float32, device=d.device)
    call("dg_block_map", ptr(d), B, h, w, ptr(out), stream())
    return out


class DeviceAugment:
    """RawDenClsBatch -> the reference's collated batch (img1, img2, (points, dmaps, bmaps))
    with all pixel work on `device`; RawDenBatch -> (imgs, imgs, (points, dmaps, <empty tensor>))."""

    def __init__(self, device):
        self.device = torch.device(device)

    def __call__(self, raw):
        if isinstance(raw, RawDenBatch):
            # one view and no block map (den_dataset.py:16-21 collates `images, (points, dmaps)`):
            # the view stands in both image slots, an empty tensor in the block map's
            imgs, dmaps = resize_crop(raw, self.device)
            points = tuple(p.to(self.device) for p in raw.points)
            return imgs, imgs, (points, dmaps, torch.empty(0, device=self.device))
        imgs = raw.imgs.to(self.device, non_blocking=True)
        params = raw.params.to(device=self.device, dtype=torch.float32).contiguous()
        img1, img2 = augment_den_cls(imgs, params)
        dmaps = raw.dmaps.to(self.device, non_blocking=True)
        bmaps = block_map(dmaps)
        gt_datas = (tuple(p.to(self.device) for p in raw.points), dmaps, bmaps)
        if raw.all_points is None:
            return img1, img2, gt_datas
        if raw.st_sizes is None:
            raise ValueError("a batch with all_points needs st_sizes")
        bl = bl_batch(raw.all_points, raw.st_sizes, params, imgs.shape[1], imgs.shape[2], self.device)
        return img1, img2, GtDatas(gt_datas, bl)


__all__ = ["AUG_PARAMS", "RESIZE_DESC", "RawDenClsBatch", "RawDenBatch", "DeviceAugment", "resize_crop", "resize_crop_u8",
           "resize_crop_f32", "GtDatas", "bl_batch", "augment_den_cls", "block_map", "draw_more_transform",
           "new_record", "hue_shift", "gaussian_weights"]
_ = K  # the kernels module loads the library (fails loudly when it is missing)
