"""Device cost of the random rescale of DensityMapDataset / JHUDomainDataset (dg_resize_crop_u8,
dg_resize_crop_f32) against the host path it replaces, on the same machine.

Batch 16, crop 768x1024, sources 1.0-1.4x the crop, factors spread over [0.75, 1.25].  Prints
device ms per batch for both kernels with the bytes they move (source windows read, intermediate
written and read, output written) and the rate that makes; the host half that remains (tap tables,
window slices, renormalisation scalar: `make_sample`) per sample; and the replaced host work (PIL
`resize` of the frame + `F.interpolate(antialias=True)` of the map + renormalise + crop) per sample
on one core."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image
from dgvcc_amd.datasets.augment import resize_crop_f32, resize_crop_u8
from dgvcc_amd.datasets.den_dataset import collate_rescaled, make_sample

B, CH, CW, DS, ITERS, REPEATS = 16, 768, 1024, 1, 500, 5
dev = torch.device("cuda")
torch.set_num_threads(1)
rng = np.random.default_rng(0)
frames, geoms, samples = [], [], []
t_host = 0.0
for k, f in enumerate(np.linspace(0.75, 1.25, B)):
    m = min(1.4, max(1.0, 1.02 / f))
    h, w = int(CH * m) + k, int(CW * m) + 2 * k
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    dmap = (rng.random((h, w)) ** 8).astype(np.float32)
    nh, nw = int(h * f), int(w * f)
    i, j = (nh - CH) // 2, (nw - CW) // 2
    frames.append((img, dmap))
    geoms.append((nh, nw, i, j))
    t0 = time.perf_counter()
    samples.append(make_sample(img, dmap, nh, nw, 0, 0, i, j, (CH, CW), DS, k % 8 == 0, k % 2 == 1, True,
                               torch.zeros(0, 2)))
    t_host += time.perf_counter() - t0
raw = collate_rescaled(samples)

img_args = [raw.img_src.to(dev), raw.img_desc, raw.img_bounds.to(dev), raw.img_weights.to(dev)]
map_args = [raw.map_src.to(dev), raw.map_desc, raw.map_bounds.to(dev), raw.map_weights.to(dev), raw.scales.to(dev)]


def timed(fn):
    """(median, min, max) ms per call over REPEATS windows of ITERS calls, after a warm-up."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / ITERS)
    return float(np.median(ms)), min(ms), max(ms)


def moved(desc, px, out_elems):
    d = desc.numpy().astype(np.int64)
    return int((d[:, 1] * d[:, 2] * px + 2 * d[:, 1] * d[:, 4] * px).sum() + out_elems * 4)


ms_u8, lo_u8, hi_u8 = timed(lambda: resize_crop_u8(*img_args, (CH, CW), dev))
ms_f32, lo_f32, hi_f32 = timed(lambda: resize_crop_f32(*map_args, (CH, CW), DS, dev))
out_u8 = resize_crop_u8(*img_args, (CH, CW), dev)
out_f32 = resize_crop_f32(*map_args, (CH, CW), DS, dev)
by_u8 = moved(raw.img_desc, 3, B * 3 * CH * CW)
by_f32 = moved(raw.map_desc, 4, B * CH * CW // (DS * DS))
print(f"dg_resize_crop_u8 : {ms_u8:.3f} ms/batch of {B} (min {lo_u8:.3f}, max {hi_u8:.3f}; {REPEATS} x {ITERS} calls, "
      f"each with its descriptor copy and two launches), {by_u8 / 1e6:.1f} MB moved, {by_u8 / ms_u8 / 1e9:.3f} TB/s",
      flush=True)
print(f"dg_resize_crop_f32: {ms_f32:.3f} ms/batch of {B} (min {lo_f32:.3f}, max {hi_f32:.3f}), "
      f"{by_f32 / 1e6:.1f} MB moved, {by_f32 / ms_f32 / 1e9:.3f} TB/s", flush=True)
print(f"host half kept (make_sample): {t_host / B * 1e3:.2f} ms/sample/core", flush=True)

t_pil = t_map = 0.0
n = 4
for (img, dmap), (nh, nw, i, j) in list(zip(frames, geoms))[::B // n]:
    t0 = time.perf_counter()
    a = np.asarray(Image.fromarray(img).resize((nw, nh)))[i:i + CH, j:j + CW]
    t1 = time.perf_counter()
    d = torch.from_numpy(dmap)[None, None]
    r = F.interpolate(d, size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)
    r = (r * d.sum() / r.sum())[..., i:i + CH, j:j + CW].contiguous()
    t2 = time.perf_counter()
    t_pil += t1 - t0
    t_map += t2 - t1
    k = geoms.index((nh, nw, i, j))
    if k % 8 and not k % 2:  # neither grey nor flipped: the device crop is PIL's, bit for bit
        want = torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)
        assert torch.equal(out_u8[k].cpu(), want), f"sample {k} differs from PIL"
        err = (out_f32[k, 0].cpu().double() - r[0, 0].double()).abs().max().item()
        # torch's f32 path forms its weights in f32 at coordinates near 1000 (~1e-4 relative); the device
        # applies float64-built weights (tests/test_resize_gpu.py holds it to the float64 restatement)
        print(f"sample {k}: image equals PIL bit for bit; map max |device - F.interpolate in f32| {err:.2e} "
              f"(map max {r.max().item():.2e})", flush=True)
print(f"host path replaced: PIL resize {t_pil / n * 1e3:.1f} ms + map interpolate {t_map / n * 1e3:.1f} ms "
      f"= {(t_pil + t_map) / n * 1e3:.1f} ms/sample/core; device {(ms_u8 + ms_f32) / B:.3f} ms/sample", flush=True)
