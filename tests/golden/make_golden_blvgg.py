"""Generate the BL VGG19 counter (BL_VGG) fixtures by RUNNING THE REFERENCE (models/baselines/BL.py)
on seeded inputs.  Run where the reference is checked out (it does not exist on the GPU box):

    python tests/golden/make_golden_blvgg.py

Writes tests/golden/blvgg.npz and tests/golden/blvgg_keys.json.  Weights and inputs are
seeded (oracle.dg_oracle.seeded_state_dict, CASES / case_input below), so neither is stored.
Per case: the float64 output, the error of the reference's own fp32 run against it, and the
parameter gradients of sum(out * g) for a seeded g, summarised as in models2_*.npz (small
tensors whole, large ones as 16 sampled entries + sums).  The output is |z|: the smallest |z| and
the fraction of negative z of the float64 run are stored too (`__zstat`), which is what makes the
abs checkable: with these weights z is negative at >= 99% of the pixels, and no |z| is within fp32
error of 0, so no sign flips.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import dg_oracle as O  # noqa: E402

# name -> (B, H, W): 16x48 has 1x3 features, the one-row align-corners case (ratio 0 along H), and a
# 2x6 output; 48x80 has 3x5 features and a 6x10 output, odd in both axes before the upsampling
CASES = {"r16x48": (2, 16, 48), "r48x80": (2, 48, 80)}
N_SAMPLE = 16


def case_input(name):
    """The case's image batch: the top-left H x W corner of the seeded synthetic frames of the next
    multiple of 16 (O.synthetic_batch block-sums 16 x 16 tiles)."""
    B, H, W = CASES[name]
    up = lambda v: -(-v // 16) * 16  # noqa: E731
    img = O.synthetic_batch(B, up(H), up(W), seed=2112, with_dmap=False)[0]
    return img[..., :H, :W].contiguous()


def summarize(prefix, d, out):
    g = torch.Generator().manual_seed(7)
    for k, v in d.items():
        v = v.detach().double().reshape(-1)
        key = prefix + k.replace(".", "__")
        if v.numel() <= 1024:
            out[key] = v.float().numpy()
        else:
            idx = torch.randint(0, v.numel(), (N_SAMPLE,), generator=g)
            out[key + "@idx"] = idx.numpy()
            out[key + "@val"] = v[idx].float().numpy()
            out[key + "@sum"] = np.array([v.sum().item(), v.abs().sum().item()])


def run(mod, name, dtype):
    model = mod.BL_VGG(pretrained=False)
    model.load_state_dict(O.seeded_state_dict(model.state_dict()))
    model.to(dtype).train()
    x = case_input(name).to(dtype)
    o = model(x)
    with torch.no_grad():  # the signed map under the abs
        up = torch.nn.functional.interpolate(model.features(x), scale_factor=2, mode="bilinear", align_corners=True)
        z = model.reg_layer(up)
    assert torch.equal(z.abs(), o.detach())
    r = torch.randn(o.shape, generator=torch.Generator().manual_seed(99), dtype=torch.float64).to(dtype)
    (o * r).sum().backward()
    return o.detach(), {k: p.grad for k, p in model.named_parameters()}, z


def main():
    from oracle.ref_import import import_ref
    mod = import_ref("models.baselines.BL")
    keys = [[k, list(v.shape)] for k, v in mod.BL_VGG(pretrained=False).state_dict().items()]
    json.dump(keys, open(os.path.join(HERE, "blvgg_keys.json"), "w"))
    out = {}
    for name in CASES:
        o64, g64, z64 = run(mod, name, torch.float64)
        o32, g32, _ = run(mod, name, torch.float32)
        out[f"{name}__zstat"] = np.array([z64.abs().min().item(), (z64 < 0).double().mean().item()])
        out[f"{name}__out"] = o64.numpy()
        err = (o32.double() - o64).abs().max().item() / max(o64.abs().max().item(), 1e-30)
        out[f"{name}__out__ref32_err"] = np.array([err])
        num = sum(float((g32[k].double() - g64[k]).norm() ** 2) for k in g64)
        den = sum(float(g64[k].norm() ** 2) for k in g64)
        out[f"{name}__grad_ref32_err"] = np.array([(num / max(den, 1e-300)) ** 0.5])
        out[f"{name}__gradnorm"] = np.array([den ** 0.5])
        summarize(f"{name}__grad__", g64, out)
        print(name, tuple(o64.shape), float(o64.abs().max()), float(o64.std()),
              {k: float(v[0]) for k, v in out.items() if k.startswith(name) and "ref32" in k},
              "zstat", out[f"{name}__zstat"].tolist())
    np.savez_compressed(os.path.join(HERE, "blvgg.npz"), **out)


if __name__ == "__main__":
    main()
