"""Generate the MCNN fixtures by RUNNING THE REFERENCE (models/baselines/MCNN.py) on seeded
inputs.  Run where the reference is checked out (it does not exist on the GPU box):

    python tests/golden/make_golden_mcnn.py

Writes tests/golden/mcnn.npz and tests/golden/mcnn_keys.json.  Weights and inputs are
seeded (oracle.dg_oracle.seeded_state_dict, CASES / case_input below), so neither is stored.
Per case: the float64 output, the error of the reference's own fp32 run against it, and the
parameter gradients of sum(out * g) for a seeded g, summarised as in models2_*.npz (small
tensors whole, large ones as 16 sampled entries + sums).
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

# name -> (B, H, W): at 32x32 the quarter-resolution 7x7 and 5x5 layers run on 8x8 maps, smaller than
# their own footprint; 36x44 gives a 9x11 output, odd in both axes
CASES = {"r32x32": (2, 32, 32), "r36x44": (2, 36, 44)}
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
    model = mod.MCNN(load_weights=True)
    model.load_state_dict(O.seeded_state_dict(model.state_dict()))
    model.to(dtype).train()
    o = model(case_input(name).to(dtype))
    r = torch.randn(o.shape, generator=torch.Generator().manual_seed(99), dtype=torch.float64).to(dtype)
    (o * r).sum().backward()
    return o.detach(), {k: p.grad for k, p in model.named_parameters()}


def main():
    from oracle.ref_import import import_ref
    mod = import_ref("models.baselines.MCNN")
    keys = [[k, list(v.shape)] for k, v in mod.MCNN(load_weights=True).state_dict().items()]
    json.dump(keys, open(os.path.join(HERE, "mcnn_keys.json"), "w"))
    out = {}
    for name in CASES:
        o64, g64 = run(mod, name, torch.float64)
        o32, g32 = run(mod, name, torch.float32)
        out[f"{name}__out"] = o64.numpy()
        err = (o32.double() - o64).abs().max().item() / max(o64.abs().max().item(), 1e-30)
        out[f"{name}__out__ref32_err"] = np.array([err])
        num = sum(float((g32[k].double() - g64[k]).norm() ** 2) for k in g64)
        den = sum(float(g64[k].norm() ** 2) for k in g64)
        out[f"{name}__grad_ref32_err"] = np.array([(num / max(den, 1e-300)) ** 0.5])
        out[f"{name}__gradnorm"] = np.array([den ** 0.5])
        summarize(f"{name}__grad__", g64, out)
        print(name, tuple(o64.shape), float(o64.abs().max()), float(o64.std()),
              {k: float(v[0]) for k, v in out.items() if k.startswith(name) and "ref32" in k})
    np.savez_compressed(os.path.join(HERE, "mcnn.npz"), **out)


if __name__ == "__main__":
    main()
