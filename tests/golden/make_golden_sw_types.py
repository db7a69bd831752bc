"""Generate tests/golden/sw_types.npz by RUNNING THE REFERENCE SwitchWhiten2d
(models/SW/ops/switchwhiten.py) in float64 on the seeded cases of tests/sw_ref.py, for every
variant outside the SW counter's own configuration: sw_type {3, 5} x tie_weight x affine, and
sw_type 2 tied and / or without affine.  Runs only where the reference exists:

    python tests/golden/make_golden_sw_types.py

Inputs and parameters are not stored (tests/sw_ref.fixture_case regenerates them); per variant
`<name>__y`, `__gx`, `__grad__<param>`, `__post__running_mean/cov`, `__y_eval` (eval mode on the
initial running statistics) and `__keys` (the state_dict keys).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import sw_ref as R  # noqa: E402


def main():
    MG._patch_offline()
    swm = MG.import_ref("models.SW.ops.switchwhiten")
    out = {}
    for sw_type, tie, affine in R.VARIANTS:
        name = R.variant_name(sw_type, tie, affine)
        x, gy, params = R.fixture_case(sw_type, tie, affine)
        m = swm.SwitchWhiten2d(R.FIXTURE_SHAPE[1], num_pergroup=16, sw_type=sw_type, T=5, tie_weight=tie,
                               eps=1e-5, momentum=0.9, affine=affine).double()
        sd = m.state_dict()
        assert list(sd) == list(params), (list(sd), list(params))
        m.load_state_dict({k: v.double() for k, v in params.items()})
        out[name + "__keys"] = np.array(list(sd))
        xr = x.double().requires_grad_(True)
        m.eval()
        with torch.no_grad():
            out[name + "__y_eval"] = m(xr.detach()).numpy()
        m.train()
        y = m(xr)
        y.backward(gy.double())
        out[name + "__y"] = y.detach().numpy()
        out[name + "__gx"] = xr.grad.numpy()
        for k, p in m.named_parameters():
            out[name + "__grad__" + k] = p.grad.numpy()
        for k in ("running_mean", "running_cov"):
            out[name + "__post__" + k] = getattr(m, k).numpy().copy()
    np.savez_compressed(os.path.join(HERE, "sw_types.npz"), **out)
    print(len(R.VARIANTS), "variants,", os.path.getsize(os.path.join(HERE, "sw_types.npz")), "bytes")


if __name__ == "__main__":
    main()
