"""Generate tests/golden/bl_targets.npz by RUNNING THE REFERENCE's Bayesian-loss target code
(datasets/bay_dataset.py `BayesianDataset._cal_dists` :38-48 and the box arithmetic of
`_train_transform` :85-98 with utils/misc.py `cal_inner_area`) on seeded float64 points.  Run where
the reference is available:

    python tests/golden/make_golden_bl_targets.py

Points lie on a 1/8-pixel lattice, so every coordinate difference is exact in float32 and the
reference's expanded squared distance is exact in float64.  Every case is a batch (most of one
image): `<case>__points` are the annotations shifted into crop coordinates (source - [j, i]),
unfiltered; `__d` / `__ratio` the reference's distance and clipped area share of every point;
`__kept` / `__targets` / `__offsets` the points with ratio >= 0.3 (x mirrored where `__flips` is
set: the image's own flip, not the reference's unconditional one) and their ratios.  No stored
ratio lies within 1e-3 of 0.3 (a case is reseeded until that holds), so a kept set never hinges
on rounding.  Arrays only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_import import REF, import_ref  # noqa: E402

CROP_I, CROP_J, CROP_H, CROP_W = 16, 32, 64, 64   # crop rows 16..80, columns 32..96
SRC_H, SRC_W = 96, 128
TILE = 256                                        # dg_bl_targets stages this many points per LDS tile
MARGIN = 1e-3


def load_reference():
    """(_cal_dists, cal_inner_area).  An installed `datasets` distribution shadows the reference's
    namespace package of that name, so bay_dataset.py is loaded by file path under a package entry
    that points at the reference's directory."""
    misc = import_ref("utils.misc")
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    spec = importlib.util.spec_from_file_location("datasets.bay_dataset",
                                                  os.path.join(REF, "datasets", "bay_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["datasets.bay_dataset"] = mod
    spec.loader.exec_module(mod)
    return (lambda pts: mod.BayesianDataset._cal_dists(None, pts)), misc.cal_inner_area


def lattice(rng, n, x0, x1, y0, y1):
    """n points on the 1/8-pixel lattice of [x0, x1) x [y0, y1) (source coordinates)."""
    x = rng.integers(int(x0 * 8), int(x1 * 8), n) / 8.0
    y = rng.integers(int(y0 * 8), int(y1 * 8), n) / 8.0
    return np.stack([x, y], 1).astype(np.float64)


def reference_image(cal_dists, cal_inner_area, gt):
    """bay_dataset.py:30 + :85-98 for one image: (d [n], ratio [n], mask [n])."""
    if len(gt) == 0:
        z = np.zeros((0,))
        return z, z, z.astype(bool)
    d = cal_dists(gt)                                   # [n, 1]
    side = np.clip(d, 4.0, 128.0)
    boxes = np.hstack([gt - side / 2.0, gt + side / 2.0])  # (left, up, right, down) in source coordinates
    inside = cal_inner_area(CROP_J, CROP_I, CROP_J + CROP_W, CROP_I + CROP_H, boxes)
    ratio = np.clip(inside / (side * side)[:, 0], 0.0, 1.0)
    return d[:, 0], ratio, ratio >= 0.3


def near_crop(rng, n):
    return lattice(rng, n, CROP_J - 8, CROP_J + CROP_W + 8, CROP_I - 8, CROP_I + CROP_H + 8)


def everywhere(rng, n):
    return lattice(rng, n, 0, SRC_W, 0, SRC_H)


def coincident(rng, n):
    p = near_crop(rng, n)
    p[1] = p[3] = p[0]          # three points on one spot: three zeros in their rows
    return p


def far_clusters(rng, n):
    """Two clusters 1900 px apart on a 2048-wide extent, 3 + 2 points: every point's three nearest
    include one across the gap, so every d exceeds 128."""
    a = lattice(rng, 3, CROP_J + 24, CROP_J + 40, CROP_I + 24, CROP_I + 40)
    b = lattice(rng, 2, 1960, 1976, CROP_I + 24, CROP_I + 40)
    return np.concatenate([a, b])


CASES = [("n0", [(everywhere, 0)], [0]), ("n1", [(near_crop, 1)], [1]), ("n2", [(near_crop, 2)], [0]),
         ("n3", [(near_crop, 3)], [1]), ("n4", [(near_crop, 4)], [0]), ("n5", [(near_crop, 5)], [1]),
         ("n64", [(everywhere, 64)], [0]), ("n65", [(everywhere, 65)], [1]),
         (f"n{TILE + 1}", [(everywhere, TILE + 1)], [0]), ("n1200", [(everywhere, 1200)], [1]),
         ("coincident", [(coincident, 6)], [1]), ("far", [(far_clusters, 5)], [0]),
         ("batch", [(everywhere, 65), (everywhere, 0), (everywhere, 300), (everywhere, 0)], [1, 0, 1, 0])]


def main():
    cal_dists, cal_inner_area = load_reference()
    out = {"cases": np.array([c[0] for c in CASES]), "crop": np.array([CROP_I, CROP_J, CROP_H, CROP_W])}
    shift = np.array([CROP_J, CROP_I], np.float64)
    for ci, (name, images, flips) in enumerate(CASES):
        for attempt in range(1000):
            rng = np.random.default_rng(1000 * ci + attempt)
            gts = [gen(rng, n) for gen, n in images]
            res = [reference_image(cal_dists, cal_inner_area, gt) for gt in gts]
            ratios = np.concatenate([r[1] for r in res])
            if not np.any(np.abs(ratios - 0.3) < MARGIN):
                break
        else:
            raise RuntimeError(f"{name}: no seed keeps every ratio {MARGIN} away from 0.3")
        assert not np.any(np.abs(ratios - 0.3) < MARGIN)
        kept, targets, offs = [], [], [0]
        for gt, (d, ratio, mask), flip in zip(gts, res, flips):
            p = gt[mask] - shift
            if flip:
                p[:, 0] = CROP_W - p[:, 0]
            kept.append(p)
            targets.append(ratio[mask])
            offs.append(offs[-1] + int(mask.sum()))
        out[f"{name}__counts"] = np.array([len(g) for g in gts], np.int64)
        out[f"{name}__points"] = np.concatenate(gts).reshape(-1, 2) - shift
        out[f"{name}__flips"] = np.array(flips, np.int64)
        out[f"{name}__d"] = np.concatenate([r[0] for r in res])
        out[f"{name}__ratio"] = ratios
        out[f"{name}__kept"] = np.concatenate(kept).reshape(-1, 2)
        out[f"{name}__targets"] = np.concatenate(targets)
        out[f"{name}__offsets"] = np.array(offs, np.int64)
        margin = np.abs(ratios - 0.3).min() if len(ratios) else float("nan")
        print(f"{name}: seed {1000 * ci + attempt}, n {[len(g) for g in gts]}, kept {offs[-1]}, "
              f"d [{out[f'{name}__d'].min() if len(ratios) else 0:.3f}, "
              f"{out[f'{name}__d'].max() if len(ratios) else 0:.3f}], margin {margin:.2e}")
    assert (out["n1200__d"] < 4.0).any(), "the 1200-point case must hold distances below the clip"
    assert (out["far__d"] > 128.0).all(), "the far-cluster case must hold distances above the clip"
    np.savez_compressed(os.path.join(HERE, "bl_targets.npz"), **out)


if __name__ == "__main__":
    main()
