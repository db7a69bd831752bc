"""Numpy float64 restatement of the Bayesian-loss point targets (dg_bl_targets, include/dgvcc.h),
written from their specification; tests/golden/bl_targets.npz pins it to the reference.

Per image with n points p_i in crop coordinates (unfiltered) and a crop of h x w:
  d_i   : n == 1 -> 4;  n >= 4 -> mean of the 2nd..4th smallest entries of row i of the distance
          matrix (the point's own 0 and the zeros of duplicates count);  n == 2, 3 -> mean of
          dist(i, k) for k = 1..n-1 by index;
  s_i   = clip(d_i, 4, 128);  ratio_i = clip(area((p_i +- s_i/2) ^ [0,w] x [0,h]) / s_i^2, 0, 1);
  kept  : ratio_i >= 0.3, in order; x -> w - x where the image's flip flag is set.
"""
from __future__ import annotations

import numpy as np

KEEP_RATIO = 0.3


def point_dists(pts: np.ndarray) -> np.ndarray:
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    n = len(pts)
    if n == 0:
        return np.zeros((0,))
    if n == 1:
        return np.array([4.0])
    diff = pts[:, None, :] - pts[None, :, :]
    dist = np.sqrt((diff * diff).sum(-1))
    if n < 4:
        return dist[:, 1:].mean(axis=1)
    return np.sort(dist, axis=1)[:, 1:4].mean(axis=1)


def point_ratios(pts: np.ndarray, d: np.ndarray, h: float, w: float) -> np.ndarray:
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    s = np.clip(d, 4.0, 128.0)
    ix = np.maximum(np.minimum(w, pts[:, 0] + s / 2) - np.maximum(0.0, pts[:, 0] - s / 2), 0.0)
    iy = np.maximum(np.minimum(h, pts[:, 1] + s / 2) - np.maximum(0.0, pts[:, 1] - s / 2), 0.0)
    return np.clip(ix * iy / (s * s), 0.0, 1.0)


def bl_targets(points_list, h, w, flips):
    """-> (kept points [m, 2], targets [m], offsets [B+1], d [total], ratio [total], keep [total])."""
    kept, targs, offs, ds, rs, keeps = [], [], [0], [], [], []
    for pts, flip in zip(points_list, flips):
        pts = np.asarray(pts, np.float64).reshape(-1, 2)
        d = point_dists(pts)
        r = point_ratios(pts, d, h, w)
        k = r >= KEEP_RATIO
        p = pts[k].copy()
        if flip:
            p[:, 0] = w - p[:, 0]
        kept.append(p)
        targs.append(r[k])
        offs.append(offs[-1] + int(k.sum()))
        ds.append(d)
        rs.append(r)
        keeps.append(k)
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape)  # noqa: E731
    return (cat(kept, (0, 2)), cat(targs, (0,)), np.asarray(offs, np.int64), cat(ds, (0,)), cat(rs, (0,)),
            cat(keeps, (0,)).astype(bool))
