"""`kmeans1d.cluster` on the HIP kernels: the call the reference's ISW code makes
(models/ISW/cov_settings.py:58, `clusters, centroids = kmeans1d.cluster(var_flatten, k)`).

    from dgvcc_amd import kmeans1d
    clusters, centroids = kmeans1d.cluster(values, 3)

Optimal 1-D k-means is a defined optimum (the contiguous partition of the sorted values with the
least within-cluster sum of squares), so this matches any exact implementation wherever the optimum
is unique.  The values are sorted with torch.sort, clustered by dg_kmeans1d on the GPU and the
labels scattered back through the sort's permutation.  It returns Python lists, so it waits for
the device; CovMatrix_ISW.set_mask_matrix runs the same kernels without it and without a wait.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import kernels as K

Clustered = namedtuple("Clustered", "clusters centroids")


def cluster(array, k: int) -> Clustered:
    """array: a list, numpy array, or CPU / GPU tensor of n >= k values (clustered as float32).
    clusters: list of n ints in the input's order, cluster 0 the one with the lowest centroid;
    centroids: list of k floats, ascending."""
    x = torch.as_tensor(array)
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise K.DGError("kmeans1d.cluster runs on the GPU (the HIP path has no CPU fallback)")
        x = x.to("cuda")
    x = x.detach().flatten().to(torch.float32)
    srt, order = torch.sort(x)
    bounds, centroids, _ = K.kmeans1d(srt.contiguous(), k)
    # label of sorted position p = number of inner boundaries <= p
    pos = torch.arange(x.numel(), device=x.device, dtype=torch.int32)
    labels_sorted = torch.bucketize(pos, bounds[1:-1].contiguous(), right=True)
    labels = torch.empty_like(labels_sorted)
    labels[order] = labels_sorted
    return Clustered(labels.tolist(), centroids.tolist())
