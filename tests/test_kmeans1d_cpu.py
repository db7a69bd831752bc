"""CPU-only checks of the 1-D k-means surface (ISW relax_denom = 0): the C-ABI symbols and their
argument validation (invalid calls return before any launch), the workspace query, the counter's
constructor, and the brute-force yardstick of the GPU tests itself (tests/kmeans1d_ref.py)."""
import ctypes

import numpy as np

import kmeans1d_ref as R

N_MAX = 1 << 20


def _lib():
    from dgvcc_amd import _capi
    return _capi.lib()


def test_symbols_exported():
    from dgvcc_amd import _capi
    syms = _capi.exported_symbols()
    for name in ("dg_kmeans1d_workspace", "dg_kmeans1d", "dg_iw_cluster_mask"):
        assert name in syms and hasattr(_capi.lib(), name)
    assert _capi.lib().dg_version() == 8  # additive: the ABI version stays


def test_invalid_arguments_rejected_without_gpu():
    L = _lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; nothing may be launched or read
    p = ctypes.addressof(buf)
    # dg_kmeans1d(sorted, n, k, bounds, centroids, cost, workspace, stream)
    assert L.dg_kmeans1d(None, 8, 3, p, None, None, p, None) == -1
    assert L.dg_kmeans1d(p, 8, 3, None, None, None, p, None) == -1
    assert L.dg_kmeans1d(p, 8, 3, p, None, None, None, None) == -1
    assert L.dg_kmeans1d(p, 2, 3, p, p, p, p, None) == -1            # n < k
    assert L.dg_kmeans1d(p, 8, 0, p, p, p, p, None) == -1            # k = 0
    assert L.dg_kmeans1d(p, 100, 65, p, p, p, p, None) == -2         # k > 64
    assert L.dg_kmeans1d(p, N_MAX + 1, 3, p, p, p, p, None) == -2    # n > 2^20
    # dg_iw_cluster_mask(v, sorted, bounds, n, prev_mask, mask, num_sensitive, workspace, stream)
    for hole in range(6):
        args = [p, p, p, 8, None, p, p, p, None]
        args[[0, 1, 2, 5, 6, 7][hole]] = None
        assert L.dg_iw_cluster_mask(*args) == -1
    assert L.dg_iw_cluster_mask(p, p, p, 0, None, p, p, p, None) == -1
    assert L.dg_iw_cluster_mask(p, p, p, N_MAX + 1, None, p, p, p, None) == -2
    assert L.dg_kmeans1d_workspace(2, 3) == -1
    assert L.dg_kmeans1d_workspace(8, 0) == -1
    assert L.dg_kmeans1d_workspace(100, 65) == -2
    assert L.dg_kmeans1d_workspace(N_MAX + 1, 3) == -2


def test_workspace_monotone_and_sized():
    L = _lib()
    for k in (1, 2, 3, 64):
        sizes = [L.dg_kmeans1d_workspace(n, k) for n in (64, 65, 66, 1000, 1001, 4096, 1 << 18, N_MAX)]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes)  # never shrinks (256-byte granules)
        assert sizes[0] < sizes[3] < sizes[5] < sizes[6] < sizes[7]  # and grows between distant n
    for n in (64, 4133, 1 << 18):
        sizes = [L.dg_kmeans1d_workspace(n, k) for k in (1, 2, 3, 5, 50, 64)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # prefix sums, two D rows (float64 [n+1] each) and the k x (n+1) int32 argmin table
    n, k = 1 << 18, 64
    assert L.dg_kmeans1d_workspace(n, k) >= 4 * 8 * (n + 1) + 4 * k * (n + 1)
    assert L.dg_kmeans1d_workspace(n, k) < 80e6


def test_isw_counter_constructs_with_relax_denom_0():
    from dgvcc_amd.models.trunks import CovMatrix_ISW, ISWCounter_ResNet
    model = ISWCounter_ResNet(relax_denom=0, pretrained=False)
    assert [c.dim for c in model.cov_matrix_layer] == [64, 256, 512]
    for c in model.cov_matrix_layer:
        assert isinstance(c, CovMatrix_ISW) and c.margin == 0 and c.clusters == 3
    assert ISWCounter_ResNet(relax_denom=0, clusters=5, pretrained=False).cov_matrix_layer[0].clusters == 5
    # the margin path's constructor arithmetic is untouched
    assert CovMatrix_ISW(64, relax_denom=2.0).margin == float((64 * 63 // 2) // 2.0)


def test_kmeans1d_module_imports_without_gpu():
    from dgvcc_amd import kmeans1d
    assert kmeans1d.Clustered._fields == ("clusters", "centroids")
    assert callable(kmeans1d.cluster)


def test_brute_force_dp_hand_case():
    """[0, 0, 0, 1, 1.1, 5], k = 3: {0,0,0} {1,1.1} {5}; cost = 2 * 0.05^2."""
    x = np.array([0, 0, 0, 1, 1.1, 5], dtype=np.float32)
    dp = R.BruteDP(x, 3)
    assert dp.bounds(3) == [0, 3, 5, 6]
    assert abs(dp.cost(3) - 2 * 0.05 ** 2) < 1e-8  # 1.1 is float32-rounded
    assert np.allclose(dp.centroids(3), [0.0, 1.05, 5.0], atol=1e-7)
    assert dp.labels(3).tolist() == [0, 0, 0, 1, 1, 2]
    # k = 2: {0,0,0,1,1.1} {5} (cost 1.33) beats {0,0,0} {1,1.1,5} (cost 10.4)
    assert dp.bounds(2) == [0, 5, 6]
    assert dp.bounds(1) == [0, 6]
    assert abs(dp.cost(1) - ((x.astype(np.float64) - x.astype(np.float64).mean()) ** 2).sum()) < 1e-12


def test_brute_force_dp_is_the_minimum_over_all_partitions():
    """n = 9, k = 4: the DP's cost equals the least cost over every one of the C(8, 3) partitions."""
    from itertools import combinations
    x = np.sort(np.random.default_rng(5).lognormal(-6, 1, 9).astype(np.float32))
    dp = R.BruteDP(x, 4)
    best = min((R.exact_cost(x, [0, *c, 9]), [0, *c, 9]) for c in combinations(range(1, 9), 3))
    assert dp.bounds(4) == best[1]
    assert abs(dp.cost(4) - best[0]) <= 1e-12 * best[0]
    # the windowed and single-boundary searches the full-size GPU checks use, against the DP
    for k in (3, 4):
        wb, wc = R.windowed(x, [0, *range(2, k + 1), 9], 64)  # the window covers every boundary
        assert wb == dp.bounds(k) and abs(wc - dp.cost(k)) <= 1e-12 * wc
        assert [R.best_single_boundary(x, wb, d) for d in range(1, k)] == wb[1:-1]
