"""Optimal 1-D k-means on the GPU (dg_kmeans1d / dg_iw_cluster_mask) and the ISW relax_denom = 0
mask built on it, against the exhaustive float64 dynamic programme of tests/kmeans1d_ref.py.

Parity is with the optimum (a defined minimum), not with a kmeans1d release.  Tolerances: the bounds
must be equal; the total cost within 1e-9 relative (float64 prefix differences carry ~n 2^-53 ~ 3e-11
of sum x^2 at the largest n here; x30), plus (n 2^-53)^2 sum x^2 for the optima whose cost is
exactly zero (k = n: a centroid taken from a prefix difference is off by that relative amount);
centroids within 1e-6 relative (they are float32: 6e-8).
"""
import functools

import numpy as np
import pytest
import torch

import kmeans1d_ref as R

pytestmark = pytest.mark.gpu

GENS = ("lognormal", "gamma", "absn3")


def _draw(gen, rng, shape):
    if gen == "lognormal":
        return rng.lognormal(-6.0, 1.0, shape)
    if gen == "gamma":
        return rng.gamma(0.5, 1e-3, shape)
    return np.abs(rng.standard_normal(shape)) ** 3 * 1e-3


@functools.lru_cache(maxsize=None)
def _triu_case(gen, seed, C):
    """sorted float32 flattening of triu(u, 1), and the brute-force DP over it (all k at once)"""
    u = _draw(gen, np.random.default_rng(seed), (C, C))
    x = np.sort(np.triu(u, 1).astype(np.float32).ravel())
    return x, R.BruteDP(x, 50 if C == 32 else 5)


@functools.lru_cache(maxsize=None)
def _ragged_case(n):
    x = np.sort(_draw(GENS[n % 3], np.random.default_rng(100 + n), n).astype(np.float32))
    return x, R.BruteDP(x, min(n, 5))


def _run(dev, x, k):
    from dgvcc_amd import kernels as K
    b, c, cost = K.kmeans1d(torch.from_numpy(x).to(dev), k)
    torch.cuda.synchronize()
    return b.cpu().tolist(), c.cpu().numpy().astype(np.float64), float(cost.item())


def _check(dev, x, dp, k):
    bounds, cent, cost = _run(dev, x, k)
    ref_cost = dp.cost(k)
    n, sx2 = len(x), float((x.astype(np.float64) ** 2).sum())
    print(f"n={n} k={k} cost dev {cost:.17g} ref {ref_cost:.17g} rel {abs(cost - ref_cost) / max(ref_cost, 1e-300):.3g}")
    assert bounds == dp.bounds(k)
    assert abs(cost - ref_cost) <= 1e-9 * ref_cost + (n * 2.0 ** -53) ** 2 * sx2
    assert np.allclose(cent, dp.centroids(k), rtol=1e-6, atol=0.0)


# ---- a. exactness against the brute-force DP ------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("C", [16, 32, 64, 128])
def test_exact_on_triu_variances(dev, C, gen, seed):
    x, dp = _triu_case(gen, seed, C)
    for k in (1, 2, 3, 5) + ((50,) if C == 32 else ()):
        _check(dev, x, dp, k)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 257, 1000, 4133])
def test_exact_on_ragged_sizes(dev, n):
    x, dp = _ragged_case(n)
    for k in sorted({k for k in (1, 2, 3, 5, n) if k <= min(n, 5)}):  # k = n included where n <= 5
        _check(dev, x, dp, k)


# ---- b. full size with a known answer -------------------------------------------------------
def test_full_size_known_groups(dev):
    C = 512
    rng = np.random.default_rng(7)
    grp = rng.choice(3, size=(C, C), p=(0.5, 0.3, 0.2))
    a = np.array([1e-4, 1e-2, 1.0])[grp]
    u = np.triu(a * (1.0 + 1e-3 * rng.random((C, C))), 1).astype(np.float32)
    x = np.sort(u.ravel())
    up = np.triu(np.ones((C, C), dtype=bool), 1)
    sizes = [int((~up).sum())] + [int((grp[up] == g).sum()) for g in range(3)]
    edges = [0] + np.cumsum(sizes).tolist()  # {structural zeros, group 1, group 2, group 3}
    assert edges[-1] == C * C == 1 << 18 and len(set(sizes)) == 4
    # k = 4.  The four groups themselves are NOT the optimum for this data: group 3 spreads over
    # 1e-3 in absolute terms, ten times group 1's distance from zero, so halving group 3 saves
    # 3/4 of its 2.18e-3 while absorbing group 1 into the zeros costs 4.4e-4.  What must hold:
    # the boundaries between groups 1|2 and 2|3 are forced (0.01 and 1 apart), the four-group
    # partition is feasible so the optimum costs no more, and the device's answer is the exhaustive
    # minimum over every boundary triple within +-64 of it and over each boundary's whole gap.
    b4, c4, cost4 = _run(dev, x, 4)
    groups4 = R.exact_cost(x, edges)
    print("k=4 device", b4, cost4, "four groups", groups4)
    assert edges[2] in b4 and edges[3] in b4
    assert cost4 <= groups4 * (1 + 1e-9)
    wb, wcost = R.windowed(x, b4, 64)
    assert wb == b4 and abs(cost4 - wcost) <= 1e-9 * wcost
    assert [R.best_single_boundary(x, b4, d) for d in (1, 2, 3)] == b4[1:-1]
    assert np.allclose(c4, [x[a_:b_].astype(np.float64).mean() for a_, b_ in zip(b4[:-1], b4[1:])],
                       rtol=1e-6, atol=0.0)
    # k = 3: the optimum merges one adjacent pair; the cheapest of the three merges, in float64
    merges = [edges[:i] + edges[i + 1:] for i in (1, 2, 3)]
    costs = [R.exact_cost(x, m) for m in merges]
    best = int(np.argmin(costs))
    b3, _, cost3 = _run(dev, x, 3)
    print("k=3 merge costs", costs, "device", cost3)
    assert b3 == merges[best]
    assert abs(cost3 - costs[best]) <= 1e-9 * costs[best]


# ---- c. mask kernel ---------------------------------------------------------------------------
def test_cluster_mask(dev):
    from dgvcc_amd import kernels as K
    C = 64
    rng = np.random.default_rng(3)
    v = torch.from_numpy(np.triu(rng.lognormal(-6.0, 1.0, (C, C)), 1).astype(np.float32)).to(dev)
    srt = torch.sort(v.flatten()).values
    bounds, _, _ = K.kmeans1d(srt, 3)
    mask, ns = K.iw_cluster_mask(v, srt, bounds)
    b1 = int(bounds[1].item())
    want = (v > srt[b1 - 1]).float()
    assert mask.shape == v.shape and torch.equal(mask, want)
    assert ns.item() == want.sum().item() == C * C - b1  # no ties at this boundary: the reference's top-k count
    assert mask.tril().abs().sum().item() == 0           # diagonal and lower triangle: structural zeros
    assert 0 < ns.item() < C * (C - 1) // 2
    prev = torch.from_numpy((rng.random((C, C)) < 0.5).astype(np.float32)).to(dev)
    prev0 = prev.clone()
    mask2, ns2 = K.iw_cluster_mask(v, srt, bounds, prev)
    assert torch.equal(mask2, (prev0.int() & want.int()).float())
    assert ns2.item() == mask2.sum().item() and 0 < ns2.item() < ns.item()
    assert torch.equal(prev, prev0)  # prev_mask is only read


def test_cluster_mask_ties_stay_in_cluster_0(dev):
    """A run of equal values never straddles the mask: everything equal to cluster 0's largest value
    is masked out.  (i) a constant block plus two spread groups, k = 3: the first boundary is the
    block's end.  (ii) three constant blocks, k = 4: every split of a block costs 0, the leftmost
    boundaries win, so the first boundary falls inside the first block ([0, 1, 40, 70, 90]; all sums
    are exact in binary) and the reference's top-k count n - 1 would keep 39 of its 40 equal values:
    here the whole block is 0."""
    from dgvcc_amd import kernels as K
    rng = np.random.default_rng(11)
    blk = np.full(40, 0.5)
    vals = np.concatenate([blk, 2.0 + 0.01 * rng.random(30), 8.0 + 0.01 * rng.random(20)]).astype(np.float32)
    const = np.concatenate([blk, np.full(30, 2.0), np.full(20, 8.0)]).astype(np.float32)
    for x, k, want_bounds in ((vals, 3, [0, 40, 70, 90]), (const, 4, [0, 1, 40, 70, 90])):
        assert R.BruteDP(np.sort(x), k).bounds(k) == want_bounds
        v = torch.from_numpy(x[rng.permutation(len(x))]).to(dev)
        srt = torch.sort(v).values
        bounds, _, _ = K.kmeans1d(srt, k)
        assert bounds.cpu().tolist() == want_bounds
        mask, ns = K.iw_cluster_mask(v, srt, bounds)
        assert torch.equal(mask, (v > 0.5).float()) and ns.item() == 50


# ---- d. the kmeans1d.cluster binding ------------------------------------------------------------
def test_cluster_binding(dev):
    from dgvcc_amd import kmeans1d
    rng = np.random.default_rng(21)
    x = rng.lognormal(-6.0, 1.0, 1000).astype(np.float32)  # unsorted
    order = np.argsort(x, kind="stable")
    dp = R.BruteDP(x[order], 5)
    for k in (1, 3, 5):
        got = kmeans1d.cluster(x, k)
        clusters, centroids = got  # unpacks like the reference's call
        assert isinstance(clusters, list) and isinstance(centroids, list)
        assert len(clusters) == 1000 and len(centroids) == k and all(isinstance(c, int) for c in clusters)
        want = np.empty(1000, dtype=np.int64)
        want[order] = dp.labels(k)
        assert clusters == want.tolist()
        assert centroids == sorted(centroids) and np.allclose(centroids, dp.centroids(k), rtol=1e-6, atol=0.0)
        assert clusters.count(0) == dp.bounds(k)[1]
        for other in (x.tolist(), torch.from_numpy(x), torch.from_numpy(x).to(dev)):
            assert kmeans1d.cluster(other, k) == got


# ---- e. ISWCounter_ResNet(relax_denom=0) end to end ------------------------------------------
def test_isw_relax_denom_0_end_to_end(dev):
    from oracle import dg_oracle as O
    from oracle import trunk_oracle as TO
    from dgvcc_amd import kernels as K
    from dgvcc_amd.models.trunks import ISWCounter_ResNet
    torch.manual_seed(0)
    model = ISWCounter_ResNet(relax_denom=0, clusters=3, pretrained=False)
    model.load_state_dict(O.seeded_state_dict(model.state_dict()))
    model = model.to(dev).set_precision("fp32")
    img1, img2, (_, dmaps, _) = O.synthetic_batch(2, 64, 64, seed=2112)
    views = [img1.to(dev), img2.to(dev)]

    def stats_pass(vs):
        model.eval()
        with torch.no_grad():
            for _ in range(2):
                assert model(vs, cal_covstat=True) == 0
        return [(cm.var_matrix / cm.count_var_cov).cpu().numpy() for cm in model.cov_matrix_layer]

    def set_mask_no_sync():
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")  # any device-to-host copy or .item() raises
        try:
            model.set_mask_matrix()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()

    # steps 1-3, 8: two cal_covstat calls, the mask on device without a host copy, the brute force
    # on the device's own variances
    vars1 = stats_pass(views)
    assert [v.shape[0] for v in vars1] == [64, 256, 512]
    set_mask_no_sync()
    masks1 = []
    for var, cm in zip(vars1, model.cov_matrix_layer):
        assert cm.var_matrix is None and cm.count_var_cov == 0
        x = np.sort(var.ravel())
        n = len(x)
        # the device's own clustering of the same values (set_mask_matrix keeps only mask and centroids)
        srt = torch.sort(torch.from_numpy(var).to(dev).flatten()).values
        assert np.array_equal(srt.cpu().numpy(), x)
        db, dc, dcost = K.kmeans1d(srt, 3)
        db, dcost = db.cpu().tolist(), float(dcost.item())
        if n <= 4096:
            dp = R.BruteDP(x, 3)
            bounds, cost = dp.bounds(3), dp.cost(3)
        else:  # beyond the exhaustive range: every boundary pair within +-64 of the device's
            bounds, cost = R.windowed(x, db, 64)
            assert cost >= dcost * (1 - 1e-9), (cost, dcost)  # the window holds nothing better
        print(f"C={var.shape[0]} bounds dev {db} ref {bounds} cost dev {dcost:.17g} ref {cost:.17g}")
        assert db == bounds and abs(dcost - cost) <= 1e-9 * cost
        want = (var > x[bounds[1] - 1]).astype(np.float32)
        got = cm.mask_matrix.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want)
        assert float(cm.num_sensitive.item()) == want.sum() > 0
        assert np.array_equal(cm.centroids.cpu().numpy(), dc.cpu().numpy()) and cm.centroids.is_cuda
        masks1.append(cm.mask_matrix.clone())

    # steps 4-6: training forward with the whitening loss against the float64 oracle on the device's
    # own whitened maps and that mask
    model.train()
    losses = model(views[0], gts=dmaps.to(dev), apply_wtloss=True)
    with torch.no_grad():
        _, ws = model._get_plan().features(views[0], model.compute_dtype, True, None)
    ref = sum(TO.whitening_loss(w.buf.permute(0, 3, 1, 2).double().cpu(), m.double().cpu(),
                                float(m.sum().item())) for w, m in zip(ws, masks1)) / len(ws)
    wt = float(losses[1].item())
    print("wt_loss dev", wt, "float64 oracle", float(ref))
    assert abs(wt - float(ref)) <= 1e-5 * abs(float(ref))
    (losses[0] + 0.6 * losses[1]).sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.layer1.parameters())

    # step 7: a second statistics pass (other views) without a reset ANDs with the first mask, as the
    # reference's set_mask_matrix does from the second epoch on; after reset_mask_matrix() (which
    # drops the mask, cov_settings.py:49-50) the same statistics give the fresh mask alone
    views2 = [views[1].flip(-1), views[0] * 0.5]
    vars2 = stats_pass(views2)
    set_mask_no_sync()
    anded = [cm.mask_matrix.clone() for cm in model.cov_matrix_layer]
    assert all(float(cm.num_sensitive.item()) == float(m.sum().item())
               for cm, m in zip(model.cov_matrix_layer, anded))
    model.reset_mask_matrix()
    assert all(cm.mask_matrix is None for cm in model.cov_matrix_layer)
    vars2b = stats_pass(views2)
    model.train()
    model(views[0], gts=dmaps.to(dev), apply_wtloss=True)  # get_mask_matrix sets the mask on first use
    for var, varb, m1, m12, cm in zip(vars2, vars2b, masks1, anded, model.cov_matrix_layer):
        assert np.array_equal(var, varb)
        fresh = cm.mask_matrix
        assert torch.equal(m12, (m1.int() & fresh.int()).float())
        assert not torch.equal(fresh, m1)  # the second pass did cluster other statistics
        assert float(cm.num_sensitive.item()) == float(fresh.sum().item())
