"""Yardstick of the k-means tests: optimal 1-D k-means by an exhaustive float64 dynamic programme
in numpy.  Every row is filled, every boundary i < j is tried for every j (no monotonicity, no
divide and conquer), the leftmost minimum wins: O(k n^2).  None of the package's code is used.

    D[1][j] = cost(0, j),  D[r][j] = min_{r-1 <= i < j} D[r-1][i] + cost(i, j)
    cost(i, j) = max(0, P2[j] - P2[i] - (P1[j] - P1[i])^2 / (j - i))  over elements i .. j-1
"""
import numpy as np


def prefix(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([[0.0], np.cumsum(x)]), np.concatenate([[0.0], np.cumsum(x * x)])


def exact_cost(x, bounds):
    """sum over clusters of sum (x - mean)^2, two-pass in float64 (no prefix-sum cancellation)."""
    x = np.asarray(x, dtype=np.float64)
    return float(sum(((x[a:b] - x[a:b].mean()) ** 2).sum() for a, b in zip(bounds[:-1], bounds[1:])))


class BruteDP:
    """All rows 1 .. kmax over the ascending values x; bounds(k) / cost(k) for any k <= kmax."""

    def __init__(self, x, kmax, chunk=256):
        self.x = np.asarray(x, dtype=np.float64)
        n = self.n = len(self.x)
        assert np.all(np.diff(self.x) >= 0) and 1 <= kmax <= n
        self.kmax = kmax
        p1, p2 = prefix(self.x)
        idx = np.arange(n + 1)
        D = np.full((kmax + 1, n + 1), np.inf)
        opt = np.zeros((kmax + 1, n + 1), dtype=np.int64)
        # D[r][j] = inf for j < r (and D[r][0] for every r): no boundary below r-1 is ever chosen
        with np.errstate(divide="ignore", invalid="ignore"):
            D[1, 1:] = np.maximum(p2[1:] - p1[1:] ** 2 / idx[1:], 0.0)
            for j0 in range(1, n + 1 if kmax > 1 else 0, chunk):
                j = idx[j0:min(n + 1, j0 + chunk)][:, None]  # rows: targets j
                i = idx[None, :j[-1, 0]]                      # columns: every boundary i
                c = p1[j] - p1[i]
                c *= c
                c /= j - i
                np.subtract(p2[j] - p2[i], c, out=c)
                np.maximum(c, 0.0, out=c)                     # cost(i, j), shared by the rows
                c[i >= j] = np.inf
                rows = np.arange(len(j))
                for r in range(2, kmax + 1):                  # row r-1 of this chunk is done by now
                    v = c + D[r - 1][i]
                    a = np.argmin(v, axis=1)                  # first (leftmost) minimum
                    D[r, j[:, 0]] = v[rows, a]
                    opt[r, j[:, 0]] = a
        self.D, self.opt = D, opt

    def bounds(self, k):
        b = [self.n]
        for r in range(k, 1, -1):
            b.append(int(self.opt[r, b[-1]]))
        return [0] + b[::-1]

    def cost(self, k):
        return exact_cost(self.x, self.bounds(k))

    def centroids(self, k):
        b = self.bounds(k)
        return [float(self.x[a:c].mean()) for a, c in zip(b[:-1], b[1:])]

    def labels(self, k):
        """cluster index of every sorted position"""
        b = self.bounds(k)
        return np.repeat(np.arange(k), np.diff(b))


def _pair_cost(p1, p2, i, j):
    with np.errstate(divide="ignore", invalid="ignore"):
        s1, s2 = p1[j] - p1[i], p2[j] - p2[i]
        return np.where(i < j, np.maximum(s2 - s1 * s1 / (j - i), 0.0), np.inf)


def windowed(x, near, half=64):
    """Best partition whose inner boundaries each lie within +-half of those of `near` ([0, b1, ..,
    n], 2 or 3 inner boundaries), exhaustively over every combination, from float64 prefix sums:
    (bounds, cost).  For n beyond BruteDP's range."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    p1, p2 = prefix(x)
    inner = near[1:-1]
    axes = []
    for d, b in enumerate(inner):
        shape = [1] * len(inner)
        shape[d] = -1
        axes.append(np.arange(max(d + 1, b - half), min(n - len(inner) + d, b + half) + 1).reshape(shape))
    edges = [np.zeros([1] * len(inner), dtype=np.int64)] + axes + [np.full([1] * len(inner), n)]
    v = sum(_pair_cost(p1, p2, a, b) for a, b in zip(edges[:-1], edges[1:]))
    at = np.unravel_index(np.argmin(v), v.shape)
    bounds = [0] + [int(ax.ravel()[i]) for ax, i in zip(axes, at)] + [n]
    return bounds, exact_cost(x, bounds)


def best_single_boundary(x, bounds, d):
    """The best position of inner boundary d (1-based) anywhere between its two neighbours, the
    others held: exhaustive over the whole gap."""
    x = np.asarray(x, dtype=np.float64)
    p1, p2 = prefix(x)
    lo, hi = bounds[d - 1], bounds[d + 1]
    i = np.arange(lo + 1, hi)
    v = _pair_cost(p1, p2, np.int64(lo), i) + _pair_cost(p1, p2, i, np.int64(hi))
    return int(i[np.argmin(v)])
