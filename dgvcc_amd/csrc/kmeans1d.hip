// Optimal 1-D k-means on device, and the ISW sensitive-covariance mask made from it
// (models/ISW/cov_settings.py:57-61: `kmeans1d.cluster(var_flatten, clusters)`, the relax_denom = 0
// setting of CovMatrix_ISW.set_mask_matrix).
//
// Optimal 1-D k-means is a defined optimum, not one package's output: the partition of the sorted values
// into k contiguous non-empty runs with the least within-cluster sum of squares.  With float64 prefix
// sums P1 (of x) and P2 (of x^2), cost(i, j) = max(0, P2[j] - P2[i] - (P1[j] - P1[i])^2 / (j - i)) over
// elements i .. j-1, and
//     D[1][j] = cost(0, j),    D[r][j] = min_{r-1 <= i < j} D[r-1][i] + cost(i, j),   leftmost i on ties.
// The cost is concave Monge, so the leftmost argmin opt[r][j] is monotone in j and a row is filled by
// level-synchronous divide and conquer: with 2^m > n, level L (stride s = 2^(m-L-1)) computes
// j = s, 3s, 5s, ... <= n, each over the candidates [opt[r][j-s], opt[r][j+s]] that the earlier levels
// left (the row's trivial bounds r-1 and j-1 at the ends), so a level looks at <= n + nodes candidates.
// Row k is needed at j = n only: one node over every candidate.  k-2 rows x m launches in all.
//
// Every loop here is bounded by n and k whatever the data holds: candidate ranges are clamped into
// [0, j-1] before they are walked and the backtrack clamps each boundary into [r-1, j-1], so a NaN
// input (torch.var over a batch of 1) gives a meaningless partition but every launch ends and stays
// inside its buffers.  Reductions are fixed-order (no atomics): results are run-to-run identical.
#include "dg_common.h"
#include <algorithm>

namespace {

constexpr int KM_MAX_K = 64;
constexpr int KM_MAX_N = 1 << 20;
constexpr int KM_EPB = 1024;                     // elements per block of the scan / cost / mask passes
constexpr int KM_MAX_BLOCKS = KM_MAX_N / KM_EPB;  // 1024: partials any of those passes leave

// workspace: P1, P2, two D rows ([n+1] doubles each), block totals [2][KM_MAX_BLOCKS] and partials
// [KM_MAX_BLOCKS] (doubles), then the argmin table opt[k][n+1] (int32; row r at index r-1)
struct KmWs {
  double *p1, *p2, *d0, *d1, *tot, *part;
  int* opt;
};
inline int64_t km_ws_doubles(int n) { return 4 * ((int64_t)n + 1) + 3 * KM_MAX_BLOCKS; }
inline KmWs km_carve(void* ws, int n) {
  KmWs w;
  const int64_t n1 = (int64_t)n + 1;
  w.p1 = (double*)ws;
  w.p2 = w.p1 + n1;
  w.d0 = w.p2 + n1;
  w.d1 = w.d0 + n1;
  w.tot = w.d1 + n1;
  w.part = w.tot + 2 * KM_MAX_BLOCKS;
  w.opt = (int*)(w.part + KM_MAX_BLOCKS);
  return w;
}

__device__ __forceinline__ double km_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum of a and of b over a 256-thread block, returned to every thread (fixed order)
__device__ __forceinline__ void block_sum2_d(double& a, double& b) {
  __shared__ double red[2][4];
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) { red[0][w] = a; red[1][w] = b; }
  __syncthreads();
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// tot[0][b], tot[1][b] = sum x, sum x^2 over block b's KM_EPB elements
__global__ __launch_bounds__(256) void km_block_totals(const float* __restrict__ x, int n, double* __restrict__ tot) {
  const int e0 = blockIdx.x * KM_EPB + threadIdx.x * 4;
  double a = 0.0, b = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (e0 + q < n) {
      const double v = (double)x[e0 + q];
      a += v;
      b += v * v;
    }
  }
  block_sum2_d(a, b);
  if (threadIdx.x == 0) {
    tot[blockIdx.x] = a;
    tot[KM_MAX_BLOCKS + blockIdx.x] = b;
  }
}

// p1[j], p2[j] = sum of x, x^2 over elements 0 .. j-1 (j = 0 .. n): the carried totals of the blocks
// before this one, then a block scan (thread: 4 consecutive elements; wave: shuffle scan; waves: LDS)
__global__ __launch_bounds__(256) void km_prefix(const float* __restrict__ x, int n, const double* __restrict__ tot,
                                                 double* __restrict__ p1, double* __restrict__ p2) {
  __shared__ double wt[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double c1 = 0.0, c2 = 0.0;
  for (int b = tid; b < (int)blockIdx.x; b += 256) {
    c1 += tot[b];
    c2 += tot[KM_MAX_BLOCKS + b];
  }
  block_sum2_d(c1, c2);
  const int e0 = blockIdx.x * KM_EPB + tid * 4;
  double a[4], b[4];
  double ta = 0.0, tb = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double v = e0 + q < n ? (double)x[e0 + q] : 0.0;
    ta += v;
    tb += v * v;
    a[q] = ta;
    b[q] = tb;
  }
  double sa = ta, sb = tb;  // inclusive scan of the thread totals over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double ua = __shfl_up(sa, o, 64), ub = __shfl_up(sb, o, 64);
    if (lane >= o) { sa += ua; sb += ub; }
  }
  if (lane == 63) { wt[0][w] = sa; wt[1][w] = sb; }
  __syncthreads();
  double ba = c1 + (sa - ta), bb = c2 + (sb - tb);
  for (int u = 0; u < w; ++u) { ba += wt[0][u]; bb += wt[1][u]; }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (e0 + q < n) {
      p1[e0 + q + 1] = ba + a[q];
      p2[e0 + q + 1] = bb + b[q];
    }
  }
  if (blockIdx.x == 0 && tid == 0) { p1[0] = 0.0; p2[0] = 0.0; }
}

__device__ __forceinline__ double km_cost(double s1, double s2, int m) {
  const double c = s2 - s1 * s1 / (double)m;
  return c > 0.0 ? c : 0.0;
}

// row 1: D[1][j] = cost(0, j); D[.][0] = inf in both row buffers (no row has an empty prefix)
__global__ __launch_bounds__(256) void km_row1(const double* __restrict__ p1, const double* __restrict__ p2, int n,
                                               double* __restrict__ d, double* __restrict__ dother) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > n) return;
  if (j == 0) {
    d[0] = km_inf();
    dother[0] = km_inf();
  } else {
    d[j] = km_cost(p1[j], p2[j], j);
  }
}

// candidates i = lo + t, lo + t + T, .. <= hi of node j for one of T threads: its least value and that
// value's leftmost i (ascending, strict <), (inf, lo) where it has none
__device__ __forceinline__ void km_scan(const double* __restrict__ p1, const double* __restrict__ p2,
                                        const double* __restrict__ dprev, int j, int lo, int hi, int t, int T, double& bv,
                                        int& bi) {
  const double pj1 = p1[j], pj2 = p2[j];
  bv = km_inf();
  bi = lo;
#pragma unroll 4
  for (int i = lo + t; i <= hi; i += T) {
    const double v = dprev[i] + km_cost(pj1 - p1[i], pj2 - p2[i], j - i);
    if (v < bv) { bv = v; bi = i; }
  }
}
__device__ __forceinline__ bool km_better(double av, int ai, double bv, int bi) {
  return av < bv || (av == bv && ai < bi);
}
__device__ __forceinline__ void km_wave_argmin(double& bv, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (km_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
}

// Nodes j = j0 + node * step (node < count) of row r at stride s: dcur[j] = min_i dprev[i] + cost(i, j)
// and opt[j] = its leftmost argmin over i in [max(r-1, opt[j-s]), min(j-1, opt[j+s])].  A block of 16
// waves takes 16 consecutive nodes: a wave walks its own node's candidates when they are few (the
// usual case deep in the recursion), and the whole block walks, one after the other, the nodes of its
// 16 whose range is long (the shallow levels, and at every level the node that brackets a jump of the
// argmin: past a run of equal values, the structural zeros, the argmin jumps by the run's length).
constexpr int KM_NPB = 16;      // nodes (waves) per block
constexpr int KM_SHORT = 512;   // candidates a wave walks alone
__global__ __launch_bounds__(64 * KM_NPB) void km_nodes(const double* __restrict__ p1, const double* __restrict__ p2,
                                                        const double* __restrict__ dprev, double* __restrict__ dcur,
                                                        int* __restrict__ opt, int n, int r, int s, int j0, int step,
                                                        int count) {
  __shared__ int slo[KM_NPB], shi[KM_NPB];  // the block's long nodes' ranges (hi < lo: none)
  __shared__ double sv[KM_NPB];
  __shared__ int si[KM_NPB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int node0 = blockIdx.x * KM_NPB;
  const bool live = node0 + w < count;
  const int j = j0 + (live ? node0 + w : 0) * step;
  int lo = r - 1, hi = j - 1;
  if (j - s >= 1) lo = max(lo, opt[j - s]);
  if ((long long)j + s <= n) hi = min(hi, opt[j + s]);
  lo = max(0, min(lo, j - 1));
  hi = max(hi, lo);
  const bool alone = hi - lo < KM_SHORT;
  if (lane == 0) {
    slo[w] = lo;
    shi[w] = live && !alone ? hi : lo - 1;
  }
  if (live && alone) {
    double bv;
    int bi;
    km_scan(p1, p2, dprev, j, lo, hi, lane, 64, bv, bi);
    km_wave_argmin(bv, bi);
    if (lane == 0) {
      dcur[j] = bv;
      opt[j] = bi;
    }
  }
  __syncthreads();
  for (int u = 0; u < KM_NPB; ++u) {
    const int ulo = slo[u], uhi = shi[u];
    if (uhi < ulo) continue;  // the same for every thread of the block
    const int uj = j0 + (node0 + u) * step;
    double bv;
    int bi;
    km_scan(p1, p2, dprev, uj, ulo, uhi, threadIdx.x, 64 * KM_NPB, bv, bi);
    km_wave_argmin(bv, bi);
    if (lane == 0) { sv[w] = bv; si[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < KM_NPB; ++q)
        if (km_better(sv[q], si[q], bv, bi)) { bv = sv[q]; bi = si[q]; }
      dcur[uj] = bv;
      opt[uj] = bi;
    }
    __syncthreads();
  }
}

// bounds[0 .. k] by following opt from j = n (boundary r-1 clamped into [r-1, bounds[r] - 1]), and the
// centroids from the prefix sums
__global__ __launch_bounds__(64) void km_backtrack(const int* __restrict__ opt, int n, int k, const double* __restrict__ p1,
                                                   int* __restrict__ bounds, float* __restrict__ centroids) {
  __shared__ int sb[KM_MAX_K + 1];
  if (threadIdx.x == 0) {
    int j = n;
    sb[k] = n;
    for (int r = k; r >= 2; --r) {
      const int i = opt[(long long)(r - 1) * (n + 1) + j];
      j = max(r - 1, min(i, j - 1));
      sb[r - 1] = j;
    }
    sb[0] = 0;
  }
  __syncthreads();
  for (int c = threadIdx.x; c <= k; c += 64) {
    bounds[c] = sb[c];
    if (c < k && centroids) centroids[c] = (float)((p1[sb[c + 1]] - p1[sb[c]]) / (double)(sb[c + 1] - sb[c]));
  }
}

// The total cost again from the values themselves, sum (x - centroid)^2: the prefix-sum form loses
// |P2| 2^-53 per difference, which for tight clusters far from zero is not small against the cost.
__global__ __launch_bounds__(256) void km_cost_partial(const float* __restrict__ x, int n, int k, const int* __restrict__ bounds,
                                                       const double* __restrict__ p1, double* __restrict__ part) {
  __shared__ int sb[KM_MAX_K + 1];
  __shared__ double sc[KM_MAX_K];
  for (int c = threadIdx.x; c <= k; c += 256) sb[c] = bounds[c];
  __syncthreads();
  for (int c = threadIdx.x; c < k; c += 256) sc[c] = (p1[sb[c + 1]] - p1[sb[c]]) / (double)(sb[c + 1] - sb[c]);
  __syncthreads();
  double acc = 0.0, unused = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = blockIdx.x * KM_EPB + q * 256 + threadIdx.x;
    if (e < n) {
      int c = 0;
      for (int u = 1; u < k; ++u) c += e >= sb[u] ? 1 : 0;
      const double d = (double)x[e] - sc[c];
      acc += d * d;
    }
  }
  block_sum2_d(acc, unused);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void km_cost_final(const double* __restrict__ part, int nb, double* __restrict__ cost) {
  double acc = 0.0, unused = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) acc += part[b];
  block_sum2_d(acc, unused);
  if (threadIdx.x == 0) cost[0] = acc;
}

// mask[e] = v[e] > (the largest value of cluster 0) [& prev[e]]; ipart[b] = the block's count
__global__ __launch_bounds__(256) void km_mask(const float* __restrict__ v, const float* __restrict__ sorted,
                                               const int* __restrict__ bounds, int n, const float* prev, float* mask,
                                               int* __restrict__ ipart) {
  __shared__ int red[4];
  const float thr = sorted[max(0, min(bounds[1] - 1, n - 1))];
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = blockIdx.x * KM_EPB + q * 256 + threadIdx.x;
    if (e < n) {
      int m = v[e] > thr ? 1 : 0;
      if (prev) m &= (int)prev[e];
      mask[e] = (float)m;
      cnt += m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) ipart[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void km_mask_final(const int* __restrict__ ipart, int nb, float* __restrict__ num_sensitive) {
  __shared__ int red[4];
  int cnt = 0;
  for (int b = threadIdx.x; b < nb; b += 256) cnt += ipart[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) num_sensitive[0] = (float)(red[0] + red[1] + red[2] + red[3]);
}

// one level of a row, or the last row's single node
void km_launch_nodes(hipStream_t st, const KmWs& w, const double* dprev, double* dcur, int* opt, int n, int r, int s,
                     int j0, int step, int count) {
  hipLaunchKernelGGL(km_nodes, dim3(dg_cdiv(count, KM_NPB)), dim3(64 * KM_NPB), 0, st, w.p1, w.p2, dprev, dcur, opt, n, r,
                     s, j0, step, count);
}

}  // namespace

// ================================================================ C-ABI ====
extern "C" int64_t dg_kmeans1d_workspace(int n, int k) {
  if (k < 1 || n < k) return DG_ERR_INVALID;
  if (k > KM_MAX_K || n > KM_MAX_N) return DG_ERR_UNSUPPORTED;
  const int64_t bytes = km_ws_doubles(n) * 8 + (int64_t)k * ((int64_t)n + 1) * 4;
  return (bytes + 255) & ~(int64_t)255;
}

extern "C" int dg_kmeans1d(const float* sorted, int n, int k, int* bounds, float* centroids, double* cost,
                           void* workspace, void* stream) {
  DG_REQUIRE(sorted && bounds && workspace && k >= 1 && n >= k);
  DG_SUPPORTED(k <= KM_MAX_K && n <= KM_MAX_N);
  hipStream_t st = (hipStream_t)stream;
  const KmWs w = km_carve(workspace, n);
  const int nb = dg_cdiv(n, KM_EPB);
  hipLaunchKernelGGL(km_block_totals, dim3(nb), dim3(256), 0, st, sorted, n, w.tot);
  DG_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_prefix, dim3(nb), dim3(256), 0, st, sorted, n, (const double*)w.tot, w.p1, w.p2);
  DG_CHECK_LAUNCH();
  if (k >= 2) {
    double *dprev = w.d0, *dcur = w.d1;
    hipLaunchKernelGGL(km_row1, dim3(dg_cdiv((long long)n + 1, 256)), dim3(256), 0, st, (const double*)w.p1,
                       (const double*)w.p2, n, dprev, dcur);
    DG_CHECK_LAUNCH();
    int m = 0;
    while ((1 << m) <= n) ++m;  // 2^m > n: every j in 1 .. n is an odd multiple of one stride 2^(m-L-1)
    for (int r = 2; r < k; ++r) {
      int* opt = w.opt + (int64_t)(r - 1) * ((int64_t)n + 1);
      for (int L = 0; L < m; ++L) {
        const int s = 1 << (m - L - 1);
        const int count = (n / s + 1) / 2;
        if (count == 0) continue;
        km_launch_nodes(st, w, dprev, dcur, opt, n, r, s, s, 2 * s, count);
        DG_CHECK_LAUNCH();
      }
      std::swap(dprev, dcur);
    }
    // row k at j = n alone: stride n + 1 leaves it the row's trivial bounds
    km_launch_nodes(st, w, dprev, dcur, w.opt + (int64_t)(k - 1) * ((int64_t)n + 1), n, k, n + 1, n, 1, 1);
    DG_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(km_backtrack, dim3(1), dim3(64), 0, st, (const int*)w.opt, n, k, (const double*)w.p1, bounds,
                     centroids);
  DG_CHECK_LAUNCH();
  if (cost) {
    hipLaunchKernelGGL(km_cost_partial, dim3(nb), dim3(256), 0, st, sorted, n, k, (const int*)bounds,
                       (const double*)w.p1, w.part);
    DG_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_cost_final, dim3(1), dim3(256), 0, st, (const double*)w.part, nb, cost);
    DG_CHECK_LAUNCH();
  }
  return DG_OK;
}

extern "C" int dg_iw_cluster_mask(const float* v, const float* sorted, const int* bounds, int n, const float* prev_mask,
                                  float* mask, float* num_sensitive, void* workspace, void* stream) {
  DG_REQUIRE(v && sorted && bounds && mask && num_sensitive && workspace && n >= 1);
  DG_SUPPORTED(n <= KM_MAX_N);
  hipStream_t st = (hipStream_t)stream;
  const int nb = dg_cdiv(n, KM_EPB);
  hipLaunchKernelGGL(km_mask, dim3(nb), dim3(256), 0, st, v, sorted, bounds, n, prev_mask, mask, (int*)workspace);
  DG_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_mask_final, dim3(1), dim3(256), 0, st, (const int*)workspace, nb, num_sensitive);
  DG_CHECK_LAUNCH();
  return DG_OK;
}
