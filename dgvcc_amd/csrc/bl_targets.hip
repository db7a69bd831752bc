// Per-point targets of the Bayesian loss (reference datasets/bay_dataset.py:38-48, 85-98) and the
// strided sum pool that brings a full-resolution density map onto the loss's grid.
//
// dg_bl_targets, per image with n annotations p_i (crop coordinates, unfiltered):
//   d_i   = n == 1: 4;  n >= 4: mean of the 2nd..4th smallest of row i of the distance matrix (self
//           and duplicates count as zeros);  n == 2, 3: mean of dist(i, k), k = 1..n-1 by index
//           (the reference's dists[:, 1:] on the unsorted matrix);
//   s_i   = clip(d_i, 4, 128), box = p_i +- s_i / 2;
//   ratio = clip(area(box ^ [0, w] x [0, h]) / s_i^2, 0, 1);  kept when ratio >= 0.3.
// Distances are f32 in difference form, sqrtf(dx*dx + dy*dy); the minima are tracked on the squares
// (sqrt is monotonic), so only the four survivors are rooted.  The overlap along an axis is taken
// relative to the point, min(w - x, s/2) - max(-x, -s/2), which keeps the rounding at the scale of
// s whatever the magnitude of x.
// The compaction is stable and has no atomics: one tile of NT points per block (ordered by image,
// then tile), a block scan of the keep flags, one scan over the tiles' counts, a scatter.
#include "dg_common.h"

namespace {

constexpr int NT = 256;
constexpr float KEEP_RATIO = 0.3f;

struct TgArgs {
  const float* pts;       // [total][2] (x, y)
  const int64_t* offs;    // [B+1]
  int64_t total;
  int B;
  int max_tiles;         // blocks of the launch = room of tcnt / tbase
  float h, w;
  const float* flips;     // flag of image b at flips[b * flip_stride]
  int flip_stride;
  float* ratio;           // [total] workspace
  int* rank;              // [total] rank of a kept point among its tile's kept points
  int* tcnt;              // [tiles] kept points per tile
  int* tbase;             // [tiles + 1] exclusive scan of tcnt
  float* out_pts;         // [total][2]
  float* out_tg;          // [total]
  int64_t* out_offs;      // [B+1]
  float* dist_out;        // [total] or NULL: unclipped d
  float* ratio_out;       // [total] or NULL
};

// the image's point range, clamped to the packed array
__device__ __forceinline__ void img_range(const TgArgs& a, int b, int64_t& p0, int64_t& p1) {
  p0 = a.offs[b]; p1 = a.offs[b + 1];
  p0 = p0 < 0 ? 0 : (p0 > a.total ? a.total : p0);
  p1 = p1 < p0 ? p0 : (p1 > a.total ? a.total : p1);
}

__device__ __forceinline__ int tiles_of(int64_t n) { return (int)((n + NT - 1) / NT); }

// block -> (image, tile within the image); false for the spare blocks of the launch
__device__ __forceinline__ bool locate(const TgArgs& a, int blk, int& b, int& tile, int64_t& p0, int64_t& p1) {
  int acc = 0;
  for (b = 0; b < a.B; ++b) {
    img_range(a, b, p0, p1);
    const int t = tiles_of(p1 - p0);
    if (blk < acc + t) { tile = blk - acc; return true; }
    acc += t;
  }
  return false;
}

__device__ __forceinline__ float sqdist(float xi, float yi, float xj, float yj) {
  const float dx = xi - xj, dy = yi - yj;
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

// overlap of [p - hs, p + hs] with [0, lim], relative to p
__device__ __forceinline__ float axis_overlap(float p, float hs, float lim) {
  return fmaxf(fminf(lim - p, hs) - fmaxf(-p, -hs), 0.f);
}

__global__ __launch_bounds__(NT) void tg_points(TgArgs a) {
  int b, tile;
  int64_t p0, p1;
  if (!locate(a, blockIdx.x, b, tile, p0, p1)) return;
  const int64_t n = p1 - p0;
  const int64_t li = (int64_t)tile * NT + threadIdx.x;
  const bool live = li < n;
  const int64_t gi = p0 + li;
  float x = 0.f, y = 0.f;
  if (live) { x = a.pts[2 * gi]; y = a.pts[2 * gi + 1]; }

  float d;
  if (n >= 4) {
    __shared__ float sx[NT], sy[NT];
    float m0 = INFINITY, m1 = INFINITY, m2 = INFINITY, m3 = INFINITY;
    for (int64_t j0 = 0; j0 < n; j0 += NT) {
      const int64_t lj = j0 + threadIdx.x;
      __syncthreads();
      if (lj < n) { sx[threadIdx.x] = a.pts[2 * (p0 + lj)]; sy[threadIdx.x] = a.pts[2 * (p0 + lj) + 1]; }
      __syncthreads();
      const int cnt = (int)((n - j0) < NT ? (n - j0) : NT);
      for (int k = 0; k < cnt; ++k) {
        float t = sqdist(x, y, sx[k], sy[k]), u;
        u = fminf(m0, t); t = fmaxf(m0, t); m0 = u;
        u = fminf(m1, t); t = fmaxf(m1, t); m1 = u;
        u = fminf(m2, t); t = fmaxf(m2, t); m2 = u;
        m3 = fminf(m3, t);
      }
    }
    d = (sqrtf(m1) + sqrtf(m2) + sqrtf(m3)) / 3.f;
  } else if (n == 1) {
    d = 4.f;
  } else {  // n = 2, 3: columns 1.. of the unsorted matrix
    float s = 0.f;
    for (int64_t k = 1; k < n; ++k) s += sqrtf(sqdist(x, y, a.pts[2 * (p0 + k)], a.pts[2 * (p0 + k) + 1]));
    d = s / (float)(n - 1);
  }

  const float s = fminf(fmaxf(d, 4.f), 128.f);
  const float inner = axis_overlap(x, 0.5f * s, a.w) * axis_overlap(y, 0.5f * s, a.h);
  const float ratio = fminf(fmaxf(inner / (s * s), 0.f), 1.f);
  const bool keep = live && ratio >= KEEP_RATIO;
  if (live) {
    a.ratio[gi] = ratio;
    if (a.dist_out) a.dist_out[gi] = d;
    if (a.ratio_out) a.ratio_out[gi] = ratio;
  }

  // exclusive scan of the keep flags over the block: ballot within a wave, then over the 4 waves
  const unsigned long long bal = __ballot(keep);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int inwave = __popcll(bal & ((1ull << lane) - 1ull));
  __shared__ int wcnt[NT / 64];
  if (lane == 0) wcnt[wv] = __popcll(bal);
  __syncthreads();
  int before = 0;
  for (int q = 0; q < wv; ++q) before += wcnt[q];
  if (live) a.rank[gi] = before + inwave;
  if (threadIdx.x == 0) a.tcnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// one block: exclusive scan of the tiles' counts, then the images' output offsets
__global__ __launch_bounds__(NT) void tg_scan(TgArgs a) {
  __shared__ int sh[NT];
  __shared__ int carry;
  int tiles = 0;
  for (int b = 0; b < a.B; ++b) {
    int64_t p0, p1;
    img_range(a, b, p0, p1);
    tiles += tiles_of(p1 - p0);
  }
  tiles = tiles < a.max_tiles ? tiles : a.max_tiles;  // offsets that overlap could claim more
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int t0 = 0; t0 < tiles; t0 += NT) {
    const int t = t0 + threadIdx.x;
    const int v = t < tiles ? a.tcnt[t] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {  // Hillis-Steele inclusive scan
      const int add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    if (t < tiles) a.tbase[t] = carry + sh[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += sh[NT - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.tbase[tiles] = carry;
  __syncthreads();
  for (int b = threadIdx.x; b <= a.B; b += NT) {
    int first = 0;  // the first tile of image b (= tiles for b == B)
    for (int q = 0; q < b; ++q) {
      int64_t p0, p1;
      img_range(a, q, p0, p1);
      first += tiles_of(p1 - p0);
    }
    a.out_offs[b] = (int64_t)a.tbase[first < tiles ? first : tiles];
  }
}

__global__ __launch_bounds__(NT) void tg_scatter(TgArgs a) {
  int b, tile;
  int64_t p0, p1;
  if (!locate(a, blockIdx.x, b, tile, p0, p1)) return;
  const int64_t li = (int64_t)tile * NT + threadIdx.x;
  if (li >= p1 - p0) return;
  const int64_t gi = p0 + li;
  const float ratio = a.ratio[gi];
  if (!(ratio >= KEEP_RATIO)) return;
  const int64_t o = (int64_t)a.tbase[blockIdx.x] + a.rank[gi];
  if (o >= a.total) return;  // unreachable with consistent offsets
  const float x = a.pts[2 * gi];
  const bool flip = a.flips[(int64_t)b * a.flip_stride] != 0.f;
  a.out_pts[2 * o] = flip ? a.w - x : x;
  a.out_pts[2 * o + 1] = a.pts[2 * gi + 1];
  a.out_tg[o] = ratio;
}

// y[b][i][j] = scale * sum of the s x s window: rows summed left to right, then top to bottom
__global__ __launch_bounds__(NT) void sum_pool1_fwd_k(const float* __restrict__ x, int64_t nout, int Ho, int Wo,
                                                      int s, float scale, float* __restrict__ y) {
  const int64_t o = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (o >= nout) return;
  const int j = (int)(o % Wo);
  const int64_t r = o / Wo;
  const int i = (int)(r % Ho);
  const int64_t b = r / Ho;
  const int64_t W = (int64_t)Wo * s;
  const float* p = x + (b * Ho * s + (int64_t)i * s) * W + (int64_t)j * s;
  float acc = 0.f;
  for (int u = 0; u < s; ++u) {
    float row = 0.f;
    for (int v = 0; v < s; ++v) row += p[u * W + v];
    acc += row;
  }
  y[o] = scale * acc;
}

__global__ __launch_bounds__(NT) void sum_pool1_bwd_k(const float* __restrict__ gy, int64_t nin, int H, int W,
                                                      int s, float scale, float* __restrict__ gx) {
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (e >= nin) return;
  const int j = (int)(e % W);
  const int64_t r = e / W;
  const int i = (int)(r % H);
  const int64_t b = r / H;
  gx[e] = scale * gy[(b * (H / s) + i / s) * (W / s) + j / s];
}

int64_t max_tiles(int B, int64_t total) { return (total + NT - 1) / NT + B; }

}  // namespace

extern "C" int64_t dg_bl_targets_workspace(int B, int64_t total_points) {
  if (B <= 0 || total_points < 0) return DG_ERR_INVALID;
  if (total_points >= (1ll << 31) - NT) return DG_ERR_UNSUPPORTED;
  const int64_t words = 2 * total_points + 2 * max_tiles(B, total_points) + 1;
  return (words * 4 + 255) / 256 * 256;
}

extern "C" int dg_bl_targets(const float* points, const int64_t* offsets, int64_t total_points, int B, int h, int w,
                             const float* flips, int flip_stride, float* out_points, float* out_targets,
                             int64_t* out_offsets, float* dist_out, float* ratio_out, void* workspace,
                             void* stream) {
  DG_REQUIRE(offsets && flips && out_offsets && workspace && B > 0 && h > 0 && w > 0 && flip_stride > 0);
  DG_REQUIRE(total_points >= 0);
  DG_REQUIRE(total_points == 0 || (points && out_points && out_targets));
  DG_SUPPORTED(total_points < (1ll << 31) - NT);
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = max_tiles(B, total_points);
  TgArgs a;
  a.pts = points; a.offs = offsets; a.total = total_points; a.B = B; a.max_tiles = (int)tiles;
  a.h = (float)h; a.w = (float)w;
  a.flips = flips; a.flip_stride = flip_stride;
  a.ratio = (float*)workspace;
  a.rank = (int*)workspace + total_points;
  a.tcnt = a.rank + total_points;
  a.tbase = a.tcnt + tiles;
  a.out_pts = out_points; a.out_tg = out_targets; a.out_offs = out_offsets;
  a.dist_out = dist_out; a.ratio_out = ratio_out;
  if (total_points > 0) {
    hipLaunchKernelGGL(tg_points, dim3((unsigned)tiles), dim3(NT), 0, st, a);
    DG_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(tg_scan, dim3(1), dim3(NT), 0, st, a);
  DG_CHECK_LAUNCH();
  if (total_points > 0) {
    hipLaunchKernelGGL(tg_scatter, dim3((unsigned)tiles), dim3(NT), 0, st, a);
    DG_CHECK_LAUNCH();
  }
  return DG_OK;
}

extern "C" int dg_sum_pool1_fwd(const float* x, int B, int H, int W, int s, float scale, float* y, void* stream) {
  DG_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && s > 0);
  DG_SUPPORTED(H % s == 0 && W % s == 0);
  const int64_t nout = (int64_t)B * (H / s) * (W / s);
  DG_SUPPORTED((nout + NT - 1) / NT < (1ll << 31));
  hipLaunchKernelGGL(sum_pool1_fwd_k, dim3((unsigned)((nout + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, x,
                     nout, H / s, W / s, s, scale, y);
  DG_CHECK_LAUNCH();
  return DG_OK;
}

extern "C" int dg_sum_pool1_bwd(const float* gy, int B, int H, int W, int s, float scale, float* gx, void* stream) {
  DG_REQUIRE(gy && gx && B > 0 && H > 0 && W > 0 && s > 0);
  DG_SUPPORTED(H % s == 0 && W % s == 0);
  const int64_t nin = (int64_t)B * H * W;
  DG_SUPPORTED((nin + NT - 1) / NT < (1ll << 31));
  hipLaunchKernelGGL(sum_pool1_bwd_k, dim3((unsigned)((nin + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, gy,
                     nin, H, W, s, scale, gx);
  DG_CHECK_LAUNCH();
  return DG_OK;
}
