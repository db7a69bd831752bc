// Polyphase layout passes on NHWC activations: a stride-1 3x3 convolution with dilation d and
// padding d is the dense pad-1 convolution on the d*d phase sub-images of its input,
//   xs[(n*d + i)*d + j][hp][wp][c] = x[n][hp*d + i][wp*d + j][c]   (zero outside the image),
// with Hp = ceil(H / d), Wp = ceil(W / d).  dg_space_to_batch forms the phase batch,
// dg_batch_to_space writes it back (dropping the positions outside H x W).  Each is the other's
// adjoint, so the same two kernels serve the forward and the backward.
// Pure HBM passes: one 16-byte chunk per thread, adjacent lanes on adjacent chunks of one pixel, then
// on adjacent destination pixels; the grid is sized from the destination, every destination element
// is written exactly once (no memset, no atomics).
#include "dg_common.h"
#include <algorithm>

namespace {

constexpr int NT = 256;

inline int ew_grid(long long n) {
  long long g = (n + NT - 1) / NT;
  return (int)std::max<long long>(1, std::min<long long>(g, 16384));
}

// dst (+)= src for one 16-byte chunk; src == nullptr reads as zeros.  The plain copy moves the bits
// untouched; the accumulating form adds in f32 and rounds to T once.
template <typename T>
__device__ __forceinline__ void move_chunk(const T* src, T* dst, int accumulate) {
  constexpr int V = 16 / (int)sizeof(T);
  if (!accumulate) {
    *(u4v*)dst = src ? *(const u4v*)src : u4v{0u, 0u, 0u, 0u};
    return;
  }
  if (!src) return;  // dst += 0
  float a[V], b[V];
  ldv(src, a);
  ldv(dst, b);
#pragma unroll
  for (int e = 0; e < V; ++e) b[e] += a[e];
  stv(dst, b);
}

// I: the flat index type (unsigned while the chunk count fits 31 bits: 32-bit divisions)
template <typename T, typename I>
__global__ __launch_bounds__(NT) void space_to_batch_kernel(const T* __restrict__ x, long long ldx, int N, int H, int W,
                                                            int C, int d, int Hp, int Wp, T* __restrict__ y,
                                                            long long ldy, int accumulate) {
  constexpr int V = 16 / (int)sizeof(T);
  const I tpp = (I)(C / V);
  const I total = (I)N * (I)d * (I)d * (I)Hp * (I)Wp * tpp;
  for (I i = (I)blockIdx.x * NT + threadIdx.x; i < total; i += (I)gridDim.x * NT) {
    const I px = i / tpp;  // destination pixel ((n*d + pi)*d + pj, hp, wp)
    const int ch = (int)(i - px * tpp);
    I t = px / (I)Wp;
    const int wp = (int)(px - t * (I)Wp);
    const I b = t / (I)Hp;
    const int hp = (int)(t - b * (I)Hp);
    const I bi = b / (I)d;
    const int pj = (int)(b - bi * (I)d);
    const int n = (int)(bi / (I)d);
    const int pi = (int)(bi - (I)n * (I)d);
    const int h = hp * d + pi, w = wp * d + pj;
    const T* src = (h < H && w < W) ? x + (((long long)n * H + h) * W + w) * ldx + ch * V : nullptr;
    move_chunk<T>(src, y + (long long)px * ldy + ch * V, accumulate);
  }
}

template <typename T, typename I>
__global__ __launch_bounds__(NT) void batch_to_space_kernel(const T* __restrict__ x, long long ldx, int N, int H, int W,
                                                            int C, int d, int Hp, int Wp, T* __restrict__ y,
                                                            long long ldy, int accumulate) {
  constexpr int V = 16 / (int)sizeof(T);
  const I tpp = (I)(C / V);
  const I total = (I)N * (I)H * (I)W * tpp;
  for (I i = (I)blockIdx.x * NT + threadIdx.x; i < total; i += (I)gridDim.x * NT) {
    const I px = i / tpp;  // destination pixel (n, h, w)
    const int ch = (int)(i - px * tpp);
    I t = px / (I)W;
    const int w = (int)(px - t * (I)W);
    const int n = (int)(t / (I)H);
    const int h = (int)(t - (I)n * (I)H);
    const int hp = h / d, pi = h - hp * d;  // hp < Hp and wp < Wp: always inside the phase batch
    const int wp = w / d, pj = w - wp * d;
    const long long sp = ((((long long)n * d + pi) * d + pj) * Hp + hp) * Wp + wp;
    move_chunk<T>(x + sp * ldx + ch * V, y + (long long)px * ldy + ch * V, accumulate);
  }
}

template <typename T>
int launch(bool to_batch, const void* x, int64_t ldx, int N, int H, int W, int C, int d, void* y, int64_t ldy,
           int accumulate, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  const int Hp = (H + d - 1) / d, Wp = (W + d - 1) / d;
  const long long total = (to_batch ? (long long)N * d * d * Hp * Wp : (long long)N * H * W) * (C / V);
  const bool small = total < (1ll << 31) - (long long)16384 * NT;  // the grid stride must not wrap either
  const dim3 grid(ew_grid(total)), block(NT);
  if (to_batch) {
    if (small)
      hipLaunchKernelGGL((space_to_batch_kernel<T, unsigned>), grid, block, 0, st, (const T*)x, ldx, N, H, W, C, d, Hp,
                         Wp, (T*)y, ldy, accumulate);
    else
      hipLaunchKernelGGL((space_to_batch_kernel<T, long long>), grid, block, 0, st, (const T*)x, ldx, N, H, W, C, d,
                         Hp, Wp, (T*)y, ldy, accumulate);
  } else {
    if (small)
      hipLaunchKernelGGL((batch_to_space_kernel<T, unsigned>), grid, block, 0, st, (const T*)x, ldx, N, H, W, C, d, Hp,
                         Wp, (T*)y, ldy, accumulate);
    else
      hipLaunchKernelGGL((batch_to_space_kernel<T, long long>), grid, block, 0, st, (const T*)x, ldx, N, H, W, C, d,
                         Hp, Wp, (T*)y, ldy, accumulate);
  }
  DG_CHECK_LAUNCH();
  return DG_OK;
}

int phase_entry(bool to_batch, int dtype, const void* x, int64_t ldx, int N, int H, int W, int C, int d, void* y,
                int64_t ldy, int accumulate, void* stream) {
  DG_REQUIRE(x && y && d >= 1 && N > 0 && H > 0 && W > 0 && C > 0 && ldx >= C && ldy >= C);
  DG_REQUIRE(dtype == DG_F32 || DG_IS16(dtype));
  DG_REQUIRE((long long)N * d * d < (1ll << 31) && (long long)d <= (1 << 15));
  const int V = DG_IS16(dtype) ? 8 : 4;
  DG_SUPPORTED(C % V == 0 && ldx % V == 0 && ldy % V == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0);
  hipStream_t st = (hipStream_t)stream;
  return dtype == DG_BF16 ? launch<bf16>(to_batch, x, ldx, N, H, W, C, d, y, ldy, accumulate, st)
         : dtype == DG_F16 ? launch<f16>(to_batch, x, ldx, N, H, W, C, d, y, ldy, accumulate, st)
                           : launch<float>(to_batch, x, ldx, N, H, W, C, d, y, ldy, accumulate, st);
}

}  // namespace

extern "C" int dg_space_to_batch(int dtype, const void* x, int64_t ldx, int N, int H, int W, int C, int d, void* y,
                                 int64_t ldy, int accumulate, void* stream) {
  return phase_entry(true, dtype, x, ldx, N, H, W, C, d, y, ldy, accumulate, stream);
}

extern "C" int dg_batch_to_space(int dtype, const void* x, int64_t ldx, int N, int H, int W, int C, int d, void* y,
                                 int64_t ldy, int accumulate, void* stream) {
  return phase_entry(false, dtype, x, ldx, N, H, W, C, d, y, ldy, accumulate, stream);
}
