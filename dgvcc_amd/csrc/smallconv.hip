// Small-channel k x k convolution: stride 1, "same" padding, R == S in {1,3,5,7,9},
// 1 <= C, Cout <= 64, NHWC activations whose channel count is rounded up to a multiple of 8 (Cp) with
// exact zeros in the padded lanes.  f32 / bf16 / f16; the 16-bit types run v_mfma_f32_16x16x32, f32 the
// exact v_mfma_f32_16x16x4_f32 (in every dg_set_f32_math mode), both with f32 accumulation.
//
//  forward / input gradient   one implicit GEMM over an LDS-staged halo tile: M = output channel (the
//      packed filter, read from global memory: <= 50 KB for the MCNN layers, L1/L2 resident), N = 16
//      pixels of a tile row, K ordered (tap row, tap column, channel) inside a stage of <= 32 input
//      channels, so one lane's K run (8 16-bit / 4 f32 consecutive channels at one tap) is one 16-byte LDS
//      read.  The accumulator then holds 4 consecutive output channels of one pixel per lane: 8 / 16-byte
//      stores.  The input gradient is the same kernel on the filter packed flipped and transposed.
//  weight / bias gradient     M = output channel (dy), N = (tap, channel) (+ one column of ones: the bias
//      gradient), K = pixels.  A block walks pixel tiles with a fixed stride and keeps its partial dW in
//      registers; it writes one slab, and a second launch sums the slabs in block order: no atomics,
//      bit-identical from run to run.
#include "dg_common.h"
#include <algorithm>

namespace {

constexpr int NTH = 256;            // 4 waves
constexpr int TW = 32;              // tile width in pixels (two 16-pixel MFMA column groups)
constexpr int CS = 32;              // input channels per LDS stage
constexpr int LDS_BUDGET = 64 * 1024;
constexpr int WG_NW = 8;            // weight gradient: (tap, channel) tiles per wave
constexpr int WG_MAX_SLABS = 512;

__host__ __device__ inline int rup(int a, int b) { return (a + b - 1) / b * b; }

template <typename T> __device__ __forceinline__ f4v mma(const u4v& a, const u4v& b, f4v c) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[j]), c, 0, 0, 0);
    return c;
  } else {
    return mfma16x16x32<T>(__builtin_bit_cast(s8v, a), __builtin_bit_cast(s8v, b), c);
  }
}

// ------------------------------------------------------------------ filter packing --
// wp[stage][o < Cop16][k < Kst], k = (r*R + s)*ck + c, stage = 32 input channels; ck = the stage's real
// channels rounded up to the lane's K run V (8 16-bit: the padded count; 4 f32: a Cin = 3 layer packs 4
// channels per tap, not 8), Kst = R*R*ck rounded up to one MFMA step group (4 lane groups x V); zero in
// every padded entry.  flip: the input gradient's filter, wp[ci = conv o][o = conv c] = w[ci][o][R-1-r][R-1-s].
__host__ __device__ inline long long pack_elems(int Co, int Ci, int R, int V) {
  const int Cip = rup(Ci, 8), nst = (Cip + CS - 1) / CS, cwl = rup(Ci - CS * (nst - 1), V);
  return (long long)rup(Co, 16) * ((long long)(nst - 1) * rup(R * R * CS, 4 * V) + rup(R * R * cwl, 4 * V));
}

template <typename T>
__global__ __launch_bounds__(NTH) void pack_kernel(const float* __restrict__ w, int Csrc, int R, int flip, int Co, int Ci,
                                                   T* __restrict__ wp, long long total) {
  constexpr int V = 16 / (int)sizeof(T);
  const int Cip = rup(Ci, 8), nst = (Cip + CS - 1) / CS, Cop16 = rup(Co, 16);
  const long long stsz = (long long)Cop16 * rup(R * R * CS, 4 * V);
  for (long long i = (long long)blockIdx.x * NTH + threadIdx.x; i < total; i += (long long)gridDim.x * NTH) {
    const long long sq = i / stsz;
    const int st = sq < nst - 1 ? (int)sq : nst - 1;
    const int rem = (int)(i - st * stsz);
    const int ck = rup(min(CS, Ci - CS * st), V), Kst = rup(R * R * ck, 4 * V);
    const int o = rem / Kst, k = rem - o * Kst;
    const int tap = k / ck, ci = st * CS + (k - tap * ck);
    float v = 0.f;
    if (tap < R * R && o < Co && ci < Ci) {
      const int r = tap / R, s = tap - r * R;
      v = flip ? w[(((long long)ci * Csrc + o) * R + (R - 1 - r)) * R + (R - 1 - s)]
               : w[(((long long)o * Csrc + ci) * R + r) * R + s];
    }
    wp[i] = from_f<T>(v);
  }
}

// ------------------------------------------------------------------ forward --
template <typename T, int NT>
__global__ __launch_bounds__(NTH) void fwd_kernel(const T* __restrict__ x, long long ldx, int H, int W, int Ci, int Cip,
                                                  const T* __restrict__ wp, const float* __restrict__ bias, int Co,
                                                  int R, int relu, T* __restrict__ y, long long ldy, int TH,
                                                  int tilesH, int tilesW) {
  constexpr int V = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_smem[];
  T* lds = (T*)sc_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  int b = blockIdx.x;
  const int tw = b % tilesW;
  b /= tilesW;
  const int th = b % tilesH, n = b / tilesH;
  const int h0 = th * TH, w0 = tw * TW, pad = R >> 1;
  const int LW = TW + R - 1, LH = TH + R - 1, nseg = TH * 2;
  const int Cop16 = NT * 16, Cop8 = rup(Co, 8);
  const int K32 = rup(R * R * CS, 4 * V), nst = (Cip + CS - 1) / CS;
  f4v acc[4][NT];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[j][nt] = f4v{0.f, 0.f, 0.f, 0.f};

  for (int st = 0; st < nst; ++st) {
    const int cw = min(CS, Cip - CS * st), cpt = cw / V, xs = cw + V;  // xs: LDS pixel stride (+16 B)
    if (st) __syncthreads();
    const int nchunk = LH * LW * cpt;
    for (int i = tid; i < nchunk; i += NTH) {
      const int px = i / cpt, cv = i - px * cpt;
      const int lh = px / LW, lw = px - lh * LW;
      const int h = h0 + lh - pad, w = w0 + lw - pad;
      u4v v = u4v{0u, 0u, 0u, 0u};
      if (h >= 0 && h < H && w >= 0 && w < W)
        v = *(const u4v*)(x + (((long long)n * H + h) * W + w) * ldx + st * CS + cv * V);
      *(u4v*)(lds + px * xs + cv * V) = v;
    }
    __syncthreads();
    const int cpu = (min(CS, Ci - CS * st) + V - 1) / V;  // K runs per tap that hold a real channel
    const int nch = R * R * cpu, nsteps = (nch + 3) >> 2, Kst = nsteps * 4 * V;
    const T* wst = wp + (long long)st * Cop16 * K32 + (long long)li * Kst;
    int q = g, tap = q / cpu, cv = q - tap * cpu, r = tap / R, s = tap - r * R;
    for (int t = 0; t < nsteps; ++t) {
      const bool valid = q < nch;
      u4v wf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[nt] = *(const u4v*)(wst + (long long)nt * 16 * Kst + q * V);
      const int aoff = valid ? (r * LW + s) * xs + cv * V : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int seg = wave + 4 * j;
        if (seg < nseg) {
          const int row = seg >> 1, col = (seg & 1) * 16 + li;
          u4v xf = *(const u4v*)(lds + (row * LW + col) * xs + aoff);
          if (!valid) xf = u4v{0u, 0u, 0u, 0u};
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[j][nt] = mma<T>(wf[nt], xf, acc[j][nt]);
        }
      }
      q += 4;
      cv += 4;
      while (cv >= cpu) {
        cv -= cpu;
        if (++s == R) { s = 0; ++r; }
      }
    }
  }
  // lane: output channels nt*16 + 4g .. + 3 of pixel (row, (seg & 1)*16 + li)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int seg = wave + 4 * j;
    if (seg >= nseg) continue;
    const int h = h0 + (seg >> 1), w = w0 + (seg & 1) * 16 + li;
    if (h >= H || w >= W) continue;
    T* yp = y + (((long long)n * H + h) * W + w) * ldy;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int o0 = nt * 16 + 4 * g;
      if (o0 >= Cop8) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = o0 + i;
        float a = acc[j][nt][i] + ((bias && o < Co) ? bias[o] : 0.f);
        if (relu) a = fmaxf(a, 0.f);
        v[i] = o < Co ? a : 0.f;  // the padded lanes hold exact zeros
      }
      st4(yp + o0, v);
    }
  }
}

// ------------------------------------------------------------------ weight gradient --
template <typename T, int MT>
__global__ __launch_bounds__(NTH) void wgrad_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ dy,
                                                    long long lddy, int H, int W, int C, int Cip, int Cop8, int R, int TH,
                                                    int tilesH, int tilesW, int ntiles, int ysplit,
                                                    float* __restrict__ slabs, int slabcols, int colstride) {
  constexpr int V = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int st = blockIdx.y / ysplit, sub = blockIdx.y - st * ysplit;
  const int cw = min(CS, Cip - CS * st), cpt = cw / V, xs = cw + V;
  const int cr = min(CS, C - CS * st);  // the stage's real channels: N runs over them alone
  const int Nst = R * R * cr + 1, NTst = (Nst + 15) >> 4;  // the last column: ones (bias gradient)
  const int tpb = (NTst + ysplit - 1) / ysplit, tile0 = sub * tpb, tend = min(NTst, tile0 + tpb);
  const int pad = R >> 1, LW = TW + R - 1, LH = TH + R - 1;
  constexpr int dys = MT * 16 + V, dcpt = MT * 16 / V;
  T* xl = (T*)sc_smem;
  T* dl = xl + LH * LW * xs;

  int toff[WG_NW];
  bool ones[WG_NW];
#pragma unroll
  for (int k = 0; k < WG_NW; ++k) {
    const int ng = (tile0 + wave + 4 * k) * 16 + li;
    ones[k] = ng == Nst - 1;
    const int tap = ng / cr, c = ng - tap * cr, r = tap / R, s = tap - r * R;
    toff[k] = ng < Nst - 1 ? (r * LW + s) * xs + c : 0;
  }
  f4v acc[WG_NW][MT];
#pragma unroll
  for (int k = 0; k < WG_NW; ++k)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[k][mt] = f4v{0.f, 0.f, 0.f, 0.f};

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int b = tile;
    const int tw = b % tilesW;
    b /= tilesW;
    const int th = b % tilesH, n = b / tilesH;
    const int h0 = th * TH, w0 = tw * TW;
    if (tile != (int)blockIdx.x) __syncthreads();
    for (int i = tid; i < LH * LW * cpt; i += NTH) {
      const int px = i / cpt, cv = i - px * cpt;
      const int lh = px / LW, lw = px - lh * LW;
      const int h = h0 + lh - pad, w = w0 + lw - pad;
      u4v v = u4v{0u, 0u, 0u, 0u};
      if (h >= 0 && h < H && w >= 0 && w < W)
        v = *(const u4v*)(x + (((long long)n * H + h) * W + w) * ldx + st * CS + cv * V);
      *(u4v*)(xl + px * xs + cv * V) = v;
    }
    for (int i = tid; i < TH * TW * dcpt; i += NTH) {
      const int px = i / dcpt, cv = i - px * dcpt;
      const int lh = px / TW, lw = px - lh * TW;
      const int h = h0 + lh, w = w0 + lw;
      u4v v = u4v{0u, 0u, 0u, 0u};
      if (h < H && w < W && cv * V < Cop8) v = *(const u4v*)(dy + (((long long)n * H + h) * W + w) * lddy + cv * V);
      *(u4v*)(dl + px * dys + cv * V) = v;
    }
    __syncthreads();
    for (int row = 0; row < TH; ++row) {
      if constexpr (sizeof(T) == 4) {
        // K = 4 pixels per MFMA: lane group g takes pixel 4j + g of the row
        for (int j = 0; j < TW / 4; ++j) {
          const int col = 4 * j + g;
          float a[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a[mt] = dl[(row * TW + col) * dys + mt * 16 + li];
          const T* xr = xl + (row * LW + col) * xs;
#pragma unroll
          for (int k = 0; k < WG_NW; ++k) {
            if (tile0 + wave + 4 * k < tend) {
              const float bv = ones[k] ? 1.f : xr[toff[k]];
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                acc[k][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], bv, acc[k][mt], 0, 0, 0);
            }
          }
        }
      } else {
        // K = the row's 32 pixels: lane group g takes pixels 8g .. 8g + 7
        const unsigned short* du = (const unsigned short*)dl + (row * TW + 8 * g) * dys + li;
        const unsigned short* xu = (const unsigned short*)xl + (row * LW + 8 * g) * xs;
        const unsigned short one = f_to_u16<T>(1.f);
        s8v a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int i = 0; i < 8; ++i) a[mt][i] = (short)du[i * dys + mt * 16];
#pragma unroll
        for (int k = 0; k < WG_NW; ++k) {
          if (tile0 + wave + 4 * k < tend) {
            s8v bv;
#pragma unroll
            for (int i = 0; i < 8; ++i) bv[i] = (short)(ones[k] ? one : xu[i * xs + toff[k]]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[k][mt] = mfma16x16x32<T>(a[mt], bv, acc[k][mt]);
          }
        }
      }
    }
  }
  float* slab = slabs + (long long)blockIdx.x * MT * 16 * slabcols + (long long)st * colstride;
#pragma unroll
  for (int k = 0; k < WG_NW; ++k) {
    const int nt = tile0 + wave + 4 * k;
    if (nt >= tend) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[(long long)(mt * 16 + 4 * g + i) * slabcols + nt * 16 + li] = acc[k][mt][i];
  }
}

// dw[o][c][r][s] (and db[o]) = the slabs' sum in block order
__global__ __launch_bounds__(NTH) void wgrad_reduce_kernel(const float* __restrict__ slabs, int nblk, long long slabsz,
                                                           int slabcols, int colstride, int Cout, int C, int R,
                                                           float* __restrict__ dw, float* __restrict__ db) {
  const int nW = Cout * C * R * R;
  const int i = blockIdx.x * NTH + threadIdx.x;
  if (i >= nW + Cout) return;
  int o, col;
  if (i < nW) {
    o = i / (C * R * R);
    const int rem = i - o * C * R * R, c = rem / (R * R), tap = rem - c * R * R;
    const int st = c / CS, cr = min(CS, C - CS * st);
    col = st * colstride + tap * cr + (c - st * CS);
  } else {
    if (!db) return;
    o = i - nW;
    col = R * R * min(CS, C);
  }
  const float* p = slabs + (long long)o * slabcols + col;
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += p[b * slabsz];
  if (i < nW) dw[i] = s; else db[o] = s;
}

// ------------------------------------------------------------------ image layout --
template <typename T>
__global__ __launch_bounds__(NTH) void image_kernel(const float* __restrict__ img, int C, long long HW, long long M, int Cp,
                                                    T* __restrict__ y, long long ldy) {
  constexpr int V = 16 / (int)sizeof(T);
  const int cpp = Cp / V;
  const long long total = M * cpp;
  for (long long i = (long long)blockIdx.x * NTH + threadIdx.x; i < total; i += (long long)gridDim.x * NTH) {
    const long long px = i / cpp;
    const int c0 = (int)(i - px * cpp) * V;
    const long long n = px / HW, hw = px - n * HW;
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = c0 + e < C ? img[(n * C + c0 + e) * HW + hw] : 0.f;
    stv(y + px * ldy + c0, v);
  }
}

// ------------------------------------------------------------------ host side --
inline bool in_family(int C, int Cout, int R, int S, int stride, int pad, int dil) {
  return R == S && (R == 1 || R == 3 || R == 5 || R == 7 || R == 9) && stride == 1 && dil == 1 && pad == (R - 1) / 2 &&
         C >= 1 && C <= 64 && Cout >= 1 && Cout <= 64;
}

inline size_t fwd_lds(int TH, int R, int cw, int es) { return (size_t)(TH + R - 1) * (TW + R - 1) * (cw * es + 16); }
inline size_t wg_lds(int TH, int R, int cw, int Cop16, int es) {
  return fwd_lds(TH, R, cw, es) + (size_t)TH * TW * (Cop16 * es + 16);
}

template <typename F> inline int pick_th(int H, F bytes) {
  int TH = 8;
  while (TH > 1 && (bytes(TH) > (size_t)LDS_BUDGET || TH / 2 >= H)) TH >>= 1;
  return TH;
}

template <typename T, int NT>
int launch_fwd(const void* x, int64_t ldx, int N, int H, int W, int Ci, int Cip, const void* wp, const float* bias, int Co, int R,
               int relu, void* y, int64_t ldy, hipStream_t st) {
  const int es = (int)sizeof(T), cw = std::min(CS, Cip);
  const int TH = pick_th(H, [&](int t) { return fwd_lds(t, R, cw, es); });
  const int tilesH = dg_cdiv(H, TH), tilesW = dg_cdiv(W, TW);
  const long long blocks = (long long)N * tilesH * tilesW;
  if (blocks >= (1ll << 31)) return DG_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((fwd_kernel<T, NT>), dim3((unsigned)blocks), dim3(NTH), fwd_lds(TH, R, cw, es), st, (const T*)x,
                     (long long)ldx, H, W, Ci, Cip, (const T*)wp, bias, Co, R, relu, (T*)y, (long long)ldy, TH, tilesH,
                     tilesW);
  DG_CHECK_LAUNCH();
  return DG_OK;
}

template <typename T>
int launch_fwd_t(int NT, const void* x, int64_t ldx, int N, int H, int W, int Ci, int Cip, const void* wp, const float* bias,
                 int Co, int R, int relu, void* y, int64_t ldy, hipStream_t st) {
  switch (NT) {
    case 1: return launch_fwd<T, 1>(x, ldx, N, H, W, Ci, Cip, wp, bias, Co, R, relu, y, ldy, st);
    case 2: return launch_fwd<T, 2>(x, ldx, N, H, W, Ci, Cip, wp, bias, Co, R, relu, y, ldy, st);
    case 3: return launch_fwd<T, 3>(x, ldx, N, H, W, Ci, Cip, wp, bias, Co, R, relu, y, ldy, st);
    default: return launch_fwd<T, 4>(x, ldx, N, H, W, Ci, Cip, wp, bias, Co, R, relu, y, ldy, st);
  }
}

// the weight gradient's launch geometry (shared by the workspace query and the launch)
struct WgPlan {
  int TH, tilesH, tilesW, ntiles, nblk, nst, ysplit, colstride, slabcols, Cop16;
  long long slabsz;
};

inline WgPlan wg_plan(int dtype, int N, int H, int W, int C, int Cout, int R) {
  WgPlan p;
  const int es = dtype == DG_F32 ? 4 : 2, Cip = rup(C, 8), cw = std::min(CS, Cip);
  p.Cop16 = rup(Cout, 16);
  p.TH = pick_th(H, [&](int t) { return wg_lds(t, R, cw, p.Cop16, es); });
  p.tilesH = dg_cdiv(H, p.TH);
  p.tilesW = dg_cdiv(W, TW);
  const long long nt = (long long)N * p.tilesH * p.tilesW;
  p.ntiles = (int)std::min<long long>(nt, (1ll << 31) - 1);
  p.nst = (Cip + CS - 1) / CS;
  const int NTmax = (R * R * std::min(CS, C) + 1 + 15) / 16;
  p.ysplit = dg_cdiv(NTmax, 4 * WG_NW);
  p.colstride = NTmax * 16;
  p.slabcols = p.nst * p.colstride;
  p.slabsz = (long long)p.Cop16 * p.slabcols;
  // slabs: enough blocks to fill the device, bounded by ~128 MB of workspace
  const long long cap = std::max<long long>(32, std::min<long long>(WG_MAX_SLABS, (128ll << 20) / (p.slabsz * 4)));
  p.nblk = (int)std::min<long long>(nt, cap);
  return p;
}

template <typename T, int MT>
int launch_wgrad(const WgPlan& p, const void* x, int64_t ldx, const void* dy, int64_t lddy, int H, int W, int C, int Cip,
                 int Cop8, int R, float* slabs, hipStream_t st) {
  const size_t lds = wg_lds(p.TH, R, std::min(CS, Cip), p.Cop16, (int)sizeof(T));
  hipLaunchKernelGGL((wgrad_kernel<T, MT>), dim3(p.nblk, p.nst * p.ysplit), dim3(NTH), lds, st, (const T*)x,
                     (long long)ldx, (const T*)dy, (long long)lddy, H, W, C, Cip, Cop8, R, p.TH, p.tilesH, p.tilesW,
                     p.ntiles, p.ysplit, slabs, p.slabcols, p.colstride);
  DG_CHECK_LAUNCH();
  return DG_OK;
}

template <typename T>
int launch_wgrad_t(const WgPlan& p, const void* x, int64_t ldx, const void* dy, int64_t lddy, int H, int W, int C,
                   int Cip, int Cop8, int R, float* slabs, hipStream_t st) {
  switch (p.Cop16 / 16) {
    case 1: return launch_wgrad<T, 1>(p, x, ldx, dy, lddy, H, W, C, Cip, Cop8, R, slabs, st);
    case 2: return launch_wgrad<T, 2>(p, x, ldx, dy, lddy, H, W, C, Cip, Cop8, R, slabs, st);
    case 3: return launch_wgrad<T, 3>(p, x, ldx, dy, lddy, H, W, C, Cip, Cop8, R, slabs, st);
    default: return launch_wgrad<T, 4>(p, x, ldx, dy, lddy, H, W, C, Cip, Cop8, R, slabs, st);
  }
}

inline bool dtype_ok(int dtype) { return dtype == DG_F32 || DG_IS16(dtype); }
inline bool act_ok(const void* p, int64_t ld, int Cp, int V) { return ld >= Cp && ld % V == 0 && (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" int64_t dg_smallconv_pack_elems(int dtype, int Cout, int C, int R, int S, int flip) {
  if (!dtype_ok(dtype)) return DG_ERR_INVALID;
  if (!in_family(C, Cout, R, S, 1, (R - 1) / 2, 1)) return DG_ERR_UNSUPPORTED;
  const int V = dtype == DG_F32 ? 4 : 8;
  return flip ? pack_elems(C, Cout, R, V) : pack_elems(Cout, C, R, V);
}

extern "C" int dg_smallconv_pack(int dtype, const float* w, int Cout, int C, int R, int S, int flip, void* wp,
                                 void* stream) {
  DG_REQUIRE(w && wp && dtype_ok(dtype));
  DG_SUPPORTED(in_family(C, Cout, R, S, 1, (R - 1) / 2, 1) && (uintptr_t)wp % 16 == 0);
  const int V = dtype == DG_F32 ? 4 : 8;
  const int Co = flip ? C : Cout, Ci = flip ? Cout : C;
  const long long total = pack_elems(Co, Ci, R, V);
  const dim3 grid((unsigned)std::min<long long>((total + NTH - 1) / NTH, 4096)), block(NTH);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DG_BF16)
    hipLaunchKernelGGL((pack_kernel<bf16>), grid, block, 0, st, w, C, R, flip, Co, Ci, (bf16*)wp, total);
  else if (dtype == DG_F16)
    hipLaunchKernelGGL((pack_kernel<f16>), grid, block, 0, st, w, C, R, flip, Co, Ci, (f16*)wp, total);
  else
    hipLaunchKernelGGL((pack_kernel<float>), grid, block, 0, st, w, C, R, flip, Co, Ci, (float*)wp, total);
  DG_CHECK_LAUNCH();
  return DG_OK;
}

extern "C" int dg_smallconv_fwd(int dtype, const void* x, int64_t ldx, int N, int H, int W, int C, const void* wp,
                                int Cout, int R, int S, int stride, int pad, int dil, const float* bias, int relu,
                                void* y, int64_t ldy, void* stream) {
  DG_REQUIRE(x && wp && y && dtype_ok(dtype) && N > 0 && H > 0 && W > 0);
  DG_SUPPORTED(in_family(C, Cout, R, S, stride, pad, dil));
  const int V = dtype == DG_F32 ? 4 : 8, Cip = rup(C, 8), Cop8 = rup(Cout, 8);
  DG_SUPPORTED(act_ok(x, ldx, Cip, V) && act_ok(y, ldy, Cop8, V) && (uintptr_t)wp % 16 == 0);
  hipStream_t st = (hipStream_t)stream;
  const int NT = rup(Cout, 16) / 16;
  return dtype == DG_BF16 ? launch_fwd_t<bf16>(NT, x, ldx, N, H, W, C, Cip, wp, bias, Cout, R, relu, y, ldy, st)
         : dtype == DG_F16 ? launch_fwd_t<f16>(NT, x, ldx, N, H, W, C, Cip, wp, bias, Cout, R, relu, y, ldy, st)
                           : launch_fwd_t<float>(NT, x, ldx, N, H, W, C, Cip, wp, bias, Cout, R, relu, y, ldy, st);
}

extern "C" int64_t dg_smallconv_wgrad_workspace(int dtype, int N, int H, int W, int C, int Cout, int R, int S) {
  if (!dtype_ok(dtype) || N <= 0 || H <= 0 || W <= 0) return DG_ERR_INVALID;
  if (!in_family(C, Cout, R, S, 1, (R - 1) / 2, 1)) return DG_ERR_UNSUPPORTED;
  const WgPlan p = wg_plan(dtype, N, H, W, C, Cout, R);
  return (int64_t)p.nblk * p.slabsz * 4;
}

extern "C" int dg_smallconv_wgrad(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, int N, int H,
                                  int W, int C, int Cout, int R, int S, int stride, int pad, int dil, float* dw,
                                  float* dbias, void* work, int64_t work_bytes, void* stream) {
  DG_REQUIRE(x && dy && dw && work && dtype_ok(dtype) && N > 0 && H > 0 && W > 0);
  DG_SUPPORTED(in_family(C, Cout, R, S, stride, pad, dil));
  const int V = dtype == DG_F32 ? 4 : 8, Cip = rup(C, 8), Cop8 = rup(Cout, 8);
  DG_SUPPORTED(act_ok(x, ldx, Cip, V) && act_ok(dy, lddy, Cop8, V));
  const WgPlan p = wg_plan(dtype, N, H, W, C, Cout, R);
  DG_SUPPORTED((long long)N * p.tilesH * p.tilesW < (1ll << 31));
  DG_REQUIRE(work_bytes >= (int64_t)p.nblk * p.slabsz * 4 && (uintptr_t)work % 16 == 0);
  hipStream_t st = (hipStream_t)stream;
  float* slabs = (float*)work;
  const int rc = dtype == DG_BF16 ? launch_wgrad_t<bf16>(p, x, ldx, dy, lddy, H, W, C, Cip, Cop8, R, slabs, st)
                 : dtype == DG_F16 ? launch_wgrad_t<f16>(p, x, ldx, dy, lddy, H, W, C, Cip, Cop8, R, slabs, st)
                                   : launch_wgrad_t<float>(p, x, ldx, dy, lddy, H, W, C, Cip, Cop8, R, slabs, st);
  if (rc != DG_OK) return rc;
  const int nout = Cout * C * R * R + Cout;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(dg_cdiv(nout, NTH)), dim3(NTH), 0, st, slabs, p.nblk, p.slabsz,
                     p.slabcols, p.colstride, Cout, C, R, dw, dbias);
  DG_CHECK_LAUNCH();
  return DG_OK;
}

extern "C" int dg_image_nhwc_pad(int dtype, const float* img, int N, int C, int H, int W, void* y, int64_t ldy, int Cp,
                                 void* stream) {
  DG_REQUIRE(img && y && dtype_ok(dtype) && N > 0 && C > 0 && H > 0 && W > 0);
  const int V = dtype == DG_F32 ? 4 : 8;
  DG_SUPPORTED(Cp >= C && Cp % 8 == 0 && act_ok(y, ldy, Cp, V));
  const long long HW = (long long)H * W, M = HW * N, total = M * (Cp / V);
  const dim3 grid((unsigned)std::min<long long>((total + NTH - 1) / NTH, 16384)), block(NTH);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DG_BF16)
    hipLaunchKernelGGL((image_kernel<bf16>), grid, block, 0, st, img, C, HW, M, Cp, (bf16*)y, (long long)ldy);
  else if (dtype == DG_F16)
    hipLaunchKernelGGL((image_kernel<f16>), grid, block, 0, st, img, C, HW, M, Cp, (f16*)y, (long long)ldy);
  else
    hipLaunchKernelGGL((image_kernel<float>), grid, block, 0, st, img, C, HW, M, Cp, (float*)y, (long long)ldy);
  DG_CHECK_LAUNCH();
  return DG_OK;
}
