// Learned perceptual distance on the device: the tail of LPIPS v0.1 (Zhang, Isola, Efros, Shechtman and Wang 2018) per tapped layer,
// and the 2 x 2 max pool its VGG16 trunk needs beside tgsr_gconv.
//   per tap   f0, f1 [B][C][HW] (post-ReLU features of the two images), w[C] >= 0:
//             n(f) = f / (sqrt(sum_c f^2) + 1e-10),  d[b] = mean_p sum_c w[c] (n(f0) - n(f1))^2
//   expanded  with S0 = sum f0^2, S1 = sum f1^2, A = sum w f0^2, X = sum w f0 f1, Cc = sum w f1^2 and N = sqrt(S) + 1e-10 a pixel's term is
//             A / N0^2 - 2 X / (N0 N1) + Cc / N1^2: five channel sums, so every feature is read ONCE.  The three terms cancel where the
//             images are close (f1 = f0 + 1e-3 noise: to one part in 1e6), which float32 sums do not survive; here the floats are
//             widened exactly, their products f0^2, f0 f1, f1^2 are exact in fp64 (48 bits), and the sums run in fp64 - what is left
//             is 1e-16 C against the cancellation.  The fp64 pipe is not the limit: eight fp64 operations per pair of loaded floats.
//   gradient  d(d)/d(f0[c]) = (2 / HW) (w[c] (f0[c] / N0 - f1[c] / N1) / N0 - f0[c] T / (N0 sqrt(S0))),  T = A / N0^2 - X / (N0 N1);
//             0 at a pixel whose S0 is 0 (autograd's sqrt'(0) gives NaN there: the declared deviation).  Elementwise part in fp64 too.
// Launch shape: a workgroup of 256 threads walks tiles of TP pixels of one image; lanes run along pixels (coalesced rows of a channel
// plane), and the 64 / TP lane groups of each of the four waves take the channels c = group, group + 4 * 64 / TP, ...  TP = 64 for the wide
// early maps, 16 where HW <= 1024 (256 pixels x 512 channels at the deep taps would otherwise be 4 workgroups per image: with TP = 16
// they are 16, each splitting the channels 16 ways).  From HW = 32768 on the FORWARD splits nothing: a wave takes all channels of 64
// pixels (lpips_layer_fwd_wide_kernel), slots of four tiles at least.  The lane groups of a wave meet by an xor butterfly, the waves in
// LDS in wave order, the pixels of a tile by a shuffle tree and the tiles of a slot in tile order: no atomics, the same bits on every run.
// Every pointer needs 4 bytes only: all accesses are dwords (partial, per_layer's source: 8 bytes, they are doubles).
#include "tgsr_common.h"

namespace tgsr {

constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / 64;
constexpr int kLpMaxSlots = 512;                // slots (workgroups) per image and tap
constexpr int kLpSmallHW = 1024;                // up to here tiles of 16 pixels
constexpr int kLpWideHW = 32768;                // from here the forward does not split channels over lanes and waves
constexpr double kLpEps = 1e-10;
constexpr int kLpMaxTaps = 8;

struct LpPlan {
  int tp;                                       // pixels per tile
  int ntiles, tps, nslots;                      // tiles of an image, tiles per slot, slots
  bool wide;                                    // the forward takes whole tiles per wave (lpips_layer_fwd_wide_kernel)
};

static LpPlan lp_plan(int C, int HW, bool fwd = true) {
  LpPlan p{0, 0, 0, 0, false};
  if (C < 1 || HW < 1) return p;
  p.tp = HW <= kLpSmallHW ? 16 : 64;
  p.wide = fwd && HW >= kLpWideHW;          // (the backward keeps the split form and its own, finer grid: it writes no slots)
  p.ntiles = (HW + p.tp - 1) / p.tp;
  p.tps = (p.ntiles + kLpMaxSlots - 1) / kLpMaxSlots;
  if (p.wide && p.tps < kLpWaves) p.tps = kLpWaves;          // a tile per wave at least
  p.nslots = (p.ntiles + p.tps - 1) / p.tps;
  return p;
}

static int lp_grid(int64_t total, int cap = 8192) {
  const int64_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

static bool lp_aligned4(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr,
                        const void* f = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d) |
           reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(f)) & 3) == 0;
}

// The channel sums of this thread's pixel (p, valid where ok) over its channels: v[0..NS) = S0, S1, A, X (, Cc), then combined over the
// lane groups of the wave and over the waves; afterwards lanes [0, TP) of wave 0 hold the pixel's sums.  red: [kLpWaves][NS][TP].
template <int TP, int NS>
__device__ __forceinline__ void lp_pixel_sums(const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ w, int C,
                                              int64_t HW, int64_t p, bool ok, double (&v)[NS], double* __restrict__ red) {
  constexpr int NCG = kLpWaves * (64 / TP);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cg = wave * (64 / TP) + lane / TP;
#pragma unroll
  for (int k = 0; k < NS; ++k) v[k] = 0.0;
  if (ok) {
#pragma unroll 4
    for (int c = cg; c < C; c += NCG) {
      const double x0 = (double)p0[(int64_t)c * HW + p], x1 = (double)p1[(int64_t)c * HW + p], wc = (double)w[c];
      const double q0 = x0 * x0, q1 = x1 * x1, qx = x0 * x1;            // exact
      v[0] += q0;
      v[1] += q1;
      v[2] = fma(wc, q0, v[2]);
      v[3] = fma(wc, qx, v[3]);
      if (NS > 4) v[4] = fma(wc, q1, v[4]);
    }
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
#pragma unroll
    for (int o = TP; o < 64; o <<= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (lane < TP) red[(wave * NS + k) * TP + lane] = v[k];
  }
  __syncthreads();
  if (wave == 0 && lane < TP) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      double s = red[k * TP + lane];
#pragma unroll
      for (int u = 1; u < kLpWaves; ++u) s += red[(u * NS + k) * TP + lane];
      v[k] = s;
    }
  }
}

// A pixel's term from its five sums.  Not contracted into fused multiply-adds and in this order, so that identical features (A = X =
// Cc, N0 = N1) give t - 2 t + t = 0 exactly; a rounding residue below zero (the term is a sum of squares) is clamped.
__device__ __forceinline__ double lp_pixel_term(const double (&v)[5]) {
#pragma clang fp contract(off)
  const double i0 = 1.0 / (sqrt(v[0]) + kLpEps), i1 = 1.0 / (sqrt(v[1]) + kLpEps);
  const double t0 = v[2] * i0 * i0, tx = 2.0 * v[3] * i0 * i1, t1 = v[4] * i1 * i1;
  const double d = (t0 - tx) + t1;
  return d > 0.0 ? d : 0.0;
}

template <int TP>
__global__ __launch_bounds__(kLpThreads) void lpips_layer_fwd_kernel(const float* __restrict__ f0, int64_t bs0, const float* __restrict__ f1,
                                                                     int64_t bs1, const float* __restrict__ w, int C, int64_t HW,
                                                                     int ntiles, int tps, double* __restrict__ partial, int nslots) {
  __shared__ double red[kLpWaves * 5 * TP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, slot = blockIdx.x;
  const float* p0 = f0 + (int64_t)b * bs0;
  const float* p1 = f1 + (int64_t)b * bs1;
  const int t_end = min(ntiles, (slot + 1) * tps);
  double acc = 0.0;
  for (int t = slot * tps; t < t_end; ++t) {
    const int64_t p = (int64_t)t * TP + lane % TP;
    const bool ok = p < HW;
    double v[5];
    lp_pixel_sums<TP, 5>(p0, p1, w, C, HW, p, ok, v, red);
    if (wave == 0 && lane < TP && ok) acc += lp_pixel_term(v);
    __syncthreads();                             // red is rewritten by the next tile
  }
  if (wave == 0) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) partial[(int64_t)b * nslots + slot] = acc;
  }
}

// The forward on the wide early maps (HW >= kLpWideHW): enough pixels to fill the card without splitting channels, so every wave takes
// whole tiles of 64 pixels - all C channels of its lane's pixel, nothing to combine per tile, no barrier inside the loop - the tiles
// t0 + wave, t0 + wave + 4, ... of the slot.  Per lane the tiles add up in tile order, then the lanes by a shuffle tree, then the four
// waves in wave order.
__global__ __launch_bounds__(kLpThreads) void lpips_layer_fwd_wide_kernel(const float* __restrict__ f0, int64_t bs0,
                                                                          const float* __restrict__ f1, int64_t bs1,
                                                                          const float* __restrict__ w, int C, int64_t HW, int ntiles,
                                                                          int tps, double* __restrict__ partial, int nslots) {
  __shared__ double wacc[kLpWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, slot = blockIdx.x;
  const float* p0 = f0 + (int64_t)b * bs0;
  const float* p1 = f1 + (int64_t)b * bs1;
  const int t_end = min(ntiles, (slot + 1) * tps);
  double acc = 0.0;
  for (int t = slot * tps + wave; t < t_end; t += kLpWaves) {
    const int64_t p = (int64_t)t * 64 + lane;
    if (p < HW) {
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
      for (int c = 0; c < C; ++c) {
        const double x0 = (double)p0[(int64_t)c * HW + p], x1 = (double)p1[(int64_t)c * HW + p], wc = (double)w[c];
        const double q0 = x0 * x0, q1 = x1 * x1, qx = x0 * x1;            // exact
        v[0] += q0;
        v[1] += q1;
        v[2] = fma(wc, q0, v[2]);
        v[3] = fma(wc, qx, v[3]);
        v[4] = fma(wc, q1, v[4]);
      }
      acc += lp_pixel_term(v);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) wacc[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(int64_t)b * nslots + slot] = ((wacc[0] + wacc[1]) + wacc[2]) + wacc[3];
}

template <int TP>
__global__ __launch_bounds__(kLpThreads) void lpips_layer_bwd_kernel(const float* __restrict__ g, const float* __restrict__ f0, int64_t bs0,
                                                                     const float* __restrict__ f1, int64_t bs1, const float* __restrict__ w,
                                                                     int C, int64_t HW, int ntiles, int tps, float* __restrict__ df0,
                                                                     int64_t dbs, int accumulate, const float* __restrict__ mask) {
  constexpr int NCG = kLpWaves * (64 / TP);
  __shared__ double red[kLpWaves * 4 * TP];
  __shared__ double coef[3 * TP];                // per pixel: 1 / N0, 1 / N1, T / (N0 sqrt(S0)); 1 / N0 = 0 marks a zero-norm pixel
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, slot = blockIdx.x;
  const int cg = wave * (64 / TP) + lane / TP, pl = lane % TP;
  const float* p0 = f0 + (int64_t)b * bs0;
  const float* p1 = f1 + (int64_t)b * bs1;
  float* dp = df0 + (int64_t)b * dbs;
  const float* mp = mask ? mask + (int64_t)b * dbs : nullptr;
  const double G = 2.0 * (double)g[b] / (double)HW;
  const int t_end = min(ntiles, (slot + 1) * tps);
  for (int t = slot * tps; t < t_end; ++t) {
    const int64_t p = (int64_t)t * TP + pl;
    const bool ok = p < HW;
    double v[4];
    lp_pixel_sums<TP, 4>(p0, p1, w, C, HW, p, ok, v, red);
    if (wave == 0 && lane < TP) {
      double i0 = 0.0, i1 = 0.0, tq = 0.0;
      if (ok && v[0] > 0.0) {
        const double r0 = sqrt(v[0]);
        i0 = 1.0 / (r0 + kLpEps);
        i1 = 1.0 / (sqrt(v[1]) + kLpEps);
        tq = (v[2] * i0 * i0 - v[3] * i0 * i1) * i0 / r0;
      }
      coef[pl] = i0;
      coef[TP + pl] = i1;
      coef[2 * TP + pl] = tq;
    }
    __syncthreads();
    if (ok) {
      const double i0 = coef[pl], i1 = coef[TP + pl], tq = coef[2 * TP + pl];
#pragma unroll 4
      for (int c = cg; c < C; c += NCG) {
        const int64_t e = (int64_t)c * HW + p;
        float r = 0.f;
        if (i0 != 0.0) {
          const double x0 = (double)p0[e], x1 = (double)p1[e];
          r = (float)(G * ((double)w[c] * (x0 * i0 - x1 * i1) * i0 - x0 * tq));
        }
        if (mp && !(mp[e] > 0.f)) r = 0.f;
        dp[e] = accumulate ? dp[e] + r : r;
      }
    }
    __syncthreads();                             // red and coef are rewritten by the next tile
  }
}

struct LpFinish {
  const double* partial[kLpMaxTaps];
  int nslots[kLpMaxTaps];
  int hw[kLpMaxTaps];
};

// per_layer[l][b] = (sum of the tap's slots in index order) / HW_l, total[b] = their sum in tap order.  One workgroup per image: all
// threads bring the image's slots of every tap into LDS (up to 8 x 512 doubles), thread l adds tap l's in index order from there (a
// dependent chain of loads from HBM by one thread per image took 150 us for five taps), thread 0 the taps.
__global__ __launch_bounds__(256) void lpips_finish_kernel(LpFinish a, int L, int B, float* __restrict__ per_layer,
                                                            float* __restrict__ total) {
  __shared__ double slots[kLpMaxTaps * kLpMaxSlots];
  __shared__ double sums[kLpMaxTaps];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int l = 0; l < L; ++l) {
    const double* p = a.partial[l] + (int64_t)b * a.nslots[l];
    for (int k = tid; k < a.nslots[l]; k += 256) slots[l * kLpMaxSlots + k] = p[k];
  }
  __syncthreads();
  if (tid < L) {
    const double* p = slots + tid * kLpMaxSlots;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < a.nslots[tid]; ++k) s += p[k];
    s /= (double)a.hw[tid];
    sums[tid] = s;
    if (per_layer) per_layer[(int64_t)tid * B + b] = (float)s;
  }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int l = 0; l < L; ++l) tot += sums[l];
    total[b] = (float)tot;
  }
}

// x [B][C][H][W] (samples x_bstride apart) -> out based at a channel slice: F.max_pool2d(x, 2), floor
__global__ __launch_bounds__(256) void maxpool2s2_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W, int OH,
                                                         int OW, int64_t x_bstride, int64_t o_bstride, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ox = (int)(e % OW), oy = (int)((e / OW) % OH), c = (int)((e / ((int64_t)OW * OH)) % C), b = (int)(e / ((int64_t)OW * OH * C));
    const float* p = x + (int64_t)b * x_bstride + ((int64_t)c * H + 2 * oy) * W + 2 * ox;
    float m = p[0];
    m = p[1] > m ? p[1] : m;
    m = p[W] > m ? p[W] : m;
    m = p[W + 1] > m ? p[W + 1] : m;
    out[(int64_t)b * o_bstride + ((int64_t)c * OH + oy) * OW + ox] = m;
  }
}

// its backward in gather form: the windows do not overlap, so input pixel (iy, ix) belongs to one window (none in an odd trailing row or
// column: 0) and takes that window's dy where it is the FIRST maximum (row-major scan, strict >: torch's rule).  dx (+)= ...
__global__ __launch_bounds__(256) void maxpool2s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ dx, int C, int H, int W, int OH, int OW,
                                                             int64_t x_bstride, int64_t dy_bstride, int64_t dx_bstride, int64_t total,
                                                             int accumulate, const float* __restrict__ mask) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ix = (int)(e % W), iy = (int)((e / W) % H), c = (int)((e / ((int64_t)W * H)) % C), b = (int)(e / ((int64_t)W * H * C));
    const int oy = iy >> 1, ox = ix >> 1;
    float gv = 0.f;
    if (oy < OH && ox < OW) {
      const float* p = x + (int64_t)b * x_bstride + ((int64_t)c * H + 2 * oy) * W + 2 * ox;
      float m = p[0];
      int arg = 0;
      if (p[1] > m) { m = p[1]; arg = 1; }
      if (p[W] > m) { m = p[W]; arg = 2; }
      if (p[W + 1] > m) { m = p[W + 1]; arg = 3; }
      if (arg == ((iy & 1) << 1 | (ix & 1))) gv = dy[(int64_t)b * dy_bstride + ((int64_t)c * OH + oy) * OW + ox];
    }
    const int64_t oo = (int64_t)b * dx_bstride + ((int64_t)c * H + iy) * W + ix;
    if (mask && !(mask[oo] > 0.f)) gv = 0.f;
    float* o = dx + oo;
    *o = accumulate ? *o + gv : gv;
  }
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int tgsr_maxpool2s2_fwd(const float* x, int64_t x_bstride, int B, int C, int H, int W, float* out, int64_t o_bstride,
                                   void* stream) {
  if (!x || !out || B < 1 || C < 1 || H < 2 || W < 2) return TGSR_EINVAL;
  if (!lp_aligned4(x, out)) return TGSR_EUNSUPPORTED;
  const int OH = H / 2, OW = W / 2;
  const int64_t total = (int64_t)B * C * OH * OW;
  hipLaunchKernelGGL(maxpool2s2_kernel, dim3(lp_grid(total)), dim3(256), 0, as_stream(stream), x, out, C, H, W, OH, OW, x_bstride, o_bstride,
                     total);
  return note_launch(hipGetLastError(), "maxpool2s2_kernel");
}

extern "C" int tgsr_maxpool2s2_bwd(const float* x, int64_t x_bstride, const float* dy, int64_t dy_bstride, int B, int C, int H, int W,
                                   float* dx, int64_t dx_bstride, int accumulate, const float* mask, void* stream) {
  if (!x || !dy || !dx || B < 1 || C < 1 || H < 2 || W < 2) return TGSR_EINVAL;
  if (!lp_aligned4(x, dy, dx, mask)) return TGSR_EUNSUPPORTED;
  const int OH = H / 2, OW = W / 2;
  const int64_t total = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(maxpool2s2_bwd_kernel, dim3(lp_grid(total)), dim3(256), 0, as_stream(stream), x, dy, dx, C, H, W, OH, OW, x_bstride,
                     dy_bstride, dx_bstride, total, accumulate, mask);
  return note_launch(hipGetLastError(), "maxpool2s2_bwd_kernel");
}

extern "C" int tgsr_lpips_nslots(int C, int HW) { return lp_plan(C, HW).nslots; }

extern "C" int tgsr_lpips_layer_fwd(const float* f0, int64_t f0_bstride, const float* f1, int64_t f1_bstride, const float* w, int B, int C,
                                    int HW, double* partial, void* stream) {
  const LpPlan p = lp_plan(C, HW);
  if (!f0 || !f1 || !w || !partial || B < 1 || B > 65535 || p.nslots < 1) return TGSR_EINVAL;
  if (!lp_aligned4(f0, f1, w) || (reinterpret_cast<uintptr_t>(partial) & 7)) return TGSR_EUNSUPPORTED;
  const dim3 grid(p.nslots, B);
  if (p.wide)
    hipLaunchKernelGGL(lpips_layer_fwd_wide_kernel, grid, dim3(kLpThreads), 0, as_stream(stream), f0, f0_bstride, f1, f1_bstride, w, C,
                       (int64_t)HW, p.ntiles, p.tps, partial, p.nslots);
  else if (p.tp == 16)
    hipLaunchKernelGGL(lpips_layer_fwd_kernel<16>, grid, dim3(kLpThreads), 0, as_stream(stream), f0, f0_bstride, f1, f1_bstride, w, C,
                       (int64_t)HW, p.ntiles, p.tps, partial, p.nslots);
  else
    hipLaunchKernelGGL(lpips_layer_fwd_kernel<64>, grid, dim3(kLpThreads), 0, as_stream(stream), f0, f0_bstride, f1, f1_bstride, w, C,
                       (int64_t)HW, p.ntiles, p.tps, partial, p.nslots);
  return note_launch(hipGetLastError(), "lpips_layer_fwd_kernel");
}

extern "C" int tgsr_lpips_finish(const double* const* partial, const int* nslots, const int* HW, int L, int B, float* per_layer,
                                 float* total, void* stream) {
  if (!partial || !nslots || !HW || !total || L < 1 || L > kLpMaxTaps || B < 1) return TGSR_EINVAL;
  LpFinish a;
  for (int l = 0; l < L; ++l) {
    if (!partial[l] || nslots[l] < 1 || nslots[l] > kLpMaxSlots || HW[l] < 1) return TGSR_EINVAL;
    if (reinterpret_cast<uintptr_t>(partial[l]) & 7) return TGSR_EUNSUPPORTED;
    a.partial[l] = partial[l];
    a.nslots[l] = nslots[l];
    a.hw[l] = HW[l];
  }
  for (int l = L; l < kLpMaxTaps; ++l) {
    a.partial[l] = nullptr;
    a.nslots[l] = a.hw[l] = 0;
  }
  if (!lp_aligned4(per_layer, total)) return TGSR_EUNSUPPORTED;
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(B), dim3(256), 0, as_stream(stream), a, L, B, per_layer, total);
  return note_launch(hipGetLastError(), "lpips_finish_kernel");
}

extern "C" int tgsr_lpips_layer_bwd(const float* g, const float* f0, int64_t f0_bstride, const float* f1, int64_t f1_bstride, const float* w,
                                    int B, int C, int HW, float* df0, int64_t df0_bstride, int accumulate, const float* mask,
                                    void* stream) {
  const LpPlan p = lp_plan(C, HW, false);
  if (!g || !f0 || !f1 || !w || !df0 || B < 1 || B > 65535 || p.nslots < 1) return TGSR_EINVAL;
  if (!lp_aligned4(g, f0, f1, w, df0, mask)) return TGSR_EUNSUPPORTED;
  const dim3 grid(p.nslots, B);
  if (p.tp == 16)
    hipLaunchKernelGGL(lpips_layer_bwd_kernel<16>, grid, dim3(kLpThreads), 0, as_stream(stream), g, f0, f0_bstride, f1, f1_bstride, w, C,
                       (int64_t)HW, p.ntiles, p.tps, df0, df0_bstride, accumulate, mask);
  else
    hipLaunchKernelGGL(lpips_layer_bwd_kernel<64>, grid, dim3(kLpThreads), 0, as_stream(stream), g, f0, f0_bstride, f1, f1_bstride, w, C,
                       (int64_t)HW, p.ntiles, p.tps, df0, df0_bstride, accumulate, mask);
  return note_launch(hipGetLastError(), "lpips_layer_bwd_kernel");
}
