// No-reference image quality on the device: the 36 NIQE features of every 96 x 96 block of an image (Mittal, Soundararajan and
// Bovik 2013, as MATLAB's niqe / computefeature and BasicSR's calculate_niqe compute them), everything in fp64.
//   plane     the uint8 Y plane of the image (tgsr_y_plane.h: the bytes tgsr_sr_metrics forms), `shave` border pixels removed, cropped
//             at the top-left to Hc x Wc = floor(H / 96) 96 x floor(W / 96) 96
//   window    w[k] ~ exp(-k^2 / (2 (7/6)^2)), k = -3..3, sum 1, applied along the rows then along the columns with replicate borders
//   MSCN      mu = w * y, sigma = sqrt(|w * y^2 - mu^2|), m = (y - mu) / (sigma + 1)
//   scale 2   y2[i][j] = sum_t sum_u tap[t] tap[u] y[refl(2i - 3 + t)][refl(2j - 3 + u)], tap = [-3 -9 29 111 111 29 -9 -3] / 256
//             (MATLAB's antialiased bicubic at 1/2), refl symmetric (-1 -> 0, n -> n - 1).  The taps are dyadic and y is a byte: y2 is
//             an integer sum / 65536, exact in any order.  MSCN of y2 with the same window; blocks of 48 x 48 on the same block grid.
//   features  per block and scale 18: aggd(m) -> (alpha, (beta_l + beta_r) / 2), and for the shifts (0,1), (1,0), (1,1), (1,-1)
//             aggd(m roll(m, s)) -> (alpha, (beta_r - beta_l) G(2/alpha) / G(1/alpha), beta_l, beta_r), the roll circular in the block
//   aggd(x)   l = sqrt(mean(x[x<0]^2)), r = sqrt(mean(x[x>0]^2)), g = l / r, rhat = mean|x|^2 / mean(x^2),
//             rn = rhat (g^3 + 1)(g + 1) / (g^2 + 1)^2, alpha = gam[argmin_k (r_gam[k] - rn)^2] (lowest index on a tie; a NaN rn gives
//             index 0, as np.argmin does), beta_l = l sqrt(G(1/alpha) / G(3/alpha)), beta_r likewise.  Empty sides and mean(x^2) = 0
//             give NaN by IEEE arithmetic; nothing traps.
// niqe_block_kernel: one workgroup of 384 threads per (image, block, scale).  It stages the block's Y bytes with their halo in LDS (scale
// 1: 102 x 102, clamped to the crop; scale 2: 114 x 114, reflected, from which the 54 x 54 values of y2 are formed), filters with one
// thread per column and a strip of rows (the seven row-filtered values of y and y^2 slide through registers), keeps the block's MSCN in
// LDS as fp64 [N][N] (73 728 B at N = 96; a wave reads 64 consecutive doubles of a row: every ds_read_b64 half-wave covers the 64 banks
// once), reads the four circular neighbours from there and reduces the six moments of the five maps - sum_{x<0} x^2, #{x<0},
// sum_{x>0} x^2, #{x>0}, sum|x|, sum x^2 - and the sum of sigma: per thread in element order, per wave by a shuffle tree, over the six
// waves in wave order.  niqe_fit_kernel does the ten fits of a block (table search, tgamma) and writes features and sharpness.
// No atomics, every reduction in an order the shapes fix: the same bits on every run, on any stream, inside a captured graph.
#include "tgsr_common.h"
#include "tgsr_y_plane.h"

namespace tgsr {

constexpr int kNB = 96;                       // block edge at scale 1 (48 at scale 2)
constexpr int kNR = 3;                        // window radius
constexpr int kNW = 2 * kNR + 1;              // window edge
constexpr int kNT = 384;                      // threads of a block workgroup: 96 columns x 4 strips, 48 columns x 8 strips
constexpr int kNWaves = kNT / 64;
constexpr int kNMom = 32;                     // doubles per (image, block, scale) in the workspace: 5 maps x 6 moments, sum sigma, pad
constexpr int kNS2 = kNB / 2 + 2 * kNR;       // 54: y2 values of a scale-2 block with its halo
constexpr int kNY2 = 2 * kNS2 + 6;            // 114: Y bytes under them (8 taps at stride 2)
constexpr int kNY1 = kNB + 2 * kNR;           // 102: Y bytes of a scale-1 block with its halo
constexpr size_t kNiqeLds = sizeof(double) * (kNB * kNB + kNS2 * kNS2 + kNWaves * kNMom) + 13056;   // 13056 >= 114^2, a multiple of 64

struct NiqeTaps {
  double w[kNW];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int refl(int v, int n) { return v < 0 ? -v - 1 : (v >= n ? 2 * n - 1 - v : v); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// One (image, block, scale): N the block edge, Src the staged plane (bytes at scale 1, y2 in fp64 at scale 2) with pitch SP.
template <int N, int SP, typename Src>
__device__ __forceinline__ void niqe_mscn_and_moments(const Src* __restrict__ src, double* __restrict__ m, double* __restrict__ wred,
                                                      const NiqeTaps& taps, double* __restrict__ out) {
  constexpr int kStrips = kNT / N, kRows = N / kStrips;
  const int tid = threadIdx.x, col = tid % N, strip = tid / N, r0 = strip * kRows;
  // MSCN of the strip's rows of this column: h1 / h2 hold the row-filtered y and y^2 of the seven rows under the window
  double h1[kNW] = {0, 0, 0, 0, 0, 0, 0}, h2[kNW] = {0, 0, 0, 0, 0, 0, 0}, ssig = 0;
#pragma unroll 1
  for (int r = 0; r < kRows + 2 * kNR; ++r) {
#pragma unroll
    for (int k = 0; k < kNW - 1; ++k) {
      h1[k] = h1[k + 1];
      h2[k] = h2[k + 1];
    }
    const Src* row = src + (r0 + r) * SP + col;
    double a1 = 0, a2 = 0;
#pragma unroll
    for (int k = 0; k < kNW; ++k) {
      const double v = (double)row[k];
      a1 += taps.w[k] * v;
      a2 += taps.w[k] * (v * v);
    }
    h1[kNW - 1] = a1;
    h2[kNW - 1] = a2;
    if (r >= 2 * kNR) {
      double mu = 0, e2 = 0;
#pragma unroll
      for (int k = 0; k < kNW; ++k) {
        mu += taps.w[k] * h1[k];
        e2 += taps.w[k] * h2[k];
      }
      const double sigma = sqrt(fabs(e2 - mu * mu));
      const int y = r0 + r - 2 * kNR;
      m[y * N + col] = ((double)src[(y + kNR) * SP + col + kNR] - mu) / (sigma + 1.0);
      ssig += sigma;
    }
  }
  __syncthreads();

  // the six moments of the five maps over this thread's elements, in element order
  double sneg[5], spos[5], sabs[5], ssq[5], cneg[5], cpos[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) sneg[q] = spos[q] = sabs[q] = ssq[q] = cneg[q] = cpos[q] = 0;
#pragma unroll 1
  for (int e = tid; e < N * N; e += kNT) {
    const int y = e / N, x = e - y * N;
    const int yu = y == 0 ? N - 1 : y - 1, xl = x == 0 ? N - 1 : x - 1, xr = x == N - 1 ? 0 : x + 1;
    const double c = m[e];
    const double v[5] = {c, c * m[y * N + xl], c * m[yu * N + x], c * m[yu * N + xl], c * m[yu * N + xr]};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const double x2 = v[q] * v[q];
      if (v[q] < 0) {
        sneg[q] += x2;
        cneg[q] += 1.0;
      }
      if (v[q] > 0) {
        spos[q] += x2;
        cpos[q] += 1.0;
      }
      sabs[q] += fabs(v[q]);
      ssq[q] += x2;
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  double* wr = wred + wave * kNMom;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const double t0 = wave_sum(sneg[q]), t1 = wave_sum(cneg[q]), t2 = wave_sum(spos[q]), t3 = wave_sum(cpos[q]);
    const double t4 = wave_sum(sabs[q]), t5 = wave_sum(ssq[q]);
    if (lane == 0) {
      wr[q * 6 + 0] = t0; wr[q * 6 + 1] = t1; wr[q * 6 + 2] = t2; wr[q * 6 + 3] = t3; wr[q * 6 + 4] = t4; wr[q * 6 + 5] = t5;
    }
  }
  const double ts = wave_sum(ssig);
  if (lane == 0) {
    wr[30] = ts;
    wr[31] = 0;
  }
  __syncthreads();
  if (tid < kNMom) {
    double a = 0;
#pragma unroll
    for (int w = 0; w < kNWaves; ++w) a += wred[w * kNMom + tid];
    out[tid] = a;
  }
}

// grid (2 nblk, B): blockIdx.x = 2 block + (scale - 1).  ws [B][nblk][2][kNMom].
template <bool F32>
__global__ __launch_bounds__(kNT) void niqe_block_kernel(const void* __restrict__ img, int H, int W, int shave, int bx_n, NiqeTaps taps,
                                                         double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char niqe_lds[];
  double* m = reinterpret_cast<double*>(niqe_lds);                 // [N][N]
  double* y2 = m + kNB * kNB;                                      // [54][54] (scale 2)
  double* wred = y2 + kNS2 * kNS2;                                 // [6][kNMom]
  uint8_t* yb = reinterpret_cast<uint8_t*>(wred + kNWaves * kNMom);  // [102][102] or [114][114]
  const int tid = threadIdx.x, blk = blockIdx.x >> 1, scale2 = blockIdx.x & 1, b = blockIdx.y;
  const int by = blk / bx_n, bx = blk - by * bx_n;
  const int Hc = ((H - 2 * shave) / kNB) * kNB, Wc = ((W - 2 * shave) / kNB) * kNB;
  const int64_t plane = (int64_t)H * W, base = (int64_t)b * 3 * plane;
  double* out = ws + (((int64_t)b * (gridDim.x >> 1) + blk) * 2 + scale2) * kNMom;

  // the Y bytes of the block and its halo: crop coordinates clamped (scale 1) or reflected (scale 2) into [0, Hc) x [0, Wc)
  const int E = scale2 ? kNY2 : kNY1, halo = scale2 ? 9 : kNR;
  for (int i = tid; i < E * E; i += kNT) {
    const int ry = i / E, rx = i - ry * E;
    int cy = by * kNB - halo + ry, cx = bx * kNB - halo + rx;
    if (scale2) {
      cy = refl(cy, Hc);
      cx = refl(cx, Wc);
    } else {
      cy = clampi(cy, 0, Hc - 1);
      cx = clampi(cx, 0, Wc - 1);
    }
    const int64_t o = base + (int64_t)(cy + shave) * W + (cx + shave);
    yb[i] = y_of_rgb(load_u8<F32>(img, o), load_u8<F32>(img, o + plane), load_u8<F32>(img, o + 2 * plane));
  }
  __syncthreads();

  if (!scale2) {
    niqe_mscn_and_moments<kNB, kNY1, uint8_t>(yb, m, wred, taps, out);
    return;
  }
  // y2 of the block and its 3-pixel halo, positions clamped into the half-size plane (the replicate border of that scale)
  const int H2 = Hc / 2, W2 = Wc / 2;
  for (int i = tid; i < kNS2 * kNS2; i += kNT) {
    const int ly = i / kNS2, lx = i - ly * kNS2;
    const int iy = clampi(by * (kNB / 2) - kNR + ly, 0, H2 - 1), ix = clampi(bx * (kNB / 2) - kNR + lx, 0, W2 - 1);
    // the first of the eight source rows / columns, in staged coordinates: 2 i - 3 - (block origin - 9)
    const int sy = 2 * iy - 3 - (by * kNB - 9), sx = 2 * ix - 3 - (bx * kNB - 9);
    constexpr int tap[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
    int acc = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const uint8_t* row = yb + (sy + t) * kNY2 + sx;
      int ra = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) ra += tap[u] * (int)row[u];
      acc += tap[t] * ra;
    }
    y2[i] = (double)acc * (1.0 / 65536.0);
  }
  __syncthreads();
  niqe_mscn_and_moments<kNB / 2, kNS2, double>(y2, m, wred, taps, out);
}

// One thread per fit: 10 fits and the sharpness of every (image, block).  feats [B nblk][36], sharp [B nblk].
__global__ __launch_bounds__(64) void niqe_fit_kernel(const double* __restrict__ ws, int64_t nrows, const double* __restrict__ gam,
                                                      const double* __restrict__ r_gam, int n_gam, double* __restrict__ feats,
                                                      double* __restrict__ sharp) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= nrows * 11) return;
  const int64_t row = i / 11;
  const int f = (int)(i - row * 11);
  if (f == 10) {
    sharp[row] = ws[row * 2 * kNMom + 30] / (double)(kNB * kNB);
    return;
  }
  const int scale2 = f / 5, q = f - scale2 * 5;
  const double* p = ws + (row * 2 + scale2) * kNMom + q * 6;
  const double n = scale2 ? (double)(kNB * kNB / 4) : (double)(kNB * kNB);
  const double l = sqrt(p[0] / p[1]), r = sqrt(p[2] / p[3]), g = l / r;
  const double mabs = p[4] / n, rhat = mabs * mabs / (p[5] / n);
  const double g2 = g * g + 1.0;
  const double rn = rhat * (g * g * g + 1.0) * (g + 1.0) / (g2 * g2);
  // k = #{r_gam < rn} (the table increases); the argmin is k - 1 or k, the lower index on a tie.  A NaN rn compares false: k = 0.
  int lo = 0, hi = n_gam;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r_gam[mid] < rn) lo = mid + 1; else hi = mid;
  }
  int k = lo;
  if (k >= n_gam) k = n_gam - 1;
  if (k > 0) {
    const double d0 = r_gam[k - 1] - rn, d1 = r_gam[k] - rn;
    if (d0 * d0 <= d1 * d1) k -= 1;
  }
  const double alpha = gam[k];
  const double g1 = tgamma(1.0 / alpha), gq = sqrt(g1 / tgamma(3.0 / alpha));
  const double bl = l * gq, br = r * gq;
  double* o = feats + row * 36 + scale2 * 18;
  if (q == 0) {
    o[0] = alpha;
    o[1] = (bl + br) / 2.0;
  } else {
    o += 2 + (q - 1) * 4;
    o[0] = alpha;
    o[1] = (br - bl) * (tgamma(2.0 / alpha) / g1);
    o[2] = bl;
    o[3] = br;
  }
}

static int64_t niqe_blocks(int H, int W, int shave) { return (int64_t)((H - 2 * shave) / kNB) * ((W - 2 * shave) / kNB); }

// At least one block after shaving; the grids (2 nblk x B workgroups, B nblk 11 / 64 fit workgroups) stay far inside the launch limits.
static bool niqe_shape_ok(int B, int H, int W, int shave) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && shave >= 0 && (int64_t)H - 2 * (int64_t)shave >= kNB &&
         (int64_t)W - 2 * (int64_t)shave >= kNB && niqe_blocks(H, W, shave) * B <= (1 << 28);
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int64_t tgsr_niqe_ws_elems(int B, int H, int W, int shave) {
  if (!niqe_shape_ok(B, H, W, shave)) return 0;
  return (int64_t)B * niqe_blocks(H, W, shave) * 2 * kNMom;
}

extern "C" int tgsr_niqe_features(const void* img, int is_f32, int B, int H, int W, int shave, const double* gam, const double* r_gam,
                                  int n_gam, double* ws, double* feats, double* sharp, void* stream) {
  if (!img || !gam || !r_gam || !ws || !feats || !sharp || n_gam < 1 || !niqe_shape_ok(B, H, W, shave)) return TGSR_EINVAL;
  const int by_n = (H - 2 * shave) / kNB, bx_n = (W - 2 * shave) / kNB;
  const int64_t nblk = (int64_t)by_n * bx_n;
  NiqeTaps taps;
  double sum = 0;
  for (int k = 0; k < kNW; ++k) sum += (taps.w[k] = exp(-(double)((k - kNR) * (k - kNR)) / (2.0 * (7.0 / 6.0) * (7.0 / 6.0))));
  for (int k = 0; k < kNW; ++k) taps.w[k] /= sum;
  static bool attr_set[64] = {false};   // > 64 KB of dynamic LDS needs the opt-in once per DEVICE (see tgsr_damsm.hip)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(niqe_block_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(niqe_block_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return note_launch(e, "hipFuncSetAttribute(niqe_block_kernel)");
    }
    attr_set[dev] = true;
  }
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)(2 * nblk), B), block(kNT);
  if (is_f32)
    hipLaunchKernelGGL(niqe_block_kernel<true>, grid, block, kNiqeLds, s, img, H, W, shave, bx_n, taps, ws);
  else
    hipLaunchKernelGGL(niqe_block_kernel<false>, grid, block, kNiqeLds, s, img, H, W, shave, bx_n, taps, ws);
  const int rc = note_launch(hipGetLastError(), "niqe_block_kernel");
  if (rc != TGSR_OK) return rc;
  const int64_t nrows = (int64_t)B * nblk;
  hipLaunchKernelGGL(niqe_fit_kernel, dim3((unsigned)((nrows * 11 + 63) / 64)), dim3(64), 0, s, ws, nrows, gam, r_gam, n_gam, feats, sharp);
  return note_launch(hipGetLastError(), "niqe_fit_kernel");
}
