// Image quality of the SR path on the device: PSNR / RMSE on RGB and on Y, SSIM on Y, of uint8 images as the reference's caller
// saves them (trainer_objective.py:153-155 quantises, :168-181 rgb2y / psnr score).
//   quantisation  a float image becomes bytes by tgsr_to_uint8's rule, round_half_even(clip((x + 1) * 127.5, 0, 255)): fp32 add, then
//                 fp32 multiply, no FMA.  The loader's normalisation (u / 255 - 0.5) / 0.5 followed by it returns every byte unchanged.
//   Y             rgb2y byte for byte: f = fp32(u8) / fp32(255) (a correctly rounded fp32 division), then in fp64, left to right,
//                 y = f_r (65.481 / 255) + f_g (128.553 / 255) + f_b (24.966 / 255) + 16 / 255; byte = trunc(y 255 + 0.5), 16..235.
//   SSE           exact integer sums of squared byte differences; the host takes rmse = sqrt(sse / n), psnr = 20 log10(255 / rmse).
//   SSIM          Wang et al. 2004 as in ssim.m: 11 x 11 Gaussian window (sigma 1.5, sum 1), 'valid' filtering, K1 = 0.01, K2 = 0.03,
//                 L = 255, sigma^2 = E[x^2] - mu^2, all in fp64; the kernels return the SUM over the windows, the host divides.
// sr_metrics_tile_kernel: one workgroup per (image, 32 x 32 tile of the shaved crop).  Both Y tiles with their 5-pixel halo (42 x 42)
// stay in LDS as bytes; the Gaussian runs as a separable pass over the five maps x, y, x^2, y^2, xy: rows first into an fp64 LDS image
// [5][42][32] (52.5 KiB - two workgroups per CU), then columns in registers.  Per tile it writes (SSE RGB, SSE Y, sum of the SSIM of
// the windows centred in the tile) into the caller's workspace; sr_metrics_finish_kernel adds a image's tiles in tile order.
// No atomics, every reduction in a fixed order: the same bits on every run, on any stream, inside a captured graph.
#include "tgsr_common.h"
#include "tgsr_y_plane.h"

namespace tgsr {

constexpr int kMT = 32;                 // tile edge
constexpr int kMR = 5;                  // window radius
constexpr int kMW = 2 * kMR + 1;        // window edge
constexpr int kME = kMT + 2 * kMR;      // tile + halo edge

struct GaussTaps {
  double g[kMW];
};

template <bool SR_F32, bool HR_F32>
__global__ __launch_bounds__(256) void sr_metrics_tile_kernel(const void* __restrict__ sr, const void* __restrict__ hr, int H, int W,
                                                              int shave, int tiles_x, GaussTaps taps, double* __restrict__ ws) {
  __shared__ uint8_t ya[kME][kME], yb[kME][kME];
  __shared__ double hrow[5][kME][kMT];
  __shared__ double red_d[256];
  __shared__ uint32_t red_u[2][256];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int Hc = H - 2 * shave, Wc = W - 2 * shave;
  const int64_t plane = (int64_t)H * W, img = (int64_t)b * 3 * plane;

  // 1. bytes -> Y of both images for the tile and its halo; the squared differences of the tile's own pixels
  uint32_t sse_rgb = 0, sse_y = 0;
  for (int i = tid; i < kME * kME; i += 256) {
    const int ry = i / kME, rx = i - ry * kME;
    const int cy = ty * kMT - kMR + ry, cx = tx * kMT - kMR + rx;          // position inside the crop
    uint8_t va = 0, vb = 0;
    if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) {
      const int64_t o = img + (int64_t)(cy + shave) * W + (cx + shave);
      const uint8_t ar = load_u8<SR_F32>(sr, o), ag = load_u8<SR_F32>(sr, o + plane), ab = load_u8<SR_F32>(sr, o + 2 * plane);
      const uint8_t br = load_u8<HR_F32>(hr, o), bg = load_u8<HR_F32>(hr, o + plane), bb = load_u8<HR_F32>(hr, o + 2 * plane);
      va = y_of_rgb(ar, ag, ab);
      vb = y_of_rgb(br, bg, bb);
      if (ry >= kMR && ry < kMR + kMT && rx >= kMR && rx < kMR + kMT) {
        const int dr = (int)ar - (int)br, dg = (int)ag - (int)bg, db = (int)ab - (int)bb, dy = (int)va - (int)vb;
        sse_rgb += (uint32_t)(dr * dr + dg * dg + db * db);
        sse_y += (uint32_t)(dy * dy);
      }
    }
    ya[ry][rx] = va;
    yb[ry][rx] = vb;
  }
  __syncthreads();

  // 2. the Gaussian along the rows, five maps
  for (int i = tid; i < kME * kMT; i += 256) {
    const int ry = i / kMT, c = i - ry * kMT;
    double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int k = 0; k < kMW; ++k) {
      const double g = taps.g[k], x = (double)ya[ry][c + k], y = (double)yb[ry][c + k];
      sx = __dadd_rn(sx, __dmul_rn(g, x));
      sy = __dadd_rn(sy, __dmul_rn(g, y));
      sxx = __dadd_rn(sxx, __dmul_rn(g, __dmul_rn(x, x)));
      syy = __dadd_rn(syy, __dmul_rn(g, __dmul_rn(y, y)));
      sxy = __dadd_rn(sxy, __dmul_rn(g, __dmul_rn(x, y)));
    }
    hrow[0][ry][c] = sx;
    hrow[1][ry][c] = sy;
    hrow[2][ry][c] = sxx;
    hrow[3][ry][c] = syy;
    hrow[4][ry][c] = sxy;
  }
  __syncthreads();

  // 3. ... along the columns, and the SSIM of every window whose centre lies in this tile and whose 11 x 11 pixels lie in the crop
  constexpr double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  double ssim = 0;
  for (int i = tid; i < kMT * kMT; i += 256) {
    const int wy = i / kMT, wx = i - wy * kMT;
    const int cy = ty * kMT + wy, cx = tx * kMT + wx;
    if (cy < kMR || cy >= Hc - kMR || cx < kMR || cx >= Wc - kMR) continue;
    double m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double a = 0;
#pragma unroll
      for (int k = 0; k < kMW; ++k) a = __dadd_rn(a, __dmul_rn(taps.g[k], hrow[q][wy + k][wx]));
      m[q] = a;
    }
    const double mxx = __dmul_rn(m[0], m[0]), myy = __dmul_rn(m[1], m[1]), mxy = __dmul_rn(m[0], m[1]);
    const double vx = __dadd_rn(m[2], -mxx), vy = __dadd_rn(m[3], -myy), cxy = __dadd_rn(m[4], -mxy);
    const double num = __dmul_rn(__dadd_rn(__dadd_rn(mxy, mxy), C1), __dadd_rn(__dadd_rn(cxy, cxy), C2));
    const double den = __dmul_rn(__dadd_rn(__dadd_rn(mxx, myy), C1), __dadd_rn(__dadd_rn(vx, vy), C2));
    ssim = __dadd_rn(ssim, __ddiv_rn(num, den));
  }

  // 4. the tile's three sums, by a fixed tree
  red_d[tid] = ssim;
  red_u[0][tid] = sse_rgb;
  red_u[1][tid] = sse_y;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      red_d[tid] = __dadd_rn(red_d[tid], red_d[tid + o]);
      red_u[0][tid] += red_u[0][tid + o];
      red_u[1][tid] += red_u[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* p = ws + ((int64_t)b * gridDim.x + tile) * 3;
    p[0] = (double)red_u[0][0];
    p[1] = (double)red_u[1][0];
    p[2] = red_d[0];
  }
}

// out[b][3] = the sums of image b's tile partials, in tile order (the integer sums stay below 2^53: exact).
__global__ void sr_metrics_finish_kernel(const double* __restrict__ ws, int ntiles, double* __restrict__ out) {
  const int b = blockIdx.x, q = threadIdx.x;
  if (q >= 3) return;
  const double* p = ws + (int64_t)b * ntiles * 3 + q;
  double a = 0;
  for (int t = 0; t < ntiles; ++t) a = __dadd_rn(a, p[(int64_t)t * 3]);
  out[b * 3 + q] = a;
}

__global__ void rgb_to_y_u8_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ y, int64_t plane, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / plane, o = b * 3 * plane + (i - b * plane);
    y[i] = y_of_rgb(rgb[o], rgb[o + plane], rgb[o + 2 * plane]);
  }
}

static inline int metrics_tiles(int n) { return (n + kMT - 1) / kMT; }

static bool metrics_shape_ok(int B, int H, int W, int shave) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && shave >= 0 && (int64_t)H - 2 * (int64_t)shave >= kMW &&
         (int64_t)W - 2 * (int64_t)shave >= kMW;
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int64_t tgsr_sr_metrics_ws_elems(int B, int H, int W, int shave) {
  if (!metrics_shape_ok(B, H, W, shave)) return 0;
  return (int64_t)B * metrics_tiles(H - 2 * shave) * metrics_tiles(W - 2 * shave) * 3;
}

extern "C" int tgsr_sr_metrics(const void* sr, int sr_f32, const void* hr, int hr_f32, int B, int H, int W, int shave, double* ws,
                               double* out, void* stream) {
  if (!sr || !hr || !ws || !out || !metrics_shape_ok(B, H, W, shave)) return TGSR_EINVAL;
  const int tiles_y = metrics_tiles(H - 2 * shave), tiles_x = metrics_tiles(W - 2 * shave);
  GaussTaps taps;
  double sum = 0;
  for (int k = 0; k < kMW; ++k) sum += (taps.g[k] = exp(-(double)((k - kMR) * (k - kMR)) / (2.0 * 1.5 * 1.5)));
  for (int k = 0; k < kMW; ++k) taps.g[k] /= sum;
  hipStream_t s = as_stream(stream);
  const dim3 grid(tiles_x * tiles_y, B), block(256);
  if (sr_f32 && hr_f32)
    hipLaunchKernelGGL((sr_metrics_tile_kernel<true, true>), grid, block, 0, s, sr, hr, H, W, shave, tiles_x, taps, ws);
  else if (sr_f32)
    hipLaunchKernelGGL((sr_metrics_tile_kernel<true, false>), grid, block, 0, s, sr, hr, H, W, shave, tiles_x, taps, ws);
  else if (hr_f32)
    hipLaunchKernelGGL((sr_metrics_tile_kernel<false, true>), grid, block, 0, s, sr, hr, H, W, shave, tiles_x, taps, ws);
  else
    hipLaunchKernelGGL((sr_metrics_tile_kernel<false, false>), grid, block, 0, s, sr, hr, H, W, shave, tiles_x, taps, ws);
  const int rc = note_launch(hipGetLastError(), "sr_metrics_tile_kernel");
  if (rc != TGSR_OK) return rc;
  hipLaunchKernelGGL(sr_metrics_finish_kernel, dim3(B), dim3(64), 0, s, ws, tiles_x * tiles_y, out);
  return note_launch(hipGetLastError(), "sr_metrics_finish_kernel");
}

extern "C" int tgsr_rgb_to_y_u8(const uint8_t* rgb, int B, int H, int W, uint8_t* y, void* stream) {
  if (!rgb || !y || B < 1 || H < 1 || W < 1) return TGSR_EINVAL;
  const int64_t plane = (int64_t)H * W, total = plane * B;
  const int64_t g = (total + 255) / 256;
  hipLaunchKernelGGL(rgb_to_y_u8_kernel, dim3((unsigned)(g > 16384 ? 16384 : g)), dim3(256), 0, as_stream(stream), rgb, y, plane, total);
  return note_launch(hipGetLastError(), "rgb_to_y_u8_kernel");
}
