// The cycle-consistency (back-projection) objective of the reference's miscc/losses.py, CycleMSE (:785-790):
//   loss = sum_i mean((F.interpolate(sr_i, size=[h, w], mode="bicubic") - lr)^2)      sr_i [B][C][H_i][W_i], lr [B][C][h][w]
// with torch's bicubic rule (align_corners=False, no antialiasing, A = -0.75): per axis, in float32,
//   scale = (float)H / h,  src = scale (y + 0.5f) - 0.5f (not clamped at 0),  i0 = floor(src),  t = src - i0,
//   taps i0 - 1 .. i0 + 2 clamped to [0, H - 1], weights cc2(t + 1), cc1(t), cc1(1 - t), cc2(2 - t).
// cycle_mse_fwd_kernel: ONE launch for all (<= 8) scales, a thread per LR pixel of one scale: 16 taps, diff = resized - lr saved for
// the backward ([n][B][C][h][w]), diff^2 into a per-thread fp32 chain, a fixed LDS tree, one partial per workgroup.
// cycle_mse_finish_kernel adds each scale's partials in index order in fp64 and divides once per scale.
// cycle_mse_bwd_kernel: ONE launch for all scales, GATHER form: a thread owns a run of <= 4 neighbouring SR pixels of one row, walks
// the LR outputs that can reach them (per axis a candidate range - a closed form at an integer ratio, a conservative float32 range
// otherwise - every candidate's four clamped taps tested with the forward's own arithmetic) and writes d_sr once - zeros where no
// tap lands, no memset - with one 16-byte store where the base is 16-byte aligned and W % 4 == 0, element by element otherwise.  A
// further segment of the same grid writes d_lr.
// No atomics anywhere: the same bits on every run, on any stream, inside a captured graph.
#include "tgsr_common.h"

namespace tgsr {

constexpr int kCMThreads = 256;
constexpr int kCMMaxScales = 8;
constexpr int kCMFwdBlocks = 256;       // workgroups (= partials) per scale of the forward launch; larger problems loop
constexpr int kCMBwdBlocks = 1024;      // workgroups per segment (a scale, or d_lr) of the backward launch; larger problems loop
constexpr int kCMMaxSide = 65536;       // every side: the candidate ranges are computed in float32 with a margin of one

struct CycleScale {
  const float* sr;      // forward: the SR image; backward: unused
  float* d_sr;          // backward: its gradient, or NULL
  int H, W;
  float sy, sx;         // (float)H / h, (float)W / w: torch's scales
  float ry, rx;         // (float)h / H, (float)w / W: for the backward's candidate ranges only
  int qy, qx;           // H / h, W / w where that is an integer >= 1 (the candidate range has a closed form there), else 0
  int upr;              // runs of <= 4 pixels per SR row
  int vec;              // d_sr takes 16-byte stores
  int64_t units;        // B C H upr
};

struct CycleArgs {
  CycleScale s[kCMMaxScales];
  int n, B, C, h, w;
  int nbs;                          // forward: workgroups per scale
  int blk0[kCMMaxScales + 2];       // backward: first workgroup of every segment (the scales, then d_lr), and the grid's size
  int64_t per;                      // B C h w
};

// torch's cubic convolution coefficients (UpSample.h: cubic_convolution1 / 2, get_cubic_upsample_coefficients), A = -0.75
__device__ __forceinline__ float cc1(float x) { return ((-0.75f + 2.f) * x - (-0.75f + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cc2(float x) { return ((-0.75f * x - 5.f * -0.75f) * x + 8.f * -0.75f) * x - 4.f * -0.75f; }

// the four clamped taps and weights of output `o` along an axis of `in` input pixels: the one place that rule is written, shared by
// the forward and the backward (explicitly rounded operations: no contraction may make the two disagree on floor(src))
__device__ __forceinline__ void cubic_taps(int o, float scale, int in, int (&idx)[4], float (&c)[4]) {
  const float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)o, 0.5f)), 0.5f);
  const int i0 = min((int)floorf(src), in - 1);
  const float t = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
  c[0] = cc2(t + 1.f);
  c[1] = cc1(t);
  c[2] = cc1(1.f - t);
  c[3] = cc2(2.f - t);
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = max(min(i0 + j - 1, in - 1), 0);
}

__device__ __forceinline__ float cm_block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = kCMThreads / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kCMThreads) void cycle_mse_fwd_kernel(CycleArgs a, const float* __restrict__ lr, float* __restrict__ diff,
                                                                   float* __restrict__ ws) {
  __shared__ float red[kCMThreads];
  const int si = blockIdx.x / a.nbs, blk = blockIdx.x - si * a.nbs;      // uniform over the workgroup
  const CycleScale& s = a.s[si];
  const float* __restrict__ sr = s.sr;
  const int H = s.H, W = s.W;
  const int64_t plane = (int64_t)H * W;
  float acc = 0.f;
  for (int64_t u = (int64_t)blk * kCMThreads + threadIdx.x; u < a.per; u += (int64_t)a.nbs * kCMThreads) {
    const int64_t row = u / a.w;
    const int x = (int)(u - row * a.w);
    const int64_t bc = row / a.h;
    const int y = (int)(row - bc * a.h);
    int iy[4], ix[4];
    float cy[4], cx[4];
    cubic_taps(y, s.sy, H, iy, cy);
    cubic_taps(x, s.sx, W, ix, cx);
    const float* __restrict__ p = sr + bc * plane;
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* __restrict__ q = p + (int64_t)iy[j] * W;
      r += cy[j] * (cx[0] * q[ix[0]] + cx[1] * q[ix[1]] + cx[2] * q[ix[2]] + cx[3] * q[ix[3]]);
    }
    const float d = r - lr[u];
    diff[(int64_t)si * a.per + u] = d;
    acc += d * d;
  }
  const float total = cm_block_sum(acc, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = total;
}

// terms[i] = (scale i's partials, added in index order) / n_elems; loss[0] = their fp32 sum in scale order (the reference's `+=`)
__global__ __launch_bounds__(kCMThreads) void cycle_mse_finish_kernel(const float* __restrict__ ws, int n, int nbs, float n_elems,
                                                                      float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ double red[kCMThreads];
  const int tid = threadIdx.x;
  float total = 0.f;
  for (int i = 0; i < n; ++i) {
    double v = 0;
    for (int k = tid; k < nbs; k += kCMThreads) v = __dadd_rn(v, (double)ws[i * nbs + k]);
    red[tid] = v;
    __syncthreads();
    for (int o = kCMThreads / 2; o >= 1; o >>= 1) {
      if (tid < o) red[tid] = __dadd_rn(red[tid], red[tid + o]);
      __syncthreads();
    }
    if (tid == 0) {
      const float term = __fdiv_rn((float)red[0], n_elems);
      terms[i] = term;
      total = i == 0 ? term : __fadd_rn(total, term);
    }
    __syncthreads();
  }
  if (tid == 0) loss[0] = total;
}

// the LR outputs along one axis that can hold SR pixel p among their taps: i0 in [p - 2, p + 1], i.e. src in [p - 2, p + 2), i.e.
// o in [(p - 1.5) / scale - 0.5, (p + 2.5) / scale - 0.5) - widened by one on either side against float32 rounding (every candidate
// is tested exactly, so a wider range costs time only).  Clamped taps add nothing: a tap clamped onto 0 comes from i0 <= 1, one
// clamped onto in - 1 from i0 >= in - 3, both inside [p - 2, p + 1] for that p.
// At an integer ratio q the range has a closed form: src = q o + (q - 1) / 2 exactly, i0 = q o + k with k = (q - 1) >> 1 (t = 1/2 at
// even ratios, 0 at odd ones; exact in float32 because every side is <= 65536: q (o + 0.5) <= 2^16 carries one fractional bit), so
// o in [ceil((p - 2 - k) / q), floor((p + 1 - k) / q)] - no margin, at most ceil(4 / q) candidates.
__device__ __forceinline__ void cm_candidates(int p_lo, int p_hi, float inv_scale, int q, int out, int* lo, int* hi) {
  int a, b;
  if (q > 0) {
    const int k = (q - 1) >> 1, na = p_lo - 2 - k, nb = p_hi + 1 - k;
    a = na >= 0 ? (na + q - 1) / q : -((-na) / q);
    b = nb >= 0 ? nb / q : -((-nb + q - 1) / q);
  } else {
    a = (int)floorf(((float)p_lo - 1.5f) * inv_scale - 0.5f) - 1;
    b = (int)ceilf(((float)p_hi + 2.5f) * inv_scale - 0.5f) + 1;
  }
  *lo = max(a, 0);
  *hi = min(b, out - 1);
}

// d_sr[b][c][Y][X] = g c2 sum_{y, x} WY(y, Y) WX(x, X) diff[b][c][y][x],  WY(y, Y) = the sum of y's weights whose clamped tap is Y;
// d_lr = -g c2 sum_i diff_i
__global__ __launch_bounds__(kCMThreads) void cycle_mse_bwd_kernel(CycleArgs a, const float* __restrict__ grad,
                                                                   const float* __restrict__ diff, float c2, float* __restrict__ d_lr) {
  int seg = 0;
#pragma unroll
  for (int i = 1; i <= kCMMaxScales; ++i)
    if (i <= a.n && (int)blockIdx.x >= a.blk0[i]) seg = i;           // uniform over the workgroup
  const int blk = blockIdx.x - a.blk0[seg], nblk = a.blk0[seg + 1] - a.blk0[seg];
  const float coef = grad[0] * c2;
  if (seg == a.n) {                                                  // the d_lr segment (present only where d_lr is asked for)
    for (int64_t u = (int64_t)blk * kCMThreads + threadIdx.x; u < a.per; u += (int64_t)nblk * kCMThreads) {
      float sum = diff[u];
      for (int i = 1; i < a.n; ++i) sum += diff[(int64_t)i * a.per + u];
      d_lr[u] = -coef * sum;
    }
    return;
  }
  const CycleScale& s = a.s[seg];
  float* __restrict__ out = s.d_sr;
  const int H = s.H, W = s.W, h = a.h, w = a.w;
  const bool vec = s.vec != 0;
  const float* __restrict__ dseg = diff + (int64_t)seg * a.per;
  for (int64_t u = (int64_t)blk * kCMThreads + threadIdx.x; u < s.units; u += (int64_t)nblk * kCMThreads) {
    const int64_t row = u / s.upr;
    const int X0 = 4 * (int)(u - row * s.upr), nv = min(4, W - X0);
    const int64_t bc = row / H;
    const int Y = (int)(row - bc * H);
    int ylo, yhi, xlo, xhi;
    cm_candidates(Y, Y, s.ry, s.qy, h, &ylo, &yhi);
    cm_candidates(X0, X0 + nv - 1, s.rx, s.qx, w, &xlo, &xhi);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int y = ylo; y <= yhi; ++y) {
      int iy[4];
      float cy[4];
      cubic_taps(y, s.sy, H, iy, cy);
      float wy = 0.f;
      bool hit = false;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (iy[j] == Y) {
          wy += cy[j];
          hit = true;
        }
      if (!hit) continue;
      const float* __restrict__ drow = dseg + (bc * h + y) * w;
      for (int x = xlo; x <= xhi; ++x) {
        int ix[4];
        float cx[4];
        cubic_taps(x, s.sx, W, ix, cx);
        const float d = wy * drow[x];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          float wx = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) wx += ix[j] == X0 + p ? cx[j] : 0.f;
          acc[p] += wx * d;
        }
      }
    }
    float* __restrict__ o = out + row * W + X0;
    if (vec) {
      *reinterpret_cast<float4*>(o) = make_float4(coef * acc[0], coef * acc[1], coef * acc[2], coef * acc[3]);
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < nv) o[p] = coef * acc[p];
    }
  }
}

// the shape rules of all three entries; fills everything of `a` that does not depend on pointers
static bool cm_shape(const int* H, const int* W, int n, int B, int C, int h, int w, CycleArgs* a) {
  if (!H || !W || n < 1 || n > kCMMaxScales || B < 1 || C < 1 || h < 1 || w < 1 || h > kCMMaxSide || w > kCMMaxSide) return false;
  const int64_t per = (int64_t)B * C * h * w;
  if (per > ((int64_t)1 << 40)) return false;
  *a = CycleArgs{};
  a->n = n, a->B = B, a->C = C, a->h = h, a->w = w, a->per = per;
  const int64_t g = (per + kCMThreads - 1) / kCMThreads;
  a->nbs = (int)(g > kCMFwdBlocks ? kCMFwdBlocks : g);
  for (int i = 0; i < n; ++i) {
    if (H[i] < 1 || W[i] < 1 || H[i] > kCMMaxSide || W[i] > kCMMaxSide) return false;
    if ((int64_t)B * C * H[i] * W[i] > ((int64_t)1 << 40)) return false;
    CycleScale& s = a->s[i];
    s.H = H[i], s.W = W[i];
    s.sy = (float)H[i] / (float)h, s.sx = (float)W[i] / (float)w;
    s.ry = (float)h / (float)H[i], s.rx = (float)w / (float)W[i];
    s.qy = H[i] % h == 0 ? H[i] / h : 0, s.qx = W[i] % w == 0 ? W[i] / w : 0;
    s.upr = (W[i] + 3) / 4;
    s.units = (int64_t)B * C * H[i] * s.upr;
  }
  return true;
}

static int cm_seg_blocks(int64_t units) {
  const int64_t g = (units + kCMThreads - 1) / kCMThreads;
  return (int)(g > kCMBwdBlocks ? kCMBwdBlocks : g);
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int64_t tgsr_cycle_mse_ws_elems(const int* H, const int* W, int n, int B, int C, int h, int w) {
  CycleArgs a;
  return cm_shape(H, W, n, B, C, h, w, &a) ? (int64_t)n * a.nbs : 0;
}

extern "C" int tgsr_cycle_mse_fwd(const float* const* sr, const int* H, const int* W, int n, const float* lr, int B, int C, int h, int w,
                                  float* ws, float* diff, float* loss, float* terms, void* stream) {
  CycleArgs a;
  if (!sr || !lr || !ws || !diff || !loss || !terms || !cm_shape(H, W, n, B, C, h, w, &a)) return TGSR_EINVAL;
  for (int i = 0; i < n; ++i) {
    if (!sr[i]) return TGSR_EINVAL;
    a.s[i].sr = sr[i];
  }
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(cycle_mse_fwd_kernel, dim3(n * a.nbs), dim3(kCMThreads), 0, st, a, lr, diff, ws);
  const int rc = note_launch(hipGetLastError(), "cycle_mse_fwd_kernel");
  if (rc != TGSR_OK) return rc;
  hipLaunchKernelGGL(cycle_mse_finish_kernel, dim3(1), dim3(kCMThreads), 0, st, ws, n, a.nbs, (float)a.per, loss, terms);
  return note_launch(hipGetLastError(), "cycle_mse_finish_kernel");
}

extern "C" int tgsr_cycle_mse_bwd(const float* grad, const float* diff, const int* H, const int* W, int n, int B, int C, int h, int w,
                                  float* const* d_sr, float* d_lr, void* stream) {
  CycleArgs a;
  if (!grad || !diff || !cm_shape(H, W, n, B, C, h, w, &a)) return TGSR_EINVAL;
  int blocks = 0;
  bool any = d_lr != nullptr;
  for (int i = 0; i < n; ++i) {
    float* p = d_sr ? d_sr[i] : nullptr;
    a.s[i].d_sr = p;
    a.s[i].vec = p && a.s[i].W % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    a.blk0[i] = blocks;
    if (p) {
      any = true;
      blocks += cm_seg_blocks(a.s[i].units);
    }
  }
  if (!any) return TGSR_EINVAL;
  a.blk0[n] = blocks;
  if (d_lr) blocks += cm_seg_blocks(a.per);
  a.blk0[n + 1] = blocks;
  const float c2 = (float)(2.0 / (double)a.per);
  hipLaunchKernelGGL(cycle_mse_bwd_kernel, dim3(blocks), dim3(kCMThreads), 0, as_stream(stream), a, grad, diff, c2, d_lr);
  return note_launch(hipGetLastError(), "cycle_mse_bwd_kernel");
}
