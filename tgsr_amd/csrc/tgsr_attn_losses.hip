// The training objectives that read the generator's word-attention maps (the reference's miscc/losses.py):
//   weight_MSE (:792-804), one scale:  wmax[b][y][x] = max_t att[b][t][y][x]  (the lowest t on a tie - the reference pins none),
//                  wups = wmax at (Y / r, X / r)  (nn.Upsample's nearest rule at an integer ratio r = H / h = W / w),
//                  term = sum_{b,c,Y,X} (T wups) (fake - label)^2 / (H W B C);
//   words_reweight_loss (:137-232):  conf[b][t] = sum of the values of att[b][t] that lie strictly above
//                  (float)(2.0 * (2.0 / (double)len_b)) - the comparison in float32, as torch compares a float32 map with a Python
//                  double - for t < len_b, 0 behind the caption's length.
// weight_mse_fwd_kernel reads each of fake, label and att once: a thread owns up to four neighbouring map pixels of one map row, takes
// their maximum over the T words, writes it (and the word's index, for the backward; and the up-sampled map where the caller keeps
// it) and walks the r x r image pixels of every channel under them.  weight_mse_bwd_kernel has the same shape and writes d_fake,
// d_label and ALL T words of d_att (the sum at the saved index, zeros elsewhere: no memset).  16 bytes per lane where every pointer
// is 16-byte aligned, the map width a multiple of 4 and r in {1, 2, 4}; element by element otherwise (any base, any width, any r).
// Reductions: per-thread fp32 sums, a fixed LDS tree per workgroup, the workgroups' partials added in index order by a finish
// kernel.  No atomics: the same bits on every run, on any stream, inside a captured graph.
#include "tgsr_common.h"

namespace tgsr {

constexpr int kALThreads = 256;
constexpr int kALMaxBlocks = 1024;      // workgroups (= partials) of one weight_mse launch: four per CU; larger problems loop

__device__ __forceinline__ float block_sum_256(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = kALThreads / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// conf[b][t]: one workgroup per map.
__global__ __launch_bounds__(kALThreads) void attn_confidence_kernel(const float* __restrict__ att, const int32_t* __restrict__ cap_lens,
                                                                     int T, int Q, float* __restrict__ conf) {
  __shared__ float red[kALThreads];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int len = cap_lens[b];
  if (len < 1 || len > T || t >= len) {             // uniform over the workgroup: the map is not read
    if (tid == 0) conf[(int64_t)b * T + t] = 0.f;
    return;
  }
  const float thr = (float)(2.0 * (2.0 / (double)len));
  const float* __restrict__ p = att + ((int64_t)b * T + t) * Q;
  // [0, head) up to the first 16-byte boundary, [head, head + 4 nv) as 16-byte loads, the rest one by one
  const int mis = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
  const int head = min(Q, (4 - mis) & 3);
  const int nv = (Q - head) >> 2;
  float s = 0.f;
  if (tid < head) {
    const float v = p[tid];
    s += v > thr ? v : 0.f;
  }
  const float4* __restrict__ pv = reinterpret_cast<const float4*>(p + head);
  for (int i = tid; i < nv; i += kALThreads) {
    const float4 v = pv[i];
    s += v.x > thr ? v.x : 0.f;
    s += v.y > thr ? v.y : 0.f;
    s += v.z > thr ? v.z : 0.f;
    s += v.w > thr ? v.w : 0.f;
  }
  const int tail = head + 4 * nv;
  if (tail + tid < Q) {                             // at most three elements
    const float v = p[tail + tid];
    s += v > thr ? v : 0.f;
  }
  const float total = block_sum_256(s, red);
  if (tid == 0) conf[(int64_t)b * T + t] = total;
}

struct WmseShape {
  int B, C, T, H, W, h, w, r;
  int upr;              // units (runs of <= 4 map pixels) per map row
  int64_t units;        // B h upr
};

__device__ __forceinline__ void ld4(const float* __restrict__ p, float (&v)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

__device__ __forceinline__ void st4(float* __restrict__ p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// R: the ratio as a template integer (0 = read it from the shape); VEC: every access 16 bytes wide (R > 0, w % 4 == 0, aligned bases)
template <int R, bool VEC>
__global__ __launch_bounds__(kALThreads) void weight_mse_fwd_kernel(const float* __restrict__ fake, const float* __restrict__ label,
                                                                    const float* __restrict__ att, WmseShape s, float* __restrict__ ws,
                                                                    float* __restrict__ wmax, uint8_t* __restrict__ widx,
                                                                    float* __restrict__ wlast) {
  static_assert(!VEC || R > 0, "the 16-byte form needs the ratio at compile time");
  __shared__ float red[kALThreads];
  const int r = R > 0 ? R : s.r;
  const int64_t mplane = (int64_t)s.h * s.w, iplane = (int64_t)s.H * s.W;
  float acc = 0.f;
  for (int64_t u = (int64_t)blockIdx.x * kALThreads + threadIdx.x; u < s.units; u += (int64_t)gridDim.x * kALThreads) {
    const int64_t row = u / s.upr;
    const int k = (int)(u - row * s.upr), b = (int)(row / s.h), y = (int)(row - (int64_t)b * s.h);
    const int x0 = 4 * k, n = min(4, s.w - x0);
    const float* __restrict__ ap = att + (int64_t)b * s.T * mplane + (int64_t)y * s.w + x0;
    float best[4];
    int bi[4] = {0, 0, 0, 0};
    if (VEC) {
      ld4(ap, best);
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) best[p] = p < n ? ap[p] : 0.f;
    }
    for (int t = 1; t < s.T; ++t) {
      float v[4];
      if (VEC) {
        ld4(ap + t * mplane, v);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = p < n ? ap[t * mplane + p] : 0.f;
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (v[p] > best[p]) {                      // strictly: the lowest index keeps a tie
          best[p] = v[p];
          bi[p] = t;
        }
    }
    const int64_t mo = ((int64_t)b * s.h + y) * s.w + x0;
    if (VEC) {
      st4(wmax + mo, best);
      *reinterpret_cast<uint32_t*>(widx + mo) = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < n) {
          wmax[mo + p] = best[p];
          widx[mo + p] = (uint8_t)bi[p];
        }
    }
    float tw[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) tw[p] = (float)s.T * best[p];
    if (VEC) {
      for (int c = 0; c < s.C; ++c)
#pragma unroll
        for (int dy = 0; dy < R; ++dy) {
          const int64_t o = ((int64_t)b * s.C + c) * iplane + (int64_t)(y * R + dy) * s.W + (int64_t)x0 * R;
#pragma unroll
          for (int q = 0; q < R; ++q) {
            float f[4], l[4];
            ld4(fake + o + 4 * q, f);
            ld4(label + o + 4 * q, l);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float d = f[e] - l[e];
              acc += tw[(4 * q + e) / R] * (d * d);
            }
          }
        }
      if (wlast != nullptr) {
#pragma unroll
        for (int dy = 0; dy < R; ++dy) {
          const int64_t o = (int64_t)b * iplane + (int64_t)(y * R + dy) * s.W + (int64_t)x0 * R;
#pragma unroll
          for (int q = 0; q < R; ++q) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = best[(4 * q + e) / R];
            st4(wlast + o + 4 * q, v);
          }
        }
      }
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p >= n) continue;
        for (int c = 0; c < s.C; ++c)
          for (int dy = 0; dy < r; ++dy) {
            const int64_t o = ((int64_t)b * s.C + c) * iplane + (int64_t)(y * r + dy) * s.W + (int64_t)(x0 + p) * r;
            for (int dx = 0; dx < r; ++dx) {
              const float d = fake[o + dx] - label[o + dx];
              acc += tw[p] * (d * d);
            }
          }
        if (wlast != nullptr)
          for (int dy = 0; dy < r; ++dy) {
            const int64_t o = (int64_t)b * iplane + (int64_t)(y * r + dy) * s.W + (int64_t)(x0 + p) * r;
            for (int dx = 0; dx < r; ++dx) wlast[o + dx] = best[p];
          }
      }
    }
  }
  const float total = block_sum_256(acc, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = total;
}

// loss = (the partials, added in index order) / n_elems
__global__ __launch_bounds__(kALThreads) void weight_mse_finish_kernel(const float* __restrict__ ws, int nparts, float n_elems,
                                                                       float* __restrict__ loss) {
  __shared__ double red[kALThreads];
  const int tid = threadIdx.x;
  double a = 0;
  for (int i = tid; i < nparts; i += kALThreads) a = __dadd_rn(a, (double)ws[i]);
  red[tid] = a;
  __syncthreads();
  for (int o = kALThreads / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] = __dadd_rn(red[tid], red[tid + o]);
    __syncthreads();
  }
  if (tid == 0) loss[0] = __fdiv_rn((float)red[0], n_elems);
}

// d_fake = g 2 T wups (fake - label) / N, d_label = -d_fake, d_att[b][t][y][x] = (t == widx) g T / N sum_{c, r x r} (fake - label)^2
template <int R, bool VEC>
__global__ __launch_bounds__(kALThreads) void weight_mse_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ fake,
                                                                    const float* __restrict__ label, const float* __restrict__ wmax,
                                                                    const uint8_t* __restrict__ widx, WmseShape s, float c_img,
                                                                    float c_att, float* __restrict__ d_fake, float* __restrict__ d_label,
                                                                    float* __restrict__ d_att) {
  static_assert(!VEC || R > 0, "the 16-byte form needs the ratio at compile time");
  const int r = R > 0 ? R : s.r;
  const int64_t mplane = (int64_t)s.h * s.w, iplane = (int64_t)s.H * s.W;
  const float g = grad[0];
  const float gi = g * c_img, ga = g * c_att;       // g 2 T / N, g T / N
  for (int64_t u = (int64_t)blockIdx.x * kALThreads + threadIdx.x; u < s.units; u += (int64_t)gridDim.x * kALThreads) {
    const int64_t row = u / s.upr;
    const int k = (int)(u - row * s.upr), b = (int)(row / s.h), y = (int)(row - (int64_t)b * s.h);
    const int x0 = 4 * k, n = min(4, s.w - x0);
    const int64_t mo = ((int64_t)b * s.h + y) * s.w + x0;
    float wm[4], sq[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4];
    if (VEC) {
      ld4(wmax + mo, wm);
      const uint32_t pk = *reinterpret_cast<const uint32_t*>(widx + mo);
#pragma unroll
      for (int p = 0; p < 4; ++p) bi[p] = (int)((pk >> (8 * p)) & 255u);
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        wm[p] = p < n ? wmax[mo + p] : 0.f;
        bi[p] = p < n ? (int)widx[mo + p] : 0;
      }
    }
    float cw[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) cw[p] = gi * wm[p];
    if (VEC) {
      for (int c = 0; c < s.C; ++c)
#pragma unroll
        for (int dy = 0; dy < R; ++dy) {
          const int64_t o = ((int64_t)b * s.C + c) * iplane + (int64_t)(y * R + dy) * s.W + (int64_t)x0 * R;
#pragma unroll
          for (int q = 0; q < R; ++q) {
            float f[4], l[4], df[4], dl[4];
            ld4(fake + o + 4 * q, f);
            ld4(label + o + 4 * q, l);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int p = (4 * q + e) / R;
              const float d = f[e] - l[e];
              sq[p] += d * d;
              df[e] = cw[p] * d;
              dl[e] = -df[e];
            }
            if (d_fake != nullptr) st4(d_fake + o + 4 * q, df);
            if (d_label != nullptr) st4(d_label + o + 4 * q, dl);
          }
        }
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p >= n) continue;
        for (int c = 0; c < s.C; ++c)
          for (int dy = 0; dy < r; ++dy) {
            const int64_t o = ((int64_t)b * s.C + c) * iplane + (int64_t)(y * r + dy) * s.W + (int64_t)(x0 + p) * r;
            for (int dx = 0; dx < r; ++dx) {
              const float d = fake[o + dx] - label[o + dx];
              sq[p] += d * d;
              const float df = cw[p] * d;
              if (d_fake != nullptr) d_fake[o + dx] = df;
              if (d_label != nullptr) d_label[o + dx] = -df;
            }
          }
      }
    }
    if (d_att != nullptr) {
      float* __restrict__ dp = d_att + (int64_t)b * s.T * mplane + (int64_t)y * s.w + x0;
      for (int t = 0; t < s.T; ++t) {
        float v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = bi[p] == t ? ga * sq[p] : 0.f;
        if (VEC) {
          st4(dp + t * mplane, v);
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (p < n) dp[t * mplane + p] = v[p];
        }
      }
    }
  }
}

static bool wmse_shape(int B, int C, int T, int H, int W, int h, int w, WmseShape* s) {
  if (B < 1 || C < 1 || T < 1 || T > 255 || H < 1 || W < 1 || h < 1 || w < 1) return false;
  if (H % h != 0 || W % w != 0 || H / h != W / w) return false;
  const int64_t upr = ((int64_t)w + 3) / 4;
  if ((int64_t)B * h > INT32_MAX || (int64_t)H * W * C > ((int64_t)1 << 40)) return false;
  *s = WmseShape{B, C, T, H, W, h, w, H / h, (int)upr, (int64_t)B * h * upr};
  return true;
}

static int wmse_blocks(const WmseShape& s) {
  const int64_t g = (s.units + kALThreads - 1) / kALThreads;
  return (int)(g > kALMaxBlocks ? kALMaxBlocks : g);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace tgsr

using namespace tgsr;

extern "C" int tgsr_attn_confidence(const float* att, const int32_t* cap_lens, int B, int T, int Q, float* conf, void* stream) {
  if (!att || !cap_lens || !conf || B < 1 || B > 65535 || T < 1 || T > 255 || Q < 1) return TGSR_EINVAL;
  hipLaunchKernelGGL(attn_confidence_kernel, dim3(T, B), dim3(kALThreads), 0, as_stream(stream), att, cap_lens, T, Q, conf);
  return note_launch(hipGetLastError(), "attn_confidence_kernel");
}

extern "C" int64_t tgsr_weight_mse_ws_elems(int B, int C, int T, int H, int W, int h, int w) {
  WmseShape s;
  return wmse_shape(B, C, T, H, W, h, w, &s) ? wmse_blocks(s) : 0;
}

#define TGSR_WMSE_DISPATCH(KERNEL, ...)                                                                                 \
  do {                                                                                                                  \
    if (vec && s.r == 1) hipLaunchKernelGGL((KERNEL<1, true>), dim3(nb), dim3(kALThreads), 0, st, __VA_ARGS__);         \
    else if (vec && s.r == 2) hipLaunchKernelGGL((KERNEL<2, true>), dim3(nb), dim3(kALThreads), 0, st, __VA_ARGS__);    \
    else if (vec && s.r == 4) hipLaunchKernelGGL((KERNEL<4, true>), dim3(nb), dim3(kALThreads), 0, st, __VA_ARGS__);    \
    else hipLaunchKernelGGL((KERNEL<0, false>), dim3(nb), dim3(kALThreads), 0, st, __VA_ARGS__);                        \
  } while (0)

extern "C" int tgsr_weight_mse_fwd(const float* fake, const float* label, const float* att, int B, int C, int T, int H, int W, int h,
                                   int w, float* ws, float* loss, float* wmax, uint8_t* widx, float* wlast, void* stream) {
  WmseShape s;
  if (!fake || !label || !att || !ws || !loss || !wmax || !widx || !wmse_shape(B, C, T, H, W, h, w, &s)) return TGSR_EINVAL;
  const bool vec = s.w % 4 == 0 && aligned16(fake) && aligned16(label) && aligned16(att) && aligned16(wmax) && aligned16(wlast) &&
                   (reinterpret_cast<uintptr_t>(widx) & 3) == 0;
  const int nb = wmse_blocks(s);
  hipStream_t st = as_stream(stream);
  TGSR_WMSE_DISPATCH(weight_mse_fwd_kernel, fake, label, att, s, ws, wmax, widx, wlast);
  const int rc = note_launch(hipGetLastError(), "weight_mse_fwd_kernel");
  if (rc != TGSR_OK) return rc;
  const float n_elems = (float)((double)H * W * B * C);
  hipLaunchKernelGGL(weight_mse_finish_kernel, dim3(1), dim3(kALThreads), 0, st, ws, nb, n_elems, loss);
  return note_launch(hipGetLastError(), "weight_mse_finish_kernel");
}

extern "C" int tgsr_weight_mse_bwd(const float* grad, const float* fake, const float* label, const float* wmax, const uint8_t* widx,
                                   int B, int C, int T, int H, int W, int h, int w, float* d_fake, float* d_label, float* d_att,
                                   void* stream) {
  WmseShape s;
  if (!grad || !fake || !label || !wmax || !widx || (!d_fake && !d_label && !d_att) || !wmse_shape(B, C, T, H, W, h, w, &s))
    return TGSR_EINVAL;
  const bool vec = s.w % 4 == 0 && aligned16(fake) && aligned16(label) && aligned16(wmax) && aligned16(d_fake) && aligned16(d_label) &&
                   aligned16(d_att) && (reinterpret_cast<uintptr_t>(widx) & 3) == 0;
  const int nb = wmse_blocks(s);
  hipStream_t st = as_stream(stream);
  const double n_elems = (double)H * W * B * C;
  const float c_img = (float)(2.0 * T / n_elems), c_att = (float)((double)T / n_elems);
  TGSR_WMSE_DISPATCH(weight_mse_bwd_kernel, grad, fake, label, wmax, widx, s, c_img, c_att, d_fake, d_label, d_att);
  return note_launch(hipGetLastError(), "weight_mse_bwd_kernel");
}
