// Attention panels for gfx950: which word steered which region (tgsr_amd/attnviz.py states the arithmetic).
//
// Per caption word the reference (miscc/utils.py:389-416) thresholds the word's attention map, expands it to the panel tile
// (linear interpolation, then a sigma = 20 Gaussian of 161 taps per axis in fp64), stretches it to [0, 255], truncates to bytes and
// pastes it over the SR image through a constant mask.  Resize and blur are linear and separable: the tile is M_h . X . M_w^T with
// the (V x a) resize-then-blur operators M built once on the host in fp64 (attnviz.expand_operator).
//
// attn_expand_kernel  one workgroup per (map, block of kAR = 16 tile rows): the map thresholded in LDS as fp32 (widened on read:
//     exact), conf = sum x [x > 2 thresh] in a fixed order (row block 0), Z = M_h[rows] . X and Y = Z . M_w^T on
//     v_mfma_f64_16x16x4_f64 (C/D: col = lane & 15, row = (lane >> 4) + 4 reg - NOT the f32 map), Y to the fp64 workspace, the
//     block's min / max beside it.  u = 1 runs the same kernel with M = I: every product is x * 1 + zeros, exact.
//     fp64 is a requirement: max - min is 0.004 at an 8 x 8 map of 5 words, and a truncation follows.
// attn_panel_kernel   one workgroup per (image, kPR = 2 panel rows): per word the block minima / maxima in block order, the word's
//     slot = the number of words that beat it in conf (counted, as retrieval_ranks_kernel counts; ties: the higher word index
//     first), then every byte of its rows - normalise, truncate, quantise the image pixel, Pillow's paste arithmetic, black
//     separators and right padding - with 16-byte stores where the address is aligned, single bytes at the two ends of its range.
//     Optionally the un-blended map bytes [B][T][Vh][Vw] the same way.
// No atomics, no host synchronisation, plain stores: capturable, the same bits on every run.
#include "tgsr_common.h"

#include <cmath>

namespace tgsr {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kAR = 16;      // tile rows per workgroup of attn_expand_kernel: one f64 MFMA tile
constexpr int kAT = 64;      // most words of a caption
constexpr int kPR = 2;       // panel rows per workgroup of attn_panel_kernel (8: 442 us at the shipped shape, 2: 372 us)
constexpr int kAMaxA = 128;  // largest side of an attention map
constexpr int kAMaxV = 512;  // largest side of a panel tile

struct AttnShape {
  int hp, wp, xp, mp, zp;    // h rounded up to 4, w rounded up to 16, pitches of the three LDS images
  size_t lds;
};

// LDS at h = w = 128: X 128 x 144 fp32 = 73 728 B, the M_h slice 16 x 132 fp64 = 16 896 B, Z 16 x 132 fp64 = 16 896 B, + 8 doubles
// = 107 584 B of the 160 KiB.  M_w (up to 512 x 128 fp64) is read from global memory: every workgroup of a launch reads the same.
static AttnShape attn_shape(int h, int w) {
  AttnShape s;
  s.hp = (h + 3) & ~3;
  s.wp = (w + 15) & ~15;
  s.xp = s.wp | 16;          // pitch % 32 == 16: the two k rows a 32-lane group reads fall on different banks
  s.mp = s.hp + 4;
  s.zp = s.wp + 4;
  const int zs = kAR * s.zp > 256 ? kAR * s.zp : 256;           // Z doubles as the conf reduction's 256 partial sums
  s.lds = sizeof(float) * (size_t)s.hp * s.xp + sizeof(double) * ((size_t)kAR * s.mp + zs + 8);
  return s;
}

struct ExpandArgs {
  const float* att;          // [B][T][h][w]
  const int32_t* lens;       // [B]
  const double* Mh;          // [Vh][h]
  const double* Mw;          // [Vw][w]
  int T, h, w, Vh, Vw, nblk;
  int hp, wp, xp, mp, zp;
  double* tile;              // [B T][Vh][Vw]
  double* mm;                // [B T][nblk][2]
  double* conf;              // [B][T]
};

__device__ __forceinline__ int clamp_len(int n, int T) { return n < 1 ? 1 : (n > T ? T : n); }

__global__ __launch_bounds__(256) void attn_expand_kernel(ExpandArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* mhs = lds_d;                                             // [kAR][mp]
  double* zs = mhs + kAR * a.mp;                                   // [kAR][zp], >= 256 doubles
  double* red = zs + (kAR * a.zp > 256 ? kAR * a.zp : 256);        // [4 waves][2]
  float* xs = reinterpret_cast<float*>(red + 8);                   // [hp][xp]

  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int map = blockIdx.x / a.nblk, blk = blockIdx.x - map * a.nblk;
  const int b = map / a.T, j = map - b * a.T;
  const int n = clamp_len(a.lens[b], a.T);
  if (j >= n) {                                                    // uniform: a word behind the caption has no map
    if (blk == 0 && tid == 0) a.conf[map] = 0.0;
    return;
  }
  const double thresh = 2.0 / (double)n;                           // utils.py:379
  const int h = a.h, w = a.w, hp = a.hp, wp = a.wp, xp = a.xp, mp = a.mp, zp = a.zp;
  const float* src = a.att + (int64_t)map * h * w;

  double part = 0.0;
  for (int o = tid; o < hp * wp; o += 256) {
    const int r = o / wp, c = o - r * wp;
    const float v = (r < h && c < w) ? src[r * w + c] : 0.f;
    const double x = (double)v;
    if (x > 2.0 * thresh) part = __dadd_rn(part, x);               // utils.py:391-392
    xs[r * xp + c] = x > thresh ? v : 0.f;                         // utils.py:393-394
  }
  for (int o = tid; o < kAR * hp; o += 256) {
    const int r = o / hp, k = o - r * hp;
    const int row = blk * kAR + r;
    mhs[r * mp + k] = (row < a.Vh && k < h) ? a.Mh[(int64_t)row * h + k] : 0.0;
  }
  if (blk == 0) {                                                  // uniform per workgroup
    zs[tid] = part;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if (tid < s) zs[tid] = __dadd_rn(zs[tid], zs[tid + s]);
      __syncthreads();
    }
    if (tid == 0) a.conf[map] = zs[0];
  }
  __syncthreads();

  // ---- Z = M_h[rows] . X: [16][wp], k over the map's rows
  for (int nt = wave; nt < (wp >> 4); nt += 4) {
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < hp; k0 += 4) {
      const double av = mhs[l15 * mp + k0 + lq];                   // A[row l15][k = lq]
      const double bv = (double)xs[(k0 + lq) * xp + nt * 16 + l15];   // B[k = lq][col l15]
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) zs[(lq + 4 * r) * zp + nt * 16 + l15] = acc[r];
  }
  __syncthreads();

  // ---- Y = Z . M_w^T: [16][Vw], k over the map's columns (columns of Z at and behind w are exact zeros)
  double mn = INFINITY, mx = -INFINITY;
  double* dst = a.tile + (int64_t)map * a.Vh * a.Vw;
  const int w4 = (w + 3) & ~3;
  for (int nt = wave; nt < ((a.Vw + 15) >> 4); nt += 4) {
    const int col = nt * 16 + l15;
    const bool cok = col < a.Vw;
    const double* mw = a.Mw + (int64_t)(cok ? col : 0) * w;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < w4; k0 += 4) {
      const int k = k0 + lq;
      const double av = zs[l15 * zp + k];
      const double bv = (cok && k < w) ? mw[k] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = blk * kAR + lq + 4 * r;
      if (cok && row < a.Vh) {
        dst[(int64_t)row * a.Vw + col] = acc[r];
        mn = fmin(mn, acc[r]);
        mx = fmax(mx, acc[r]);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, o));
    mx = fmax(mx, __shfl_xor(mx, o));
  }
  if (lane == 0) {
    red[wave * 2] = mn;
    red[wave * 2 + 1] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    double* p = a.mm + ((int64_t)map * a.nblk + blk) * 2;
    p[0] = fmin(fmin(red[0], red[2]), fmin(red[4], red[6]));
    p[1] = fmax(fmax(red[1], red[3]), fmax(red[5], red[7]));
  }
}

struct PanelArgs {
  const double* tile;        // [B T][Vh][Vw]
  const double* mm;          // [B T][nblk][2]
  const double* conf;        // [B][T]
  const int32_t* lens;       // [B]
  const void* img;           // [B][3][Vh][Vw] fp32 in [-1, 1] or uint8
  int img_f32;
  int B, T, Vh, Vw, nblk, K, by_conf, alpha;
  uint8_t* panel;            // [B][Vh][K (Vw + 2)][3]
  uint8_t* maps;             // [B][T][Vh][Vw] or null
  int32_t* order;            // [B][T]
};

// utils.py:398-400, 406, 411: ((x - min) / (max - min)) * 255 in fp64, truncated.  max == min (the reference's 0 / 0) is black.
__device__ __forceinline__ unsigned map_byte(const double* __restrict__ t, int64_t at, double mn, double rg) {
  if (!(rg > 0.0)) return 0u;
  const double y = __dmul_rn(__ddiv_rn(__dadd_rn(t[at], -mn), rg), 255.0);
  return (unsigned)(int)y;
}

// utils.py:341-343: fp32 ((v + 1) / 2) * 255, round half to even, clamp.
__device__ __forceinline__ unsigned img_byte(const void* __restrict__ img, int f32, int64_t at) {
  if (!f32) return static_cast<const uint8_t*>(img)[at];
  float v = __fmul_rn(__fdiv_rn(__fadd_rn(static_cast<const float*>(img)[at], 1.f), 2.f), 255.f);
  v = fminf(fmaxf(rintf(v), 0.f), 255.f);
  return (unsigned)(int)v;
}

// `len` <= 16 bytes into dst: one 16-byte store when len == 16 (the caller aligned dst), single bytes otherwise
__device__ __forceinline__ void put_bytes(uint8_t* dst, const unsigned (&wd)[4], int len) {
  if (len == 16) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < len) dst[i] = (uint8_t)(wd[i >> 2] >> (8 * (i & 3)));
  }
}

__global__ __launch_bounds__(256) void attn_panel_kernel(PanelArgs a) {
  __shared__ int s_word[kAT];        // the word shown in slot s, -1 = none
  __shared__ double s_mn[kAT], s_rg[kAT];
  const int tid = threadIdx.x;
  const int nrc = (a.Vh + kPR - 1) / kPR;
  const int b = blockIdx.x / nrc, rc = blockIdx.x - b * nrc;
  const int T = a.T, Vh = a.Vh, Vw = a.Vw, K = a.K;
  const int n = clamp_len(a.lens[b], T);
  const int Kb = K < n ? K : n;
  if (tid < kAT) s_word[tid] = -1;
  __syncthreads();
  if (tid < n) {
    const double* cf = a.conf + (int64_t)b * T;
    int slot = tid;
    if (a.by_conf) {
      const double cj = cf[tid];
      slot = 0;
      for (int i = 0; i < n; ++i) {
        const double ci = cf[i];
        slot += (ci > cj || (ci == cj && i > tid)) ? 1 : 0;
      }
    }
    s_word[slot] = tid;
    const double* p = a.mm + ((int64_t)b * T + tid) * a.nblk * 2;
    double mn = p[0], mx = p[1];
    for (int q = 1; q < a.nblk; ++q) {
      mn = fmin(mn, p[2 * q]);
      mx = fmax(mx, p[2 * q + 1]);
    }
    s_mn[tid] = mn;
    s_rg[tid] = __dadd_rn(mx, -mn);
  }
  __syncthreads();
  if (rc == 0 && tid < T) a.order[(int64_t)b * T + tid] = tid < n ? s_word[tid] : -1;

  const int y0 = rc * kPR, y1 = y0 + kPR < Vh ? y0 + kPR : Vh;
  const int cell = Vw + 2;
  const int64_t plane = (int64_t)Vh * Vw;

  {  // ---- the panel rows [y0, y1) of image b: one contiguous byte range
    const int64_t Wb = (int64_t)K * cell * 3;
    uint8_t* base = a.panel + (int64_t)b * Vh * Wb;
    const int64_t r0 = y0 * Wb, r1 = y1 * Wb;
    int64_t head = (16 - (int64_t)(reinterpret_cast<uintptr_t>(base + r0) & 15)) & 15;
    if (head > r1 - r0) head = r1 - r0;
    const int64_t nbody = (r1 - r0 - head) >> 4;
    const int64_t tail = r1 - r0 - head - nbody * 16;
    for (int64_t q = tid; q < nbody + 2; q += 256) {
      int64_t rel;
      int len;
      if (q < nbody) { rel = r0 + head + q * 16; len = 16; }
      else if (q == nbody) { rel = r0; len = (int)head; }
      else { rel = r1 - tail; len = (int)tail; }
      if (len == 0) continue;
      int y = (int)(rel / Wb);
      const int rem = (int)(rel - y * Wb);
      int px = rem / 3, c = rem - px * 3;
      int k = px / cell, xin = px - k * cell;
      unsigned wd[4] = {0u, 0u, 0u, 0u};
      int m = -1;                                                  // map byte of the current pixel: -1 unknown, 256 black
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i < len) {
          if (m < 0) {
            const int j = k < Kb ? s_word[k] : -1;
            m = (j >= 0 && xin < Vw) ? (int)map_byte(a.tile + ((int64_t)b * T + j) * plane, (int64_t)y * Vw + xin, s_mn[j], s_rg[j])
                                     : 256;
          }
          if (m != 256) {
            const unsigned iv = img_byte(a.img, a.img_f32, ((int64_t)b * 3 + c) * plane + (int64_t)y * Vw + xin);
            const unsigned t = (unsigned)m * (unsigned)a.alpha + iv * (unsigned)(255 - a.alpha) + 128u;   // Pillow's paste
            wd[i >> 2] |= ((((t >> 8) + t) >> 8) & 255u) << (8 * (i & 3));
          }
          if (++c == 3) {
            c = 0;
            m = -1;
            if (++xin == cell) {
              xin = 0;
              if (++k == K) { k = 0; ++y; }
            }
          }
        }
      }
      put_bytes(base + rel, wd, len);
    }
  }

  if (a.maps) {  // ---- the un-blended map bytes: rows [y0, y1) of every word's plane, black behind the caption
    const int64_t span = (int64_t)(y1 - y0) * Vw;
    for (int j = 0; j < T; ++j) {
      uint8_t* base = a.maps + ((int64_t)b * T + j) * plane;
      const double* t = a.tile + ((int64_t)b * T + j) * plane;
      const int64_t r0 = (int64_t)y0 * Vw, r1 = r0 + span;
      int64_t head = (16 - (int64_t)(reinterpret_cast<uintptr_t>(base + r0) & 15)) & 15;
      if (head > span) head = span;
      const int64_t nbody = (span - head) >> 4;
      const int64_t tail = span - head - nbody * 16;
      const bool live = j < n;
      const double mn = live ? s_mn[j] : 0.0, rg = live ? s_rg[j] : 0.0;
      for (int64_t q = tid; q < nbody + 2; q += 256) {
        int64_t rel;
        int len;
        if (q < nbody) { rel = r0 + head + q * 16; len = 16; }
        else if (q == nbody) { rel = r0; len = (int)head; }
        else { rel = r1 - tail; len = (int)tail; }
        if (len == 0) continue;
        unsigned wd[4] = {0u, 0u, 0u, 0u};
        if (live) {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (i < len) wd[i >> 2] |= map_byte(t, rel + i, mn, rg) << (8 * (i & 3));
        }
        put_bytes(base + rel, wd, len);
      }
    }
  }
}

static bool attn_shape_ok(int B, int T, int h, int w, int u) {
  if (B < 1 || T < 1 || u < 1) return false;
  if (h < 2 || w < 2 || h > kAMaxA || w > kAMaxA || T > kAT) return false;
  return (int64_t)u * h <= kAMaxV && (int64_t)u * w <= kAMaxV;
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int64_t tgsr_attn_panels_ws_elems(int B, int T, int h, int w, int u) {
  if (!attn_shape_ok(B, T, h, w, u)) return 0;
  const int Vh = u * h, Vw = u * w;
  return (int64_t)B * T * ((int64_t)Vh * Vw + 2 * ((Vh + kAR - 1) / kAR));
}

extern "C" int tgsr_attn_panels(const float* att, const int32_t* cap_lens, const void* img, int img_f32, const double* Mh,
                                const double* Mw, int B, int T, int h, int w, int u, int alpha, int K, int by_conf, double* ws,
                                uint8_t* panel, uint8_t* maps_or_null, double* conf, int32_t* order, void* stream) {
  if (!att || !cap_lens || !img || !Mh || !Mw || !ws || !panel || !conf || !order) return TGSR_EINVAL;
  if (B < 1 || T < 1 || K < 1 || K > T || u < 1 || alpha < 0 || alpha > 255) return TGSR_EINVAL;
  if (!attn_shape_ok(B, T, h, w, u)) return TGSR_EUNSUPPORTED;
  const auto low = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  if ((low(att) | low(cap_lens) | low(order) | (img_f32 ? low(img) : 0)) & 3) return TGSR_EUNSUPPORTED;   // 4-byte elements
  if ((low(Mh) | low(Mw) | low(ws) | low(conf)) & 7) return TGSR_EUNSUPPORTED;                              // fp64
  const int Vh = u * h, Vw = u * w;
  const int nblk = (Vh + kAR - 1) / kAR, nrc = (Vh + kPR - 1) / kPR;
  if ((int64_t)B * T * nblk > 0x7fffffffLL || (int64_t)B * nrc > 0x7fffffffLL) return TGSR_EUNSUPPORTED;
  const AttnShape s = attn_shape(h, w);
  static bool attr_set[64] = {false};   // > 64 KB of dynamic LDS needs the opt-in once per DEVICE (see tgsr_damsm.hip)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!attr_set[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_expand_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return note_launch(e, "hipFuncSetAttribute(attn_expand_kernel)");
    }
    attr_set[dev] = true;
  }
  ExpandArgs e;
  e.att = att; e.lens = cap_lens; e.Mh = Mh; e.Mw = Mw; e.T = T; e.h = h; e.w = w; e.Vh = Vh; e.Vw = Vw; e.nblk = nblk;
  e.hp = s.hp; e.wp = s.wp; e.xp = s.xp; e.mp = s.mp; e.zp = s.zp;
  e.tile = ws; e.mm = ws + (int64_t)B * T * Vh * Vw; e.conf = conf;
  hipLaunchKernelGGL(attn_expand_kernel, dim3((unsigned)((int64_t)B * T * nblk)), dim3(256), s.lds, as_stream(stream), e);
  const int rc = note_launch(hipGetLastError(), "attn_expand_kernel");
  if (rc != TGSR_OK) return rc;
  PanelArgs p;
  p.tile = e.tile; p.mm = e.mm; p.conf = conf; p.lens = cap_lens; p.img = img; p.img_f32 = img_f32; p.B = B; p.T = T; p.Vh = Vh;
  p.Vw = Vw; p.nblk = nblk; p.K = K; p.by_conf = by_conf; p.alpha = alpha; p.panel = panel; p.maps = maps_or_null; p.order = order;
  hipLaunchKernelGGL(attn_panel_kernel, dim3((unsigned)((int64_t)B * nrc)), dim3(256), 0, as_stream(stream), p);
  return note_launch(hipGetLastError(), "attn_panel_kernel");
}
