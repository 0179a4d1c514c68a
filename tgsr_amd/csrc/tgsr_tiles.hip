// Whole-image inference by overlapping tiles (SRPipeline.upscale; the reference's arbitrary-size example path,
// datasets.py:200-278 + the generators applied to the whole image): the two memory-bound ends of a tile batch.
//   tile_gather_kernel : windows [Tb][3][th][tw] float32 out of one planar image [3][H][W] (uint8: normalised with
//                        u8_normalize_kernel's arithmetic; float32: a bit copy), and out of a second image (the blurred LR)
//                        in the same launch.
//   tile_stitch_kernel : the rectangle each tile OWNS, out of tile outputs [Tb][C][s th][s tw] float32 into [C][s H][s W]
//                        (float32: a bit copy; uint8: tgsr_to_uint8's rule), for a short by-value list of outputs in one launch.
// The window table is int32 [Tb][6] = (y0, x0, oy0, oy1, ox0, ox1) in LR pixels: the window is rows [y0, y0 + th) x columns
// [x0, x0 + tw), the owned rectangle [oy0, oy1) x [ox0, ox1) lies inside it.  The host entry checks its copy of the table, the
// kernels skip a row of the device copy that fails the same checks: no access leaves an image whatever the table says.  Every
// output pixel has one source (the planner's owned rectangles partition the image): plain loads and stores, no atomics, the
// same bits on every run, capturable.
// Both are streaming passes: a thread moves 4 neighbouring pixels of a row, as one 16-byte access where the addresses allow
// (the image base, the row pitch and the rectangle's first column all multiples of 4 elements), element by element at the
// ragged ends of a row and wherever an image width or an owned column is odd.
#include "tgsr_common.h"

namespace tgsr {

constexpr int kTileDesc = 6;                 // int32 per window: y0 x0 oy0 oy1 ox0 ox1
constexpr int kTileMaxSide = 1 << 20;        // LR H, W (offsets are 64-bit; the caps keep the kernels' int32 products exact)
constexpr int kTileMaxTile = 4096;           // th, tw

__host__ __device__ inline bool tile_desc_ok(const int32_t* d, int H, int W, int th, int tw) {
  const int y0 = d[0], x0 = d[1], oy0 = d[2], oy1 = d[3], ox0 = d[4], ox1 = d[5];
  if (y0 < 0 || x0 < 0 || y0 > H - th || x0 > W - tw) return false;
  if (oy0 < y0 || oy1 <= oy0 || oy1 > y0 + th) return false;
  return !(ox0 < x0 || ox1 <= ox0 || ox1 > x0 + tw);
}

__device__ __forceinline__ float u8_norm(uint8_t v) {          // u8_normalize_kernel's arithmetic (tgsr_io.hip)
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.0f), 0.5f), 0.5f);
}

__device__ __forceinline__ uint8_t f32_to_u8(float v) {        // to_uint8_kernel's arithmetic (tgsr_misc.hip)
  const float t = __fmul_rn(__fadd_rn(v, 1.0f), 127.5f);
  return (uint8_t)(int)rintf(fminf(255.f, fmaxf(0.f, t)));
}

// blockIdx.y: window, blockIdx.z: which image (0: img -> out, 1: img2 -> out2).  Items of a window: (channel, row, group of
// 4 columns).  vec_out: out rows start on 16 bytes (tw % 4 == 0, aligned base); vec_in: so does every image row (W % 4 == 0,
// aligned base) - a window row then does where x0 % 4 == 0.
template <typename T>
__global__ __launch_bounds__(256) void tile_gather_kernel(const T* __restrict__ img, const T* __restrict__ img2, int H, int W,
                                                          const int32_t* __restrict__ table, int th, int tw,
                                                          float* __restrict__ out, float* __restrict__ out2, int vec_in,
                                                          int vec_out) {
  const int t = blockIdx.y;
  const int32_t* d = table + (int64_t)t * kTileDesc;
  if (!tile_desc_ok(d, H, W, th, tw)) return;                  // uniform over the workgroup
  const T* src = blockIdx.z ? img2 : img;
  float* dst = (blockIdx.z ? out2 : out) + (int64_t)t * 3 * th * tw;
  const int y0 = d[0], x0 = d[1];
  const int ng = (tw + 3) >> 2;
  const int items = 3 * th * ng;
  const bool vin = vec_in && (x0 & 3) == 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < items; i += gridDim.x * 256) {
    const int g = i % ng, y = (i / ng) % th, c = i / (ng * th);
    const int x = g * 4, n = min(4, tw - x);
    const T* p = src + ((int64_t)c * H + y0 + y) * W + x0 + x;
    float* q = dst + ((int64_t)c * th + y) * tw + x;
    if (n == 4 && vec_out) {
      float4 v;
      if constexpr (sizeof(T) == 1) {
        if (vin) {
          const uchar4 b = *reinterpret_cast<const uchar4*>(p);
          v = make_float4(u8_norm(b.x), u8_norm(b.y), u8_norm(b.z), u8_norm(b.w));
        } else {
          v = make_float4(u8_norm(p[0]), u8_norm(p[1]), u8_norm(p[2]), u8_norm(p[3]));
        }
      } else {
        v = vin ? *reinterpret_cast<const float4*>(p) : make_float4(p[0], p[1], p[2], p[3]);
      }
      *reinterpret_cast<float4*>(q) = v;
    } else {
      for (int k = 0; k < n; ++k) {
        if constexpr (sizeof(T) == 1) q[k] = u8_norm(p[k]);
        else q[k] = p[k];
      }
    }
  }
}

struct StitchList {                          // by value: one launch stitches every output of a tile batch
  const float* src[TGSR_STITCH_MAX];         // [Tb][C][s th][s tw], dense (C, s th, s tw) block, tile stride below
  void* dst[TGSR_STITCH_MAX];                // [C][s H][s W] float32 or uint8
  int64_t stride[TGSR_STITCH_MAX];           // elements between consecutive tiles of src
  int C[TGSR_STITCH_MAX];
  int s[TGSR_STITCH_MAX];
  int u8[TGSR_STITCH_MAX];                   // 0: float32 bit copy, 1: uint8 by tgsr_to_uint8's rule
  int vec_src[TGSR_STITCH_MAX];              // src base and tile stride on 16 bytes and (s tw) % 4 == 0
  int vec_dst[TGSR_STITCH_MAX];              // dst base on 16 (float32) / 4 (uint8) bytes and (s W) % 4 == 0
};

// blockIdx.y: window, blockIdx.z: entry of the list.  Items: (channel, owned row, group of 4 destination columns); with vec_dst
// the groups are the destination's aligned quads, so an owned rectangle that starts on an odd column has a partial first group.
__global__ __launch_bounds__(256) void tile_stitch_kernel(StitchList L, int H, int W, const int32_t* __restrict__ table, int th,
                                                          int tw) {
  const int t = blockIdx.y, e = blockIdx.z;
  const int32_t* d = table + (int64_t)t * kTileDesc;
  if (!tile_desc_ok(d, H, W, th, tw)) return;                  // uniform over the workgroup
  const int s = L.s[e], C = L.C[e];
  const bool u8 = L.u8[e] != 0, vdst = L.vec_dst[e] != 0;
  const int sy0 = s * d[0], sx0 = s * d[1];                    // the window's origin at this scale
  const int ya = s * d[2], yb = s * d[3], xa = s * d[4], xb = s * d[5];
  const int sth = s * th, stw = s * tw;
  const int64_t sH = (int64_t)s * H, sW = (int64_t)s * W;
  const int gx = vdst ? (xa & ~3) : xa;                        // first column of group 0
  const int ng = (xb - gx + 3) >> 2, rows = yb - ya;
  const int64_t items = (int64_t)C * rows * ng;
  const float* src = L.src[e] + (int64_t)t * L.stride[e];
  const bool vsrc = L.vec_src[e] != 0 && (sx0 & 3) == 0;       // then a destination quad is a source quad
  // one item: group g of owned row r of channel c
  auto move = [&](int g, int r, int c) {
    const int xs = gx + 4 * g;
    const int lo = max(xs, xa), hi = min(xs + 4, xb);
    const int y = ya + r;
    const float* p = src + ((int64_t)c * sth + (y - sy0)) * stw + (lo - sx0);
    const int64_t o = ((int64_t)c * sH + y) * sW + lo;
    if (vdst && hi - lo == 4) {
      const float4 v = vsrc ? *reinterpret_cast<const float4*>(p) : make_float4(p[0], p[1], p[2], p[3]);
      if (u8) {
        uchar4 b;
        b.x = f32_to_u8(v.x); b.y = f32_to_u8(v.y); b.z = f32_to_u8(v.z); b.w = f32_to_u8(v.w);
        *reinterpret_cast<uchar4*>(static_cast<uint8_t*>(L.dst[e]) + o) = b;
      } else {
        *reinterpret_cast<float4*>(static_cast<float*>(L.dst[e]) + o) = v;
      }
    } else {
      for (int k = 0; k < hi - lo; ++k) {
        if (u8) static_cast<uint8_t*>(L.dst[e])[o + k] = f32_to_u8(p[k]);
        else static_cast<float*>(L.dst[e])[o + k] = p[k];
      }
    }
  };
  // The item index splits into (c, r, g) by two divisions per item.  Every real window has far fewer than 2^31 items (an image
  // output of a 128 x 128 window at x8: 3 * 1024 * 256), so the loop runs on 32-bit unsigned divisions; the 64-bit form, an
  // emulated divide several times as long, is kept for what the entry's caps (C <= 65535, s th <= 2^18) still admit beyond that.
  const uint32_t step = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
  if (items <= (int64_t)0x7fffffff - step) {                    // uniform over the workgroup; i + step cannot wrap
    const uint32_t n = (uint32_t)items, ung = (uint32_t)ng, urows = (uint32_t)rows;
    for (uint32_t i = first; i < n; i += step) {
      const uint32_t line = i / ung;
      move((int)(i - line * ung), (int)(line % urows), (int)(line / urows));
    }
  } else {
    for (int64_t i = first; i < items; i += step) {
      const int64_t line = i / ng;
      move((int)(i - line * ng), (int)(line % rows), (int)(line / rows));
    }
  }
}

static inline bool tile_args_ok(int H, int W, const int32_t* table_host, const int32_t* table_dev, int Tb, int th, int tw) {
  if (!table_host || !table_dev || Tb < 1 || Tb > 65535) return false;
  if (H < 1 || W < 1 || H > kTileMaxSide || W > kTileMaxSide || th < 1 || tw < 1 || th > H || tw > W ||
      th > kTileMaxTile || tw > kTileMaxTile)
    return false;
  for (int t = 0; t < Tb; ++t)
    if (!tile_desc_ok(table_host + (int64_t)t * kTileDesc, H, W, th, tw)) return false;
  return true;
}

static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace tgsr

using namespace tgsr;

extern "C" int tgsr_tile_gather(const void* img, const void* img2, int is_u8, int H, int W, const int32_t* table_host,
                                const int32_t* table_dev, int Tb, int th, int tw, float* out, float* out2, void* stream) {
  if (!img || !out || (img2 != nullptr) != (out2 != nullptr)) return TGSR_EINVAL;
  if (!tile_args_ok(H, W, table_host, table_dev, Tb, th, tw)) return TGSR_EINVAL;
  const uintptr_t in_align = is_u8 ? 4 : 16;
  const int vec_in = (W % 4 == 0) && aligned_to(img, in_align) && (!img2 || aligned_to(img2, in_align));
  const int vec_out = (tw % 4 == 0) && aligned_to(out, 16) && (!out2 || aligned_to(out2, 16));
  const int items = 3 * th * ((tw + 3) / 4);
  const dim3 grid((unsigned)((items + 255) / 256 < 64 ? (items + 255) / 256 : 64), (unsigned)Tb, img2 ? 2u : 1u);
  if (is_u8)
    hipLaunchKernelGGL(tile_gather_kernel<uint8_t>, grid, dim3(256), 0, as_stream(stream), static_cast<const uint8_t*>(img),
                       static_cast<const uint8_t*>(img2), H, W, table_dev, th, tw, out, out2, vec_in, vec_out);
  else
    hipLaunchKernelGGL(tile_gather_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(img),
                       static_cast<const float*>(img2), H, W, table_dev, th, tw, out, out2, vec_in, vec_out);
  return note_launch(hipGetLastError(), "tile_gather_kernel");
}

extern "C" int tgsr_tile_stitch(int n, const float* const* src, const int64_t* src_stride, void* const* dst, const int* C,
                                const int* scale, const int* out_u8, int H, int W, const int32_t* table_host,
                                const int32_t* table_dev, int Tb, int th, int tw, void* stream) {
  if (n < 1 || n > TGSR_STITCH_MAX || !src || !src_stride || !dst || !C || !scale || !out_u8) return TGSR_EINVAL;
  if (!tile_args_ok(H, W, table_host, table_dev, Tb, th, tw)) return TGSR_EINVAL;
  StitchList L = {};
  int64_t most = 0;
  for (int e = 0; e < n; ++e) {
    const int s = scale[e];
    if (!src[e] || !dst[e] || C[e] < 1 || C[e] > 65535 || s < 1 || s > 64) return TGSR_EINVAL;
    const int64_t block = (int64_t)C[e] * s * th * s * tw;
    if (src_stride[e] < block && Tb > 1) return TGSR_EINVAL;
    L.src[e] = src[e];
    L.dst[e] = dst[e];
    L.stride[e] = src_stride[e];
    L.C[e] = C[e];
    L.s[e] = s;
    L.u8[e] = out_u8[e] ? 1 : 0;
    L.vec_src[e] = ((int64_t)s * tw) % 4 == 0 && aligned_to(src[e], 16) && src_stride[e] % 4 == 0;
    L.vec_dst[e] = ((int64_t)s * W) % 4 == 0 && aligned_to(dst[e], out_u8[e] ? 4 : 16);
    const int64_t items = (int64_t)C[e] * s * th * ((s * tw + 3) / 4 + 1);
    most = items > most ? items : most;
  }
  const int64_t gx = (most + 255) / 256;
  const dim3 grid((unsigned)(gx < 256 ? gx : 256), (unsigned)Tb, (unsigned)n);
  hipLaunchKernelGGL(tile_stitch_kernel, grid, dim3(256), 0, as_stream(stream), L, H, W, table_dev, th, tw);
  return note_launch(hipGetLastError(), "tile_stitch_kernel");
}
