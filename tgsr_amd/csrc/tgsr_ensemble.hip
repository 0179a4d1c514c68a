// Geometric self-ensemble (x8, the "+" variant of an SR model; SRPipeline.upscale(ensemble=8), SRPipeline.self_ensemble): the
// two ends of a variant batch that touch pixels.
//   d8_gather_kernel : the nk variants of every window of N planar images [N][3][H][W] (uint8: normalised with
//                      u8_normalize_kernel's arithmetic; float32: a bit copy) as float32 [N][Tb][nk][3][th'][tw'], and of a second
//                      image (the blurred LR) in the same launch.
//   d8_merge_kernel  : the rectangle each window OWNS of the mean of the eight variant outputs, each mapped back, into
//                      [N][C][s H][s W] (float32, or uint8 by tgsr_to_uint8's rule on the float32 mean), for a short by-value
//                      list of outputs in one launch.
// The transform (include/tgsr_hip.h, tgsr_amd/tiles.py): variant k = 0..7 has bits b0 = k & 1 (mirror the columns), b1 = k & 2
// (mirror the rows), b2 = k & 4 (transpose, applied first).  For a window of h x w, variant k has shape (h', w') = b2 ? (w, h) :
// (h, w) and its pixel (i, j) is win[y][x] with i' = b1 ? h' - 1 - i : i, j' = b0 ? w' - 1 - j : j, (y, x) = b2 ? (j', i') :
// (i', j').  Hence the pixel (y, x) of the window lies in variant k at
//   b2 = 0:  i = b1 ? h - 1 - y : y,   j = b0 ? w - 1 - x : x            ([h][w] image)
//   b2 = 1:  i = b1 ? w - 1 - x : x,   j = b0 ? h - 1 - y : y            ([w][h] image)
// so a kBlk x kBlk block of the window at (y_lo, x_lo) is, in every variant, a kBlk x kBlk block whose first row r0 and first
// column c0 are the expressions above at the block's first or last pixel (d8_block).  The mean is
// ((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125f in float32, one rounding per operation, in ascending k.
//
// Layout.  Both kernels are memory-bound.  A workgroup of 256 threads owns one kBlk x kBlk block of one channel on the window's
// side (the gather's source, the merge's destination).  Every global access runs along rows: a block of a variant is read (merge)
// or written (gather) row by row in ascending addresses, as the aligned 16-byte quads that cover its kBlk columns - kBlk / 4 + 1
// of them from any first column - where the base, the row pitch and the plane size are multiples of 4 elements, element by element
// otherwise (any H, W, offsets).  The mirrors and the transpose happen between LDS and registers: a block is kept in LDS as
// [kBlk][kPitch] floats, kPitch = 4 (kBlk / 4 + 1) + 1 = 37 - odd, so the 32 lanes of a ds_read_b32 group (4 rows x 8 quads of
// the thread map below) fall on 32 different banks both for a row walk (bank 5 r + 4 q + e) and for a column walk
// (bank 20 q + r + 5 e: 20 q mod 32 runs over the multiples of 4).  The merge holds the blocks of all eight variants at once
// (8 x 32 x 37 x 4 = 37 888 bytes and 122 registers: four workgroups per CU), filled through registers, three 16-byte loads of a
// thread in flight before the first of them is stored (measured against one, five and nine: DESIGN.md 3.15), one barrier, and
// each thread sums its 4 neighbouring destination pixels in registers in k order.  Plain vector loads and stores, no atomics, no
// workspace: the same bits on every run, capturable.
// (The window table, its checks and the two pixel conversions repeat tgsr_tiles.hip's, which stays as it is.)
#include "tgsr_common.h"

namespace tgsr {

constexpr int kTileDesc = 6;                 // int32 per window: y0 x0 oy0 oy1 ox0 ox1
constexpr int kTileMaxSide = 1 << 20;        // LR H, W
constexpr int kTileMaxTile = 4096;           // th, tw
constexpr int kD8MaxN = 4096;                // images per launch (blockIdx.z = entry * N + image)

constexpr int kBlk = 32;                     // a workgroup's block (measured against 64: DESIGN.md 3.15)
constexpr int kQuads = kBlk / 4 + 1;         // aligned quads that cover kBlk columns from any first column
constexpr int kPitch = 4 * kQuads + 1;       // floats per LDS row
constexpr int kPass = kBlk == 32 ? 8 : 2;    // variants held in LDS at once (64 KiB of static LDS at most)
constexpr int kRowQuads = kBlk / 4;          // the thread map of a block: (row, quad) = (tid / kRowQuads, tid % kRowQuads) ...
constexpr int kSweepRows = 256 / kRowQuads;  // ... over kSweeps sweeps of kSweepRows rows
constexpr int kSweeps = kBlk / kSweepRows;
constexpr int kLoads = (kPass * kBlk * kQuads + 255) / 256;    // quads a thread of the merge loads per pass ...
constexpr int kChunk = 3;                                      // ... of which so many are in flight at once

__host__ __device__ inline bool d8_desc_ok(const int32_t* d, int H, int W, int th, int tw) {
  const int y0 = d[0], x0 = d[1], oy0 = d[2], oy1 = d[3], ox0 = d[4], ox1 = d[5];
  if (y0 < 0 || x0 < 0 || y0 > H - th || x0 > W - tw) return false;
  if (oy0 < y0 || oy1 <= oy0 || oy1 > y0 + th) return false;
  return !(ox0 < x0 || ox1 <= ox0 || ox1 > x0 + tw);
}

__device__ __forceinline__ float d8_u8_norm(uint8_t v) {       // u8_normalize_kernel's arithmetic (tgsr_io.hip)
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.0f), 0.5f), 0.5f);
}

__device__ __forceinline__ uint8_t d8_f32_to_u8(float v) {     // to_uint8_kernel's arithmetic (tgsr_misc.hip)
  const float t = __fmul_rn(__fadd_rn(v, 1.0f), 127.5f);
  return (uint8_t)(int)rintf(fminf(255.f, fmaxf(0.f, t)));
}

// The block of variant k that holds the block (y_lo, x_lo) of an h x w window: first row r0, first column c0 (either may be
// negative or reach past the image where the window's block does), the variant's rows and columns.
struct D8Block {
  int r0, c0, rows, cols;
};

__device__ __forceinline__ D8Block d8_block(int k, int h, int w, int y_lo, int x_lo) {
  D8Block b;
  if (k & 4) {
    b.r0 = (k & 2) ? w - kBlk - x_lo : x_lo;
    b.c0 = (k & 1) ? h - kBlk - y_lo : y_lo;
    b.rows = w;
    b.cols = h;
  } else {
    b.r0 = (k & 2) ? h - kBlk - y_lo : y_lo;
    b.c0 = (k & 1) ? w - kBlk - x_lo : x_lo;
    b.rows = h;
    b.cols = w;
  }
  return b;
}

// (ry, rx) inside the window's block -> (ti, tj) inside the variant's block, and back.
__device__ __forceinline__ void d8_to_variant(int k, int ry, int rx, int& ti, int& tj) {
  const int p = (k & 4) ? rx : ry, q = (k & 4) ? ry : rx;
  ti = (k & 2) ? kBlk - 1 - p : p;
  tj = (k & 1) ? kBlk - 1 - q : q;
}

__device__ __forceinline__ void d8_to_window(int k, int ti, int tj, int& ry, int& rx) {
  const int p = (k & 2) ? kBlk - 1 - ti : ti, q = (k & 1) ? kBlk - 1 - tj : tj;
  ry = (k & 4) ? q : p;
  rx = (k & 4) ? p : q;
}

// One aligned quad of a block on its way into LDS, in two halves so that a thread can have all its loads in flight before it
// stores the first: row `tr` of the block, quad `q` of that row.  plane: the [rows][cols] image the block lies in; the quad's
// columns are cq .. cq + 3 with cq = (c0 & ~3) + 4 q (a floor: c0 may be negative), kept at tile[tr][4 q ..].  Elements outside
// the image are not loaded (they are kept as zeros) - no pixel that is written depends on them.
template <typename T>
__device__ __forceinline__ float4 d8_fetch_quad(const T* __restrict__ plane, int rows, int cols, int r0, int c0, int tr, int q,
                                                bool vec) {
  const int r = r0 + tr, cq = (c0 & ~3) + 4 * q;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r < 0 || r >= rows || cq + 3 < 0 || cq >= cols) return v;
  const T* p = plane + (int64_t)r * cols + cq;
  if (vec && cq + 4 <= cols) {                                 // cq is a multiple of 4 and > -4 here: not negative
    if constexpr (sizeof(T) == 1) {
      const uchar4 b = *reinterpret_cast<const uchar4*>(p);
      v = make_float4(d8_u8_norm(b.x), d8_u8_norm(b.y), d8_u8_norm(b.z), d8_u8_norm(b.w));
    } else {
      v = *reinterpret_cast<const float4*>(p);
    }
  } else {
    float e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      e[i] = 0.f;
      if (cq + i >= 0 && cq + i < cols) {
        if constexpr (sizeof(T) == 1) e[i] = d8_u8_norm(p[i]);
        else e[i] = p[i];
      }
    }
    v = make_float4(e[0], e[1], e[2], e[3]);
  }
  return v;
}

__device__ __forceinline__ void d8_keep_quad(float4 v, int tr, int q, float* __restrict__ tile) {
  float* t = tile + tr * kPitch + 4 * q;
  t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
}

// blockIdx.x: blocks of the window x channel (a stride loop), blockIdx.y: window, blockIdx.z: 2 * image + which source
// (0: img -> out, 1: img2 -> out2).  vec_in: every image row starts on 16 bytes (4 for uint8); vec_out: so does every row of
// every variant (th % 4 == 0 and tw % 4 == 0, aligned base).
template <typename T>
__global__ __launch_bounds__(256) void d8_gather_kernel(const T* __restrict__ img, const T* __restrict__ img2, int H, int W,
                                                        const int32_t* __restrict__ table, int Tb, int th, int tw, int k0, int nk,
                                                        float* __restrict__ out, float* __restrict__ out2, int two, int vec_in,
                                                        int vec_out) {
  __shared__ float tile[kBlk * kPitch];
  const int t = blockIdx.y, n = two ? blockIdx.z >> 1 : blockIdx.z, which = two ? blockIdx.z & 1 : 0;
  const int32_t* d = table + (int64_t)t * kTileDesc;
  if (!d8_desc_ok(d, H, W, th, tw)) return;                    // uniform over the workgroup
  const T* src = (which ? img2 : img) + (int64_t)n * 3 * H * W;
  float* dst = (which ? out2 : out) + ((int64_t)n * Tb + t) * nk * 3 * th * tw;
  const int y0 = d[0], x0 = d[1];
  const int nbx = (tw + kBlk - 1) / kBlk, nby = (th + kBlk - 1) / kBlk;
  const int tid = threadIdx.x;
  for (int blk = blockIdx.x; blk < 3 * nby * nbx; blk += gridDim.x) {
    const int bx = blk % nbx, by = (blk / nbx) % nby, c = blk / (nbx * nby);
    const int y_lo = by * kBlk, x_lo = bx * kBlk;
    __syncthreads();                                           // the previous block's readers are done with the tile
    // the window's block, rows y0 + y_lo + [0, kBlk) x the quads that cover columns x0 + x_lo + [0, kBlk) of the image
    for (int it = tid; it < kBlk * kQuads; it += 256)
      d8_keep_quad(d8_fetch_quad<T>(src + (int64_t)c * H * W, H, W, y0 + y_lo, x0 + x_lo, it / kQuads, it % kQuads, vec_in != 0),
                   it / kQuads, it % kQuads, tile);
    __syncthreads();
    const int off = (x0 + x_lo) & 3;                           // the block's first column inside its first quad
    for (int kk = 0; kk < nk; ++kk) {
      const int k = k0 + kk;
      const D8Block b = d8_block(k, th, tw, y_lo, x_lo);
      float* vo = dst + ((int64_t)kk * 3 + c) * th * tw;       // the variant's [rows][cols] plane
      const bool vst = vec_out && (b.c0 & 3) == 0;
#pragma unroll
      for (int sw = 0; sw < kSweeps; ++sw) {
        const int ti = sw * kSweepRows + tid / kRowQuads, q = tid % kRowQuads;
        const int i = b.r0 + ti, j = b.c0 + 4 * q;
        if (i < 0 || i >= b.rows) continue;
        float v[4];
        bool ok[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int ry, rx;
          d8_to_window(k, ti, 4 * q + e, ry, rx);
          ok[e] = j + e >= 0 && j + e < b.cols && y_lo + ry < th && x_lo + rx < tw;
          v[e] = ok[e] ? tile[ry * kPitch + rx + off] : 0.f;
        }
        float* p = vo + (int64_t)i * b.cols + j;
        if (vst && ok[0] && ok[3]) {
          *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (ok[e]) p[e] = v[e];
        }
      }
    }
  }
}

struct MergeList {                           // by value: one launch merges every output of a variant batch
  const float* srcA[TGSR_STITCH_MAX];        // [N][Tb][nk][C][s th][s tw]: dense (C, s th, s tw) block per row, row stride below
  const float* srcB[TGSR_STITCH_MAX];        // nk == 4: variants 4..7 as [N][Tb][4][C][s tw][s th]; else NULL
  void* dst[TGSR_STITCH_MAX];                // [N][C][s H][s W] float32 or uint8
  int64_t stride[TGSR_STITCH_MAX];           // elements between consecutive batch rows of srcA and of srcB
  int C[TGSR_STITCH_MAX];
  int s[TGSR_STITCH_MAX];
  int u8[TGSR_STITCH_MAX];                   // 0: the float32 mean, 1: its uint8 by tgsr_to_uint8's rule
  int vec_src[TGSR_STITCH_MAX];              // bases and row stride on 16 bytes, (s th) % 4 == 0 and (s tw) % 4 == 0
  int vec_dst[TGSR_STITCH_MAX];              // dst base on 16 (float32) / 4 (uint8) bytes and (s W) % 4 == 0
};

// blockIdx.x: blocks of the owned rectangle x channel (a stride loop), blockIdx.y: window, blockIdx.z: entry * N + image.  With
// vec_dst the blocks start on the destination's aligned quads, so an owned rectangle that starts on an odd column has a partial
// first quad.
__global__ __launch_bounds__(256) void d8_merge_kernel(MergeList L, int N, int H, int W, const int32_t* __restrict__ table, int Tb,
                                                       int th, int tw, int nk) {
  __shared__ float tiles[kPass * kBlk * kPitch];
  const int t = blockIdx.y, e = blockIdx.z / N, n = blockIdx.z % N;
  const int32_t* d = table + (int64_t)t * kTileDesc;
  if (!d8_desc_ok(d, H, W, th, tw)) return;                    // uniform over the workgroup
  const int s = L.s[e], C = L.C[e];
  const bool u8 = L.u8[e] != 0, vdst = L.vec_dst[e] != 0, vsrc = L.vec_src[e] != 0;
  const int sy0 = s * d[0], sx0 = s * d[1];                    // the window's origin at this scale
  const int ya = s * d[2], yb = s * d[3], xa = s * d[4], xb = s * d[5];
  const int h = s * th, w = s * tw;
  const int64_t sH = (int64_t)s * H, sW = (int64_t)s * W, plane = (int64_t)h * w;
  const int gx = vdst ? (xa & ~3) : xa;                        // first column of block column 0
  const int nbx = (xb - gx + kBlk - 1) / kBlk, nby = (yb - ya + kBlk - 1) / kBlk;
  const int64_t row = (int64_t)n * Tb + t;                     // the window's first batch row is row * nk (srcA), row * 4 (srcB)
  const int tid = threadIdx.x;
  for (int blk = blockIdx.x; blk < C * nby * nbx; blk += gridDim.x) {
    const int bx = blk % nbx, by = (blk / nbx) % nby, c = blk / (nbx * nby);
    const int Y = ya + by * kBlk, X = gx + bx * kBlk;          // the block in the destination image
    const int y_lo = Y - sy0, x_lo = X - sx0;                  // ... and in the window (x_lo may be -3 .. -1 in block column 0)
    float acc[kSweeps][4];
#pragma unroll
    for (int pass = 0; pass < 8 / kPass; ++pass) {
      __syncthreads();                                         // the previous readers are done with the tiles
      // kChunk loads of a thread in flight before the first of them is stored to LDS (3 x 16 bytes x the 1024 threads of a CU's
      // four workgroups = 48 KiB in flight; five spill under the 128 registers four workgroups leave, nine cost the fourth)
#pragma unroll
      for (int i0 = 0; i0 < kLoads; i0 += kChunk) {
        float4 v[kChunk];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
          const int it = tid + 256 * (i0 + i);
          v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (i0 + i < kLoads && it < kPass * kBlk * kQuads) {
            const int k = pass * kPass + it / (kBlk * kQuads), rq = it % (kBlk * kQuads);
            const D8Block b = d8_block(k, h, w, y_lo, x_lo);
            const float* base = (k < nk ? L.srcA[e] + (row * nk + k) * L.stride[e] : L.srcB[e] + (row * 4 + (k - 4)) * L.stride[e]);
            v[i] = d8_fetch_quad<float>(base + c * plane, b.rows, b.cols, b.r0, b.c0, rq / kQuads, rq % kQuads, vsrc);
          }
        }
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
          const int it = tid + 256 * (i0 + i);
          if (i0 + i < kLoads && it < kPass * kBlk * kQuads) {
            const int rq = it % (kBlk * kQuads);
            d8_keep_quad(v[i], rq / kQuads, rq % kQuads, tiles + (it / (kBlk * kQuads)) * kBlk * kPitch);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kPass; ++kk) {
        const int k = pass * kPass + kk;
        const D8Block b = d8_block(k, h, w, y_lo, x_lo);
        const float* tile = tiles + kk * kBlk * kPitch + (b.c0 & 3);
#pragma unroll
        for (int sw = 0; sw < kSweeps; ++sw) {
          const int ry = sw * kSweepRows + tid / kRowQuads, q = tid % kRowQuads;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            int ti, tj;
            d8_to_variant(k, ry, 4 * q + x, ti, tj);
            const float u = tile[ti * kPitch + tj];
            acc[sw][x] = k == 0 ? u : __fadd_rn(acc[sw][x], u);
          }
        }
      }
    }
#pragma unroll
    for (int sw = 0; sw < kSweeps; ++sw) {
      const int y = Y + sw * kSweepRows + tid / kRowQuads, x = X + 4 * (tid % kRowQuads);
      if (y >= yb) continue;
      const int lo = max(x, xa), hi = min(x + 4, xb);
      if (hi <= lo) continue;
      float m[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) m[i] = __fmul_rn(acc[sw][i], 0.125f);
      const int64_t o = (((int64_t)n * C + c) * sH + y) * sW + x;
      if (vdst && hi - lo == 4) {
        if (u8) {
          uchar4 b4;
          b4.x = d8_f32_to_u8(m[0]); b4.y = d8_f32_to_u8(m[1]); b4.z = d8_f32_to_u8(m[2]); b4.w = d8_f32_to_u8(m[3]);
          *reinterpret_cast<uchar4*>(static_cast<uint8_t*>(L.dst[e]) + o) = b4;
        } else {
          *reinterpret_cast<float4*>(static_cast<float*>(L.dst[e]) + o) = make_float4(m[0], m[1], m[2], m[3]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x + i >= lo && x + i < hi) {
            if (u8) static_cast<uint8_t*>(L.dst[e])[o + i] = d8_f32_to_u8(m[i]);
            else static_cast<float*>(L.dst[e])[o + i] = m[i];
          }
      }
    }
  }
}

static inline bool d8_args_ok(int N, int H, int W, const int32_t* table_host, const int32_t* table_dev, int Tb, int th, int tw) {
  if (!table_host || !table_dev || Tb < 1 || Tb > 65535 || N < 1 || N > kD8MaxN) return false;
  if (H < 1 || W < 1 || H > kTileMaxSide || W > kTileMaxSide || th < 1 || tw < 1 || th > H || tw > W ||
      th > kTileMaxTile || tw > kTileMaxTile)
    return false;
  for (int t = 0; t < Tb; ++t)
    if (!d8_desc_ok(table_host + (int64_t)t * kTileDesc, H, W, th, tw)) return false;
  return true;
}

static inline bool d8_variants_ok(int k0, int nk, int th, int tw) {
  if (nk == 8) return k0 == 0 && th == tw;
  return nk == 4 && (k0 == 0 || k0 == 4);
}

static inline bool d8_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace tgsr

using namespace tgsr;

extern "C" int tgsr_d8_gather(const void* img, const void* img2, int is_u8, int N, int H, int W, const int32_t* table_host,
                              const int32_t* table_dev, int Tb, int th, int tw, int k0, int nk, float* out, float* out2,
                              void* stream) {
  if (!img || !out || (img2 != nullptr) != (out2 != nullptr)) return TGSR_EINVAL;
  if (!d8_args_ok(N, H, W, table_host, table_dev, Tb, th, tw) || !d8_variants_ok(k0, nk, th, tw)) return TGSR_EINVAL;
  const int two = img2 ? 1 : 0;
  if ((int64_t)N * (two + 1) > 65535) return TGSR_EINVAL;
  const uintptr_t in_align = is_u8 ? 4 : 16;
  const int vec_in = (W % 4 == 0) && d8_aligned(img, in_align) && (!img2 || d8_aligned(img2, in_align));
  const int vec_out = (tw % 4 == 0) && (th % 4 == 0) && d8_aligned(out, 16) && (!out2 || d8_aligned(out2, 16));
  const int blocks = 3 * ((th + kBlk - 1) / kBlk) * ((tw + kBlk - 1) / kBlk);
  const dim3 grid((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)Tb, (unsigned)(N * (two + 1)));
  if (is_u8)
    hipLaunchKernelGGL(d8_gather_kernel<uint8_t>, grid, dim3(256), 0, as_stream(stream), static_cast<const uint8_t*>(img),
                       static_cast<const uint8_t*>(img2), H, W, table_dev, Tb, th, tw, k0, nk, out, out2, two, vec_in, vec_out);
  else
    hipLaunchKernelGGL(d8_gather_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(img),
                       static_cast<const float*>(img2), H, W, table_dev, Tb, th, tw, k0, nk, out, out2, two, vec_in, vec_out);
  return note_launch(hipGetLastError(), "d8_gather_kernel");
}

extern "C" int tgsr_d8_merge(int n, const float* const* srcA, const float* const* srcB, const int64_t* src_stride,
                             void* const* dst, const int* C, const int* scale, const int* out_u8, int nk, int N, int H, int W,
                             const int32_t* table_host, const int32_t* table_dev, int Tb, int th, int tw, void* stream) {
  if (n < 1 || n > TGSR_STITCH_MAX || !srcA || !src_stride || !dst || !C || !scale || !out_u8) return TGSR_EINVAL;
  if (!d8_args_ok(N, H, W, table_host, table_dev, Tb, th, tw) || !d8_variants_ok(0, nk, th, tw)) return TGSR_EINVAL;
  if ((int64_t)n * N > 65535 || (nk == 4 && !srcB)) return TGSR_EINVAL;
  MergeList L = {};
  int64_t most = 0;
  for (int e = 0; e < n; ++e) {
    const int s = scale[e];
    const float* b = srcB ? srcB[e] : nullptr;
    if (!srcA[e] || !dst[e] || C[e] < 1 || C[e] > 65535 || s < 1 || s > 64) return TGSR_EINVAL;
    if ((b != nullptr) != (nk == 4)) return TGSR_EINVAL;       // the transposed group apart exactly when srcA holds four
    const int64_t block = (int64_t)C[e] * s * th * s * tw;
    if (src_stride[e] < block) return TGSR_EINVAL;             // a window always has several batch rows
    L.srcA[e] = srcA[e];
    L.srcB[e] = b;
    L.dst[e] = dst[e];
    L.stride[e] = src_stride[e];
    L.C[e] = C[e];
    L.s[e] = s;
    L.u8[e] = out_u8[e] ? 1 : 0;
    L.vec_src[e] = ((int64_t)s * tw) % 4 == 0 && ((int64_t)s * th) % 4 == 0 && d8_aligned(srcA[e], 16) && (!b || d8_aligned(b, 16)) &&
                   src_stride[e] % 4 == 0;
    L.vec_dst[e] = ((int64_t)s * W) % 4 == 0 && d8_aligned(dst[e], out_u8[e] ? 4 : 16);
    const int64_t blocks = (int64_t)C[e] * ((s * th + kBlk - 1) / kBlk) * ((s * tw + 3 + kBlk - 1) / kBlk);
    most = blocks > most ? blocks : most;
  }
  const dim3 grid((unsigned)(most < 4096 ? most : 4096), (unsigned)Tb, (unsigned)(n * N));
  hipLaunchKernelGGL(d8_merge_kernel, grid, dim3(256), 0, as_stream(stream), L, N, H, W, table_dev, Tb, th, tw, nk);
  return note_launch(hipGetLastError(), "d8_merge_kernel");
}
