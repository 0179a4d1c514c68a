// The front edge of the data path on the GPU: what the reference's loaders do per image on the CPU with PIL before
// get_imgs_blur sees a square crop - the CUB bounding-box crop (datasets.py:115-123), transforms.Resize, RandomCrop /
// CenterCrop and RandomHorizontalFlip (test1.py:184-186, datasets.py:1558-1560) - for a RAGGED batch in one launch:
//     img.crop((x1, y1, x2, y2)).resize((ow, oh), BILINEAR).crop((left, top, left + S, top + S))   [mirrored if flip]
// byte-identical to Pillow.  Sources are interleaved H x W x 3 uint8 (what a decoder produces), packed back to back in
// one buffer; the output is planar [B][3][S][S] (what GpuImagePyramid takes).  Only the window is computed:
//   augment_coeffs_kernel : Pillow's precompute_coeffs for the S window columns and S window rows of every image, in
//                           fp64 on the device (the taps depend on each image's own (in, out) pair), into a workspace;
//   augment_u8_kernel     : a workgroup owns kAugTH x kAugTW window pixels of one image.  Horizontal pass over just the
//                           source rows its vertical taps reach -> uint8 intermediate in LDS (Pillow rounds and clips
//                           between the passes), vertical pass, planar store with the mirror folded into the index.
// The arithmetic of a pass is resample_kernel's (tgsr_io.hip): clip8((2^21 + sum in[first + t] * k[t]) >> 22).  A pass
// whose size does not change has the taps (2^22, 0): the same bytes as Pillow's skipping it.
#include "tgsr_common.h"

// Every fp64 step below is ONE IEEE operation in the order of Pillow's C code: no fused multiply-add, no reciprocal.
#pragma clang fp contract(off)

namespace tgsr {

constexpr int kAugDesc = 12;                 // int32 per image: off H W x1 y1 x2 y2 oh ow top left flip
constexpr int kAugMaxSide = 4096;            // source H, W
constexpr int kAugMaxOut = 65536;            // resized oh, ow
constexpr int kAugMaxRatio = 16;             // reduction per axis ...
constexpr int kAugMaxTaps = 2 * kAugMaxRatio + 1;   // ... = Pillow's ksize at that reduction
constexpr int kAugWsRow = 2 + kAugMaxTaps;   // workspace per image and axis: first[S], count[S], taps[kAugMaxTaps][S]
constexpr int kAugTH = 8, kAugTW = 64;       // window tile of a workgroup
// Source rows under kAugTH output rows: centre(r0 + TH - 1) - centre(r0) + 2 support + 1 <= 16 * 7 + 32 + 1 = 145.
constexpr int kAugRows = kAugMaxRatio * (kAugTH - 1) + kAugMaxTaps + 3;
static_assert(3 * kAugRows * kAugTW <= 48 * 1024, "LDS intermediate of augment_u8_kernel");

// The checks that keep every read inside the packed buffer and every LDS index inside the intermediate; the host
// (ops.check_augment_table) applies the same ones with messages, the kernels skip an image that fails them.
__host__ __device__ inline bool aug_desc_ok(const int32_t* d, int S, int64_t nbytes) {
  const int off = d[0], H = d[1], W = d[2], x1 = d[3], y1 = d[4], x2 = d[5], y2 = d[6], oh = d[7], ow = d[8], top = d[9],
            left = d[10], flip = d[11];
  if (off < 0 || H < 1 || W < 1 || H > kAugMaxSide || W > kAugMaxSide) return false;
  if ((int64_t)off + (int64_t)3 * H * W > nbytes) return false;
  if (x1 < 0 || x2 <= x1 || x2 > W || y1 < 0 || y2 <= y1 || y2 > H) return false;
  if (oh < S || ow < S || oh > kAugMaxOut || ow > kAugMaxOut) return false;
  if (top < 0 || top > oh - S || left < 0 || left > ow - S) return false;
  if ((int64_t)(x2 - x1) > (int64_t)kAugMaxRatio * ow || (int64_t)(y2 - y1) > (int64_t)kAugMaxRatio * oh) return false;
  return flip == 0 || flip == 1;
}

__device__ __forceinline__ double triangle(double x) {   // Pillow's bilinear_filter
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// Pillow precompute_coeffs for output index xx: first input index, tap count, and the taps in 22-bit fixed point at
// taps[t * tstride], t < ntaps (zero behind the count).
__device__ __forceinline__ void pillow_coeffs(int in, int out, int xx, int ntaps, int& first, int& count, int32_t* taps,
                                              int tstride) {
  const double scale = (double)in / (double)out;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double center = ((double)xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  if (xmin > in) xmin = in;                              // never for sizes the callers admit: keeps the reads inside
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  if (xmax < 0) xmax = 0;
  if (xmax > ntaps) xmax = ntaps;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += triangle(((double)(x + xmin) - center + 0.5) * ss);
  for (int x = 0; x < ntaps; ++x) {
    int32_t v = 0;
    if (x < xmax) {
      double w = triangle(((double)(x + xmin) - center + 0.5) * ss);   // the same value the sum took
      if (ww != 0.0) w = w / ww;
      v = (int32_t)(w < 0.0 ? -0.5 + w * 4194304.0 : 0.5 + w * 4194304.0);
    }
    taps[(int64_t)x * tstride] = v;
  }
  first = xmin;
  count = xmax;
}

__global__ void resize_coeffs_kernel(int in, int out, int ksize, int32_t* __restrict__ bounds, int32_t* __restrict__ taps) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= out) return;
  int first, count;
  pillow_coeffs(in, out, xx, ksize, first, count, taps + (int64_t)xx * ksize, 1);
  bounds[2 * xx] = first;
  bounds[2 * xx + 1] = count;
}

__global__ void augment_coeffs_kernel(const int32_t* __restrict__ desc, int B, int S, int64_t nbytes, int32_t* __restrict__ ws) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * 2 * S) return;
  const int j = (int)(i % S), axis = (int)((i / S) & 1), b = (int)(i / (2 * S));
  const int32_t* d = desc + (int64_t)b * kAugDesc;
  if (!aug_desc_ok(d, S, nbytes)) return;
  const int in = axis == 0 ? d[5] - d[3] : d[6] - d[4];            // horizontal: crop width -> ow; vertical: crop height -> oh
  const int out = axis == 0 ? d[8] : d[7];
  const int origin = axis == 0 ? d[10] : d[9];
  int32_t* w = ws + ((int64_t)b * 2 + axis) * kAugWsRow * S;
  int first, count;
  pillow_coeffs(in, out, origin + j, kAugMaxTaps, first, count, w + 2 * S + j, S);
  w[j] = first;
  w[S + j] = count;
}

__device__ __forceinline__ uint8_t clip8_22(int ss) {
  ss >>= 22;
  return (uint8_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
}

__global__ __launch_bounds__(256) void augment_u8_kernel(const uint8_t* __restrict__ src, int64_t nbytes,
                                                         const int32_t* __restrict__ desc, const int32_t* __restrict__ ws,
                                                         int S, uint8_t* __restrict__ out) {
  __shared__ uint8_t inter[3 * kAugRows * kAugTW];                 // [channel][source row][window column]
  const int b = blockIdx.z, c0 = blockIdx.x * kAugTW, r0 = blockIdx.y * kAugTH, tid = threadIdx.x;
  const int32_t* d = desc + (int64_t)b * kAugDesc;
  if (!aug_desc_ok(d, S, nbytes)) return;                          // uniform over the workgroup
  const int tw = min(kAugTW, S - c0), th = min(kAugTH, S - r0);
  const int W = d[2], x1 = d[3], y1 = d[4], flip = d[11];
  const int32_t* hw = ws + (int64_t)b * 2 * kAugWsRow * S;
  const int32_t* vw = hw + (int64_t)kAugWsRow * S;
  const int rbase = vw[r0];                                        // first source row of the tile (first[] never decreases)
  const int nrows = min(vw[r0 + th - 1] + vw[S + r0 + th - 1] - rbase, kAugRows);
  const uint8_t* img = src + d[0];

  // horizontal pass: channel fastest, so neighbouring lanes read neighbouring bytes of the interleaved source row
  for (int i = tid; i < nrows * tw * 3; i += 256) {
    const int c = i % 3, col = (i / 3) % tw, row = i / (3 * tw);
    const int first = hw[c0 + col], cnt = hw[S + c0 + col];
    const int32_t* k = hw + 2 * S + c0 + col;
    const uint8_t* p = img + ((int64_t)(y1 + rbase + row) * W + x1 + first) * 3 + c;
    int ss = 1 << 21;
    for (int j = 0; j < cnt; ++j) ss += (int)p[3 * j] * k[(int64_t)j * S];
    inter[(c * kAugRows + row) * kAugTW + col] = clip8_22(ss);
  }
  __syncthreads();

  // vertical pass and the planar store, mirrored where the descriptor says so
  for (int i = tid; i < 3 * th * tw; i += 256) {
    const int col = i % tw, r = (i / tw) % th, c = i / (tw * th);
    const int first = vw[r0 + r] - rbase;
    const int cnt = min(vw[S + r0 + r], nrows - first);
    const int32_t* k = vw + 2 * S + r0 + r;
    const uint8_t* p = inter + (c * kAugRows + first) * kAugTW + col;
    int ss = 1 << 21;
    for (int j = 0; j < cnt; ++j) ss += (int)p[j * kAugTW] * k[(int64_t)j * S];
    const int x = flip ? S - 1 - (c0 + col) : c0 + col;
    out[(((int64_t)b * 3 + c) * S + r0 + r) * S + x] = clip8_22(ss);
  }
}

static inline int aug_ksize(int in, int out) {                     // Pillow: (int)ceil(support) * 2 + 1
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  int c = (int)support;
  if ((double)c < support) ++c;
  return 2 * c + 1;
}

static inline bool aug_aligned4(const void* a, const void* b, const void* c = nullptr) {   // the int32 operands
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 3) == 0;
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int tgsr_resize_coeffs(int in_size, int out_size, int ksize, int32_t* bounds, int32_t* taps, void* stream) {
  if (!bounds || !taps || in_size < 1 || out_size < 1 || in_size > kAugMaxOut || out_size > kAugMaxOut) return TGSR_EINVAL;
  if ((int64_t)in_size > (int64_t)kAugMaxRatio * out_size || ksize != aug_ksize(in_size, out_size)) return TGSR_EINVAL;
  if (!aug_aligned4(bounds, taps)) return TGSR_EUNSUPPORTED;
  hipLaunchKernelGGL(resize_coeffs_kernel, dim3((out_size + 255) / 256), dim3(256), 0, as_stream(stream), in_size, out_size,
                     ksize, bounds, taps);
  return note_launch(hipGetLastError(), "resize_coeffs_kernel");
}

extern "C" int64_t tgsr_augment_ws_elems(int B, int S) {
  if (B < 1 || S < 1) return 0;
  return (int64_t)B * 2 * kAugWsRow * S;
}

extern "C" int tgsr_augment_u8(const uint8_t* packed, int64_t nbytes, const int32_t* table_host, const int32_t* table_dev,
                               int B, int S, int32_t* ws, uint8_t* out, void* stream) {
  if (!packed || !table_host || !table_dev || !ws || !out || nbytes < 1 || nbytes > INT32_MAX) return TGSR_EINVAL;
  if (B < 1 || B > 65535 || S < 1 || S > kAugMaxSide) return TGSR_EINVAL;
  if (!aug_aligned4(table_host, table_dev, ws)) return TGSR_EUNSUPPORTED;
  for (int b = 0; b < B; ++b)
    if (!aug_desc_ok(table_host + (int64_t)b * kAugDesc, S, nbytes)) return TGSR_EINVAL;
  hipStream_t s = as_stream(stream);
  const int64_t n = (int64_t)B * 2 * S;
  hipLaunchKernelGGL(augment_coeffs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, table_dev, B, S, nbytes, ws);
  hipLaunchKernelGGL(augment_u8_kernel, dim3((S + kAugTW - 1) / kAugTW, (S + kAugTH - 1) / kAugTH, B), dim3(256), 0, s, packed,
                     nbytes, table_dev, ws, S, out);
  return note_launch(hipGetLastError(), "augment_u8_kernel");
}
