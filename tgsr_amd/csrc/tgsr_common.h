// Shared helpers for the gfx950 kernels of libtgsr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>

#include "../../include/tgsr_hip.h"

namespace tgsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;     // CDNA wavefront
constexpr int kConvCK = 4;    // input channels per LDS stage (== the packed-weight chunk)

// Records a launch failure for tgsr_last_error(); returns the ABI status.
int note_launch(hipError_t e, const char* what);
// Records a non-HIP failure (e.g. an RCCL status) for tgsr_last_error(); returns TGSR_ELAUNCH.
int note_error(const char* what, const char* detail, int code);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Row of a 32x32 MFMA accumulator register: D[row][col = lane & 31], lane half h = lane >> 5.
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// Blocks b and b+8 share an XCD (round-robin dispatch): give each XCD a contiguous run of tile ids so that
// neighbouring tiles (shared halo rows, same weights) hit the same 4 MiB L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// BatchNorm statistics of one accumulator tile of the trunk's 256-thread implicit GEMMs (gconv_igemm_kernel, dconv_igemm6_kernel:
// wave (wm, wn) holds rows wm 64 + [0, 64) and columns wn 64 + [0, 64) as acc[mb][nb] of the 32x32 MFMA; the wide tile is 64 x 256,
// the square one 128 x 128): per row m < M, over the tile's n_t = min(NB, N - n0) columns n < N, the pair st[(m nslots + slot) 2 +
// {0, 1}] = (sum, sum of squared deviations from the tile's own mean) - the second from the accumulators again once the mean is
// known, so no E[x^2] - E[x]^2 cancellation enters it (tgsr_bn_train_relu_slice_from_stats combines the pairs by Chan's formula).
// Each half-wave reduces its 32 columns by a fixed butterfly, the waves of a row meet in `red` (>= 512 floats of LDS the caller no
// longer reads) in wave order: no atomics, the same bits on every run.
template <bool WIDE>
__device__ __forceinline__ void gemm_tile_stats(const f32x16 (&acc)[2][2], int m0, int n0, int M, int N, float* __restrict__ st,
                                                int nslots, int slot, float* red) {
  constexpr int MB = WIDE ? 64 : 128, NB = WIDE ? 256 : 128, NWN = WIDE ? 4 : 2;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5, wave = tid >> 6;
  const int wm = WIDE ? 0 : wave >> 1, wn = WIDE ? wave : wave & 1;
  const bool ok0 = n0 + wn * 64 + l31 < N, ok1 = n0 + wn * 64 + 32 + l31 < N;
  float* sum_s = red + NWN * MB;                          // [MB] the tile's row sums
  float* mu_s = sum_s + MB;                               // [MB] ... and means
  __syncthreads();                                        // every wave is done with what `red` held
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = wm * 64 + mb * 32 + acc_row(i, hh);
        float v;
        if (pass == 0) {
          v = (ok0 ? acc[mb][0][i] : 0.f) + (ok1 ? acc[mb][1][i] : 0.f);
        } else {
          const float mu = mu_s[r];
          const float d0 = ok0 ? acc[mb][0][i] - mu : 0.f, d1 = ok1 ? acc[mb][1][i] - mu : 0.f;
          v = d0 * d0 + d1 * d1;
        }
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if (l31 == 0) red[wn * MB + r] = v;
      }
    __syncthreads();
    if (tid < MB) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NWN; ++w) v += red[w * MB + tid];
      if (pass == 0) {
        sum_s[tid] = v;
        mu_s[tid] = v / (float)min(NB, N - n0);
      } else if (m0 + tid < M) {
        float* p = st + ((int64_t)(m0 + tid) * nslots + slot) * 2;
        p[0] = sum_s[tid];
        p[1] = v;
      }
    }
    __syncthreads();
  }
}

}  // namespace tgsr
