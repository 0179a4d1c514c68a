// Distribution distances for gfx950: the statistics side of the Frechet and kernel distances (tgsr_amd/featdist.py
// states the scores, include/tgsr_hip.h the arithmetic).
//
// Both kernels read float32 features and widen them to fp64 - exact, and the product of two widened values is exact in fp64 - and
// contract them on v_mfma_f64_16x16x4_f64 (C/D: col = lane & 15, row = (lane >> 4) + 4 reg - NOT the f32 map; A[row l15][k = lq],
// B[k = lq][col l15], one f64 per lane).  A workgroup of four waves owns a 64 x 64 tile of the result, wave (wm, wn) its 32 x 32
// quarter as 2 x 2 MFMA tiles; the two operand tiles of a k chunk are staged in LDS as fp32 and widened on the way to the MFMA.
//
// feat_moments_kernel  X^T X: the contraction runs over the ROWS of the batch.  LDS image [k][64 columns], pitch 80 floats (pitch %
//     32 == 16: the two k rows a 32-lane group reads fall on different banks).  Only the tiles on or above the block diagonal run;
//     a tile's 64 x 64 block of `outer` is read, added to and stored by the one lane that owns each element.  The diagonal tiles
//     also add the column sums of their 64 columns, row by row.
// poly_mmd_kernel      G = A B^T over D for 64 gathered rows of each side: LDS image [row][k], pitch 34 floats, read two k at a time
//     (fd_mma_rows); the next chunk of 32 features travels into registers while the MFMAs run on this one.  The epilogue cubes (g / D + 1) in fp64, masks the rows behind m (and, in
//     the two symmetric sums, the diagonal), adds the lane's 16 values, the wave's 64 lanes by a fixed butterfly and the four
//     waves in wave order into ONE partial of `work`; a tile above the diagonal of a symmetric sum counts twice (exact).
// poly_mmd_finish_kernel  adds a sum's partials in tile order.
// No atomics, no host synchronisation, sizes are launch arguments: capturable, and every reduction runs in an order the shapes
// alone fix - the same bits on every run.
#include "tgsr_common.h"

namespace tgsr {

typedef double fd_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kFT = 64;        // side of a workgroup's output tile
constexpr int kFKC = 32;       // rows (moments) / features (mmd) per LDS stage
constexpr int kFMP = 80;       // moments: pitch of a k row of the LDS image, floats
constexpr int kFGP = 34;       // mmd: pitch of a gathered row of the LDS image, floats

// acc[a][b] += A-tile . B-tile over k in [0, kend) (kend % 4 == 0): this wave's 32 x 32 quarter.  As / Bs point at the wave's first
// row / column of the two LDS images; element (row r, k) of either lies at r * rs + k * ks.
__device__ __forceinline__ void fd_mma(const float* __restrict__ As, const float* __restrict__ Bs, int rs, int ks, int kend,
                                       fd_f64x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  for (int k0 = 0; k0 < kend; k0 += 4) {
    const int k = (k0 + lq) * ks;
    const double a0 = (double)As[l15 * rs + k], a1 = (double)As[(16 + l15) * rs + k];
    const double b0 = (double)Bs[l15 * rs + k], b1 = (double)Bs[(16 + l15) * rs + k];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// The same for the [row][k] image of poly_mmd_kernel (pitch kFGP), k in [0, kend) with kend % 8 == 0: a lane reads TWO neighbouring
// k of its row at once (8 bytes) - the order of a contraction is free as long as both operands follow it, so MFMA 2 p takes k =
// 8 p + {0, 2, 4, 6} and MFMA 2 p + 1 takes k = 8 p + {1, 3, 5, 7}.  (l15 34 + 2 lq) mod 64 are 32 different even banks: no conflict.
template <bool FULL>
__device__ __forceinline__ void fd_mma_rows(const float* __restrict__ As, const float* __restrict__ Bs, int kend,
                                            fd_f64x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const float* ap = As + l15 * kFGP + 2 * lq;
  const float* bp = Bs + l15 * kFGP + 2 * lq;
#pragma unroll
  for (int k0 = 0; k0 < kFKC; k0 += 8) {
    if (!FULL && k0 >= kend) break;                                // uniform
    const float2 a0 = *reinterpret_cast<const float2*>(ap + k0), a1 = *reinterpret_cast<const float2*>(ap + 16 * kFGP + k0);
    const float2 b0 = *reinterpret_cast<const float2*>(bp + k0), b1 = *reinterpret_cast<const float2*>(bp + 16 * kFGP + k0);
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a0.x, (double)b0.x, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a0.x, (double)b1.x, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a1.x, (double)b0.x, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a1.x, (double)b1.x, acc[1][1], 0, 0, 0);
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a0.y, (double)b0.y, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a0.y, (double)b1.y, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a1.y, (double)b0.y, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a1.y, (double)b1.y, acc[1][1], 0, 0, 0);
  }
}

__device__ __forceinline__ void fd_zero(fd_f64x4 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = fd_f64x4{0.0, 0.0, 0.0, 0.0};
}

__global__ __launch_bounds__(256) void feat_moments_kernel(const float* __restrict__ x, int n, int D, int64_t ldx,
                                                           double* __restrict__ sum, double* __restrict__ outer) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;                                             // below the block diagonal: not computed, not defined
  __shared__ float xi[kFKC * kFMP], xj[kFKC * kFMP];
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  const int i0 = bi * kFT, j0 = bj * kFT;
  const bool diag = bi == bj;

  fd_f64x4 acc[2][2];
  fd_zero(acc);
  double colsum = 0.0;
  for (int r0 = 0; r0 < n; r0 += kFKC) {
    const int left = n - r0;
    const int kend = left >= kFKC ? kFKC : ((left + 3) & ~3);
    __syncthreads();                                               // the previous chunk's reads are done
    for (int o = tid; o < kFKC * kFT; o += 256) {
      const int r = o >> 6, c = o & 63;
      // every load is unconditional and lands on an element that exists (the row and the column clamped into the matrix); what
      // lies behind n or D is replaced by zero afterwards - a branch around each load would wait for each in turn
      const float* row = x + (int64_t)(r0 + (r < left ? r : left - 1)) * ldx;
      const int ci = i0 + c < D ? i0 + c : D - 1, cj = j0 + c < D ? j0 + c : D - 1;
      const float vi = row[ci], vj = row[cj];
      xi[r * kFMP + c] = (r < left && i0 + c < D) ? vi : 0.f;
      xj[r * kFMP + c] = (r < left && j0 + c < D) ? vj : 0.f;
    }
    __syncthreads();
    fd_mma(xi + wm * 32, xj + wn * 32, 1, kFMP, kend, acc);
    if (diag && tid < kFT) {
      const int rows = left < kFKC ? left : kFKC;
      for (int r = 0; r < rows; ++r) colsum = __dadd_rn(colsum, (double)xi[r * kFMP + tid]);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + wm * 32 + a * 16 + lq + 4 * q, j = j0 + wn * 32 + b * 16 + l15;
        if (i < D && j < D) {
          double* p = outer + (int64_t)i * D + j;
          *p = __dadd_rn(*p, acc[a][b][q]);
        }
      }
  if (diag && tid < kFT && i0 + tid < D) sum[i0 + tid] = __dadd_rn(sum[i0 + tid], colsum);
}

struct MmdArgs {
  const float* x;              // [nx][ldx]
  const float* y;              // [ny][ldy]
  const int32_t* ix;           // [S][m]
  const int32_t* iy;           // [S][m]
  int nx, ny, m, D, T;         // T = tiles per side
  int64_t ldx, ldy;
  double* work;                // [S][3][T T]
};

__global__ __launch_bounds__(256) void poly_mmd_kernel(MmdArgs a) {
  const int which = blockIdx.y, s = blockIdx.z;
  const int ti = blockIdx.x / a.T, tj = blockIdx.x - ti * a.T;
  const bool sym = which < 2;
  if (sym && ti > tj) return;                                      // the lower tiles of a symmetric sum: the upper ones count twice
  __shared__ __attribute__((aligned(16))) float as[kFT * kFGP], bs[kFT * kFGP];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  const int m = a.m, D = a.D;
  const float* A = which == 1 ? a.y : a.x;                         // rows i: x, except in the y-y sum
  const float* B = which == 0 ? a.x : a.y;                         // rows j: y, except in the x-x sum
  const int nA = which == 1 ? a.ny : a.nx, nB = which == 0 ? a.nx : a.ny;
  const int64_t ldA = which == 1 ? a.ldy : a.ldx, ldB = which == 0 ? a.ldx : a.ldy;
  const int32_t* tA = (which == 1 ? a.iy : a.ix) + (int64_t)s * m;
  const int32_t* tB = (which == 0 ? a.ix : a.iy) + (int64_t)s * m;

  // the rows this thread stages: row (tid >> 5) + 8 q of either tile, q < 8, feature tid & 31 of the chunk.  A position behind m
  // or an index outside the feature set stages zeros: its pointer is row 0's (which exists) and its bit in va / vb is clear.
  const int kc = tid & 31, rb = tid >> 5;
  const float* pa[8];
  const float* pb[8];
  unsigned va = 0u, vb = 0u;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = rb + 8 * q;
    const int ia = ti * kFT + r < m ? tA[ti * kFT + r] : -1;
    const int ib = tj * kFT + r < m ? tB[tj * kFT + r] : -1;
    const bool oka = ia >= 0 && ia < nA, okb = ib >= 0 && ib < nB;
    pa[q] = A + (int64_t)(oka ? ia : 0) * ldA;
    pb[q] = B + (int64_t)(okb ? ib : 0) * ldB;
    va |= (oka ? 1u : 0u) << q;
    vb |= (okb ? 1u : 0u) << q;
  }

  // The chunk after the one the MFMAs work on is already on its way into registers: its latency hides behind them.  Every load is
  // unconditional and lands on an element that exists (the feature clamped to D - 1); zeros are selected afterwards - a branch
  // around each load would wait for each in turn.
  float ra[8], rq[8];
  auto fetch = [&](int k0) {
    const bool kok = k0 + kc < D;
    const int kk = kok ? k0 + kc : D - 1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float fa = pa[q][kk], fb = pb[q][kk];
      ra[q] = (kok && ((va >> q) & 1u)) ? fa : 0.f;
      rq[q] = (kok && ((vb >> q) & 1u)) ? fb : 0.f;
    }
  };
  fd_f64x4 acc[2][2];
  fd_zero(acc);
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += kFKC) {
    const int left = D - k0;
    __syncthreads();                                               // the previous chunk's reads are done
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      as[(rb + 8 * q) * kFGP + kc] = ra[q];
      bs[(rb + 8 * q) * kFGP + kc] = rq[q];
    }
    __syncthreads();
    if (left > kFKC) fetch(k0 + kFKC);
    if (left >= kFKC) fd_mma_rows<true>(as + wm * 32 * kFGP, bs + wn * 32 * kFGP, kFKC, acc);
    else fd_mma_rows<false>(as + wm * 32 * kFGP, bs + wn * 32 * kFGP, (left + 7) & ~7, acc);
  }

  const double dD = (double)D;
  double part = 0.0;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = ti * kFT + wm * 32 + p * 16 + lq + 4 * q, j = tj * kFT + wn * 32 + b * 16 + l15;
        const double t = __dadd_rn(__ddiv_rn(acc[p][b][q], dD), 1.0);
        const double k3 = __dmul_rn(__dmul_rn(t, t), t);
        const bool on = i < m && j < m && !(sym && i == j);
        part = __dadd_rn(part, on ? k3 : 0.0);
      }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) part = __dadd_rn(part, __shfl_xor(part, o));
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (tid == 0) {
    double v = __dadd_rn(__dadd_rn(red[0], red[1]), __dadd_rn(red[2], red[3]));
    if (sym && ti < tj) v = __dmul_rn(v, 2.0);
    a.work[((int64_t)s * 3 + which) * a.T * a.T + blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(64) void poly_mmd_finish_kernel(const double* __restrict__ work, int S, int T, double* __restrict__ out) {
  const int o = blockIdx.x * 64 + threadIdx.x;                     // (subset, which)
  if (o >= S * 3) return;
  const bool sym = o % 3 < 2;
  const double* w = work + (int64_t)o * T * T;
  double v = 0.0;
  for (int ti = 0; ti < T; ++ti)
    for (int tj = sym ? ti : 0; tj < T; ++tj) v = __dadd_rn(v, w[ti * T + tj]);
  out[o] = v;
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int tgsr_feat_moments_add(const float* x, int n, int D, int64_t ldx, double* sum, double* outer, void* stream) {
  if (!x || !sum || !outer || n < 1 || D < 1 || ldx < D) return TGSR_EINVAL;
  const int nb = (D + kFT - 1) / kFT;
  if (nb > 65535) return TGSR_EUNSUPPORTED;
  hipLaunchKernelGGL(feat_moments_kernel, dim3(nb, nb), dim3(256), 0, as_stream(stream), x, n, D, ldx, sum, outer);
  return note_launch(hipGetLastError(), "feat_moments_kernel");
}

extern "C" int64_t tgsr_poly_mmd_ws_elems(int S, int m) {
  if (S < 1 || m < 2) return 0;
  const int64_t T = (m + kFT - 1) / kFT;
  return (int64_t)S * 3 * T * T;
}

extern "C" int tgsr_poly_mmd_sums(const float* x, int nx, int64_t ldx, const float* y, int ny, int64_t ldy, const int32_t* ix,
                                  const int32_t* iy, int S, int m, int D, double* work, double* out, void* stream) {
  if (!x || !y || !ix || !iy || !work || !out) return TGSR_EINVAL;
  if (nx < 1 || ny < 1 || S < 1 || m < 2 || D < 1 || ldx < D || ldy < D) return TGSR_EINVAL;
  const int64_t T = (m + kFT - 1) / kFT;
  if (S > 65535 || T * T > 0x7fffffffLL || (int64_t)S * 3 > 0x7fffffffLL - 64) return TGSR_EUNSUPPORTED;
  MmdArgs a;
  a.x = x; a.y = y; a.ix = ix; a.iy = iy; a.nx = nx; a.ny = ny; a.m = m; a.D = D; a.T = (int)T; a.ldx = ldx; a.ldy = ldy;
  a.work = work;
  hipLaunchKernelGGL(poly_mmd_kernel, dim3((unsigned)(T * T), 3, S), dim3(256), 0, as_stream(stream), a);
  const int rc = note_launch(hipGetLastError(), "poly_mmd_kernel");
  if (rc != TGSR_OK) return rc;
  hipLaunchKernelGGL(poly_mmd_finish_kernel, dim3((S * 3 + 63) / 64), dim3(64), 0, as_stream(stream), work, S, (int)T, out);
  return note_launch(hipGetLastError(), "poly_mmd_finish_kernel");
}
