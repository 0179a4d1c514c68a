// Text-image retrieval for gfx950: a gallery of DAMSM similarities, sentence cosines and retrieval ranks.
//
// damsm_gallery_kernel scores N images against a candidate list of captions each (cand [N][K], or every caption of the pool):
// the arithmetic of damsm_pair_kernel (tgsr_damsm.hip: scores on fp32 MFMA + softmax over words, x gamma1 + softmax over
// regions, weighted context on MFMA, cosine, log sum exp) with one addition, the PACKED pass: the reference's captions are at
// most 18 words and mostly shorter, so a 32-row MFMA tile per caption multiplies mostly zero rows.  A workgroup owns image n
// and the candidate columns (2q, 2q + 1); when both captions have at most 16 words they share the tile - caption a in rows
// 0-15, caption b in rows 16-31 - and ONE pass over the context scores both.  Anything else (a caption of more than 16 words,
// a lone last column, the partner of an empty slot) runs a pass of its own; a long and a short caption go one after the other.
//
// A pair's result does not depend on where it ran.  Every sum over a caption's words runs over its rows in row order, in a
// chain that starts at the caption's first row, and what follows the caption in the tile is an exact zero (x + 0 = x):
//   A   an MFMA output element depends on its own A row and B column only; the softmax over words keeps one running sum per
//       half tile (registers 0-7 are rows 0-15, registers 8-15 rows 16-31 in both half-waves): a solo pass continues the first
//       into the second, a packed pass starts the second at zero
//   B   one wave per row, the same lanes whichever row it is
//   C   one accumulator column per word; the waves' partial sums meet in wave order
//   end the butterfly over the words runs over 16 lanes; a solo pass adds the two halves first, as damsm_pair_kernel does
// so sim for (image, caption) is the same bits packed or solo, in column 2q or 2q + 1, whatever the neighbour.
//
// sent_gallery_kernel (one wave per pair) and retrieval_ranks_kernel (one wave per row) are plain VALU: neither is a hot path.
// No atomics anywhere: the same bits on every run.
#include "tgsr_common.h"

namespace tgsr {

struct GalleryArgs {
  const float* words;      // [M][ndf][Tw]
  const int32_t* lens;     // [M] or null (= Tw)
  const float* ctx;        // [N][ndf][S]
  const int32_t* cand;     // [N][K] or null (cand[n][k] = k)
  int N, M, K, ndf, Tw, S;
  float gamma1, gamma2;
  float* sim;              // [N][K]
};

constexpr int kGSP = 321;  // pitch of the attention image rows (S <= 320)

__global__ __launch_bounds__(256) void damsm_gallery_kernel(GalleryArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* word_s = lds;                        // [ndf][32]   words of the caption(s), zero rows behind each
  float* p_s = word_s + a.ndf * 32;           // [32][kGSP]  attention image
  float* cs = p_s + 32 * kGSP;                // [4 waves][32][65] ctx staging for phase C
  float* red_s = cs + 4 * 32 * 65;            // [3][32]: dot, |wc|^2, |word|^2 per word
  float* wpart_s = red_s + 96;                // [4 waves][96]

  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = a.S, ndf = a.ndf, Tw = a.Tw;
  const int nq = (a.K + 1) >> 1;
  // workgroups go round-robin to the eight XCDs, and with cand == NULL column pair q costs the same (one pass or two) for every
  // image: the pairs are rotated by the image index, so that no XCD is handed the two-pass pairs of every image
  const int n = blockIdx.x / nq;
  int q = blockIdx.x - n * nq + n % nq;
  if (q >= nq) q -= nq;
  const float* cb = a.ctx + (int64_t)n * ndf * S;
  float* out = a.sim + (int64_t)n * a.K;

  // the two columns of this workgroup: caption index (-1 = nothing to score) and length
  int cap0 = -1, cap1 = -1, len0 = 0, len1 = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int k = 2 * q + t;
    if (k < a.K) {
      const int c = a.cand ? a.cand[(int64_t)n * a.K + k] : k;
      if (c >= 0 && c < a.M) {
        int L = a.lens ? a.lens[c] : Tw;
        L = L < 1 ? 1 : (L > Tw ? Tw : L);
        if (t == 0) { cap0 = c; len0 = L; } else { cap1 = c; len1 = L; }
      } else if (tid == 0) {
        out[k] = -INFINITY;                   // an empty slot: nothing is read for it
      }
    }
  }
  const bool packed = cap0 >= 0 && cap1 >= 0 && len0 <= 16 && len1 <= 16;
  const int nsb = (S + 31) / 32;

  for (int pass = 0; pass < 2; ++pass) {      // packed: one pass for both columns; else one pass per caption present
    const int ca = pass ? cap1 : cap0, La = pass ? len1 : len0;
    if (packed ? pass == 1 : ca < 0) continue;                 // uniform per workgroup
    // rows [0, 16) hold words of caption a below lim_lo; rows [16, 32) the rest of a (solo) or caption b (packed) below lim_hi
    const int lim_lo = La < 16 ? La : 16;
    const int lim_hi = packed ? 16 + len1 : La;
    const float* wa = a.words + (int64_t)ca * ndf * Tw;
    const float* wb = packed ? a.words + (int64_t)cap1 * ndf * Tw : wa;
    __syncthreads();                          // the pass before is done with the LDS
    {
      // a thread fills one tile row l = tid & 31 for the features d = tid >> 5, + 8, ...: its source column and whether the row
      // holds a word at all are fixed, so the loop is plain strided loads
      const int l = tid & 31;
      const bool wok = l < (l < 16 ? lim_lo : lim_hi);
      const float* src = (packed && l >= 16) ? wb + (l - 16) : wa + l;
#pragma unroll 8
      for (int d = tid >> 5; d < ndf; d += 8) word_s[d * 32 + l] = wok ? src[d * Tw] : 0.f;
    }
    __syncthreads();

    // ---- A: scores + softmax over the words of each caption, 32 regions per wave pass
    for (int sb = wave; sb < nsb; sb += 4) {
      const int s = sb * 32 + l31;
      const bool sok = s < S;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int k0 = 0; k0 < ndf / 2; k0 += 16) {
        float bv[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) bv[k] = sok ? cb[(int64_t)(2 * (k0 + k) + hh) * S + s] : 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(word_s[(2 * (k0 + k) + hh) * 32 + l31], bv[k], acc, 0, 0, 0);
      }
      float mx_lo = -INFINITY, mx_hi = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, hh);
        if (row >= (r < 8 ? lim_lo : lim_hi)) acc[r] = -INFINITY;
        if (r < 8) mx_lo = fmaxf(mx_lo, acc[r]);
        else mx_hi = fmaxf(mx_hi, acc[r]);
      }
      mx_lo = fmaxf(mx_lo, __shfl_xor(mx_lo, 32));
      mx_hi = fmaxf(mx_hi, __shfl_xor(mx_hi, 32));
      if (!packed) mx_lo = mx_hi = fmaxf(mx_lo, mx_hi);
      float sum_lo = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        acc[r] = __expf(acc[r] - mx_lo);
        sum_lo += acc[r];
      }
      float sum_hi = packed ? 0.f : sum_lo;   // solo: one chain over the 16 registers; packed: caption b starts its own
#pragma unroll
      for (int r = 8; r < 16; ++r) {
        acc[r] = __expf(acc[r] - mx_hi);
        sum_hi += acc[r];
      }
      sum_lo += __shfl_xor(sum_lo, 32);
      sum_hi += __shfl_xor(sum_hi, 32);
      const float inv_hi = a.gamma1 / sum_hi;                  // softmax over words, then x gamma1 (GlobalAttention.py:56,64)
      const float inv_lo = packed ? a.gamma1 / sum_lo : inv_hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) p_s[acc_row(r, hh) * kGSP + s] = sok ? acc[r] * (r < 8 ? inv_lo : inv_hi) : 0.f;
    }
    // zero the padding columns [nsb*32, 320) that phase C multiplies
    for (int o = tid; o < 32 * (320 - nsb * 32); o += 256) {
      const int l = o / (320 - nsb * 32), c = o - l * (320 - nsb * 32);
      p_s[l * kGSP + nsb * 32 + c] = 0.f;
    }
    __syncthreads();

    // ---- B: softmax over regions for each word row (8 rows per wave)
    for (int l = wave * 8; l < wave * 8 + 8; ++l) {
      float* row = p_s + l * kGSP;
      if (l < (l < 16 ? lim_lo : lim_hi)) {
        float v[5];
        float mx = -INFINITY;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          const int s = lane + 64 * m;
          v[m] = s < S ? row[s] : -INFINITY;
          mx = fmaxf(mx, v[m]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float sum = 0.f;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          v[m] = __expf(v[m] - mx);
          sum += v[m];
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
        const float inv = 1.f / sum;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          const int s = lane + 64 * m;
          if (s < S) row[s] = v[m] * inv;
        }
      } else {
        for (int s = lane; s < 320; s += 64) row[s] = 0.f;
      }
    }
    __syncthreads();

    // ---- C: weighted context on MFMA, 32 feature rows per wave pass, then the cosine partial sums per word column
    float* my_cs = cs + wave * 32 * 65;
    float dot = 0.f, nwc = 0.f, nwd = 0.f;
    for (int db = wave; db < ndf / 32; db += 4) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int sc = 0; sc < 5; ++sc) {
        __builtin_amdgcn_wave_barrier();
        for (int o = lane; o < 32 * 64; o += 64) {       // [32 d][64 s] <- ctx rows, coalesced along s
          const int r = o >> 6, c = o & 63;
          const int s = sc * 64 + c;
          my_cs[r * 65 + c] = s < S ? cb[(int64_t)(db * 32 + r) * S + s] : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
          const float av = my_cs[l31 * 65 + 2 * k + hh];                    // A[d = l31][s]
          const float bv = p_s[l31 * kGSP + sc * 64 + 2 * k + hh];          // B[s][l = l31]
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = db * 32 + acc_row(r, hh);
        const float w = word_s[d * 32 + l31];
        dot = fmaf(acc[r], w, dot);
        nwc = fmaf(acc[r], acc[r], nwc);
        nwd = fmaf(w, w, nwd);
      }
    }
    dot += __shfl_xor(dot, 32);
    nwc += __shfl_xor(nwc, 32);
    nwd += __shfl_xor(nwd, 32);
    if (hh == 0) {
      wpart_s[wave * 96 + l31] = dot;
      wpart_s[wave * 96 + 32 + l31] = nwc;
      wpart_s[wave * 96 + 64 + l31] = nwd;
    }
    __syncthreads();
    if (tid < 96) red_s[tid] = ((wpart_s[tid] + wpart_s[96 + tid]) + wpart_s[192 + tid]) + wpart_s[288 + tid];
    __syncthreads();
    if (wave == 0) {
      float e = 0.f;
      if (lane < 32 && lane < (lane < 16 ? lim_lo : lim_hi)) {
        const float den = fmaxf(sqrtf(red_s[64 + lane]) * sqrtf(red_s[32 + lane]), 1e-8f);   // losses.py:12-18
        e = __expf(a.gamma2 * (red_s[lane] / den));                                            // losses.py:279
      }
      e += __shfl_xor(e, 32);                            // lanes 32-63 hold zeros
      if (!packed) e += __shfl_xor(e, 16);               // one caption over both halves of the tile
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) e += __shfl_xor(e, o);
      if (lane == 0) out[2 * q + pass] = __logf(e);                                              // losses.py:280-281
      if (packed && lane == 16) out[2 * q + 1] = __logf(e);
    }
  }
}

// One wave per (image n, candidate k): dot, |cnn|^2 and |rnn|^2 over lanes striding ndf, a fixed butterfly.
__global__ __launch_bounds__(256) void sent_gallery_kernel(const float* __restrict__ cnn, const float* __restrict__ rnn,
                                                           const int32_t* __restrict__ cand, int N, int M, int K, int ndf,
                                                           float eps, float gamma3, float* __restrict__ sim) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (int64_t)N * K) return;                    // uniform per wave
  const int n = (int)(pair / K), k = (int)(pair - (int64_t)n * K);
  const int c = cand ? cand[pair] : k;
  if (c < 0 || c >= M) {
    if (lane == 0) sim[pair] = -INFINITY;
    return;
  }
  const float* x = cnn + (int64_t)n * ndf;
  const float* y = rnn + (int64_t)c * ndf;
  float dot = 0.f, nx = 0.f, ny = 0.f;
  for (int d = lane; d < ndf; d += 64) {
    const float xv = x[d], yv = y[d];
    dot = fmaf(xv, yv, dot);
    nx = fmaf(xv, xv, nx);
    ny = fmaf(yv, yv, ny);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    dot += __shfl_xor(dot, o);
    nx += __shfl_xor(nx, o);
    ny += __shfl_xor(ny, o);
  }
  if (lane == 0) sim[pair] = dot / fmaxf(sqrtf(nx) * sqrtf(ny), eps) * gamma3;   // losses.py:241-246
}

// One wave per row: the position of column t in a stable descending sort of the row, by counting.
__global__ __launch_bounds__(256) void retrieval_ranks_kernel(const float* __restrict__ sim, const int32_t* __restrict__ target,
                                                              int N, int K, int32_t* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                    // uniform per wave
  const int t = target[n];
  if (t < 0 || t >= K) {
    if (lane == 0) rank[n] = -1;
    return;
  }
  const float* row = sim + n * K;
  const float ref = row[t];
  int cnt = 0;
  for (int k = lane; k < K; k += 64) {
    const float v = row[k];
    cnt += (v > ref || (v == ref && k < t)) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) rank[n] = cnt;
}

}  // namespace tgsr

using namespace tgsr;

extern "C" int tgsr_damsm_gallery_fwd(const float* words, const int32_t* cap_lens, const float* ctx, const int32_t* cand,
                                      int N, int M, int K, int ndf, int Tw, int S, float gamma1, float gamma2, float* sim,
                                      void* stream) {
  if (!words || !ctx || !sim || N < 1 || M < 1 || K < 1 || ndf < 32 || Tw < 1 || S < 1) return TGSR_EINVAL;
  if (!cand && K != M) return TGSR_EINVAL;
  if (ndf % 32 != 0 || Tw > 32 || S > 320 || ndf > 512) return TGSR_EUNSUPPORTED;
  const int64_t groups = (int64_t)N * ((K + 1) / 2);
  if (groups > 0x7fffffffLL) return TGSR_EUNSUPPORTED;
  GalleryArgs a;
  a.words = words; a.lens = cap_lens; a.ctx = ctx; a.cand = cand; a.N = N; a.M = M; a.K = K; a.ndf = ndf; a.Tw = Tw; a.S = S;
  a.gamma1 = gamma1; a.gamma2 = gamma2; a.sim = sim;
  const size_t lds = sizeof(float) * ((size_t)ndf * 32 + 32 * kGSP + 4 * 32 * 65 + 96 + 4 * 96);
  static bool attr_set[64] = {false};   // > 64 KB of dynamic LDS needs the opt-in once per DEVICE (see tgsr_damsm.hip)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!attr_set[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(damsm_gallery_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return note_launch(e, "hipFuncSetAttribute(damsm_gallery_kernel)");
    }
    attr_set[dev] = true;
  }
  hipLaunchKernelGGL(damsm_gallery_kernel, dim3((unsigned)groups), dim3(256), lds, as_stream(stream), a);
  return note_launch(hipGetLastError(), "damsm_gallery_kernel");
}

extern "C" int tgsr_sent_gallery_fwd(const float* cnn, const float* rnn, const int32_t* cand, int N, int M, int K, int ndf,
                                     float eps, float gamma3, float* sim, void* stream) {
  if (!cnn || !rnn || !sim || N < 1 || M < 1 || K < 1 || ndf < 1) return TGSR_EINVAL;
  if (!cand && K != M) return TGSR_EINVAL;
  const int64_t blocks = ((int64_t)N * K + 3) / 4;
  if (blocks > 0x7fffffffLL) return TGSR_EUNSUPPORTED;
  hipLaunchKernelGGL(sent_gallery_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), cnn, rnn, cand, N, M, K, ndf,
                     eps, gamma3, sim);
  return note_launch(hipGetLastError(), "sent_gallery_kernel");
}

extern "C" int tgsr_retrieval_ranks(const float* sim, const int32_t* target, int N, int K, int32_t* rank, void* stream) {
  if (!sim || !target || !rank || N < 1 || K < 1) return TGSR_EINVAL;
  hipLaunchKernelGGL(retrieval_ranks_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, as_stream(stream), sim, target, N, K,
                     rank);
  return note_launch(hipGetLastError(), "retrieval_ranks_kernel");
}
