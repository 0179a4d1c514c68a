// The host-side launch plan of the implicit-GEMM family: the discriminators' 4x4 stride-2 and 3x3 convolutions (tgsr_down.hip,
// ig_plan) and the Inception trunk's generic taps (tgsr_igemm.hip, gc_plan; their three-piece form is tgsr_down.hip's
// dconv_igemm6_kernel).  A plan is computed ONCE per call from the shape, the process-wide switches and - where a launcher knows them -
// the operand alignments; the exported planners read it, the launchers launch from it.  Tile geometry and K-split arithmetic live here
// and nowhere else.
#pragma once
#include "tgsr_common.h"

namespace tgsr {

constexpr int kIgKC = 16;   // K-chunk of every kernel of the family: reduction elements per LDS stage

struct GcArgs {
  const float* A;        // forward: w' [Cout][Cin KH KW]; data gradient: w'T [Cin][Cout KH KW]
  const float* S;        // the gathered tensor (forward: x, data gradient: g), based at its channel slice
  const float* bias;     // forward: shift [Cout]; nullptr: none
  float* out;            // output based at its channel slice (or the slabs when nsplit > 1)
  int M, N, K;
  int Hs, Ws;            // spatial size of S
  int PH, PW;            // the pixel grid N runs over (forward: output pixels; data gradient: input pixels)
  int64_t s_bstride, o_bstride;      // batch strides (elements) of S and out
  int KH, KW, SH, PADH, PADW;
  int relu, accumulate;
  union {
    const float* mask;   // nullable; laid out like `out`: the contribution is kept where mask > 0 (the ReLU of the tensor whose gradient this is)
    float* st;           // STATS (no mask): BatchNorm statistics partials [M][gridDim.x][2]
  };
  int nsplit, chunks_per_split;
  int64_t slab_stride;
};

enum IgForm {
  kIgFp32,       // fp32 MFMA: dconv_igemm_kernel | gconv_igemm_kernel
  kIgSplit,      // bf16 matrix pipe, exact three-piece fp32 operands: dconv_igemm6_kernel
  kIgSplitPre,   // ... with the A operand pre-split into the kernel's LDS images by a pass of its own (bit 2 of tgsr_dconv_set_split)
  kIgImage       // M = a few image channels: the data-gradient kernels with one thread per pixel, no GEMM tile
};

struct IgPlan {
  IgForm form;
  bool wide;                 // WIDE: a 64 (M) x 256 (N) tile; otherwise 128 x 128
  int MB, NB;
  int64_t M, N, K;           // GEMM sizes (K = reduction)
  int ncls;                  // GEMMs per launch (the 4x4 data gradient's four parity classes), folded into grid.z
  int asked, nsplit, cps;    // K split: slabs the fill heuristic asks for; slabs used (no empty one) and chunks per slab
  dim3 grid;
  int64_t head, slab_stride, ws_elems;   // workspace (floats): [head | `asked` slabs of slab_stride] - slab_stride = the output's elements
  int64_t a_bytes, s_bytes;  // what dconv_igemm6_kernel's buffer descriptors of A and S cover
  int nslots, slot_px;       // statistics form: slots per channel and pixels per slot
};

inline void ig_tile(IgPlan& p, bool wide) {
  p.wide = wide;
  p.MB = wide ? 64 : 128;
  p.NB = wide ? 256 : 128;
}
inline int64_t ig_tiles(const IgPlan& p) { return ((p.M + p.MB - 1) / p.MB) * ((p.N + p.NB - 1) / p.NB) * p.ncls; }

// From the slabs asked for to the split that runs - every slab holds at least one chunk - and the grid.  The workspace is sized
// for `asked`, which the used split never exceeds.
inline void ig_split(IgPlan& p, int64_t asked) {
  const int chunks = (int)((p.K + kIgKC - 1) / kIgKC);
  p.asked = (int)asked;
  p.cps = chunks > 0 ? (chunks + p.asked - 1) / p.asked : 1;
  p.nsplit = (chunks + p.cps - 1) / p.cps;
  p.grid = dim3((unsigned)((p.N + p.NB - 1) / p.NB), (unsigned)((p.M + p.MB - 1) / p.MB), (unsigned)(p.nsplit * p.ncls));
  p.ws_elems = p.head + (p.asked > 1 ? p.asked * p.slab_stride : 0);
}

// tgsr_down.hip: tgsr_dconv_set_split != 0.  dconv_igemm6_kernel is one kernel: switching it off takes the trunk's generic taps off
// the three-piece form too, whatever tgsr_gconv_set_form says.
bool ig6_enabled();
// tgsr_down.hip: the generic-tap instance of dconv_igemm6_kernel a kIgSplit plan names.  mode: 0 forward, 1 data gradient, 2 forward
// in its statistics form (one slab: g.st gets one (sum, sum of squares) pair per channel and N tile).
int ig6_gconv_launch(const IgPlan& p, int mode, const GcArgs& g, hipStream_t s);

}  // namespace tgsr
