// The host-side launch plan of the generator's fp32 weight gradients: tgsr_conv3x3_wgrad.hip, tgsr_wino_wgrad.hip, tgsr_upwino_wgrad.hip
// and the image heads' tgsr_conv_to3_bwd.hip.  A plan is computed ONCE per call from the sizes, the TGSR_WGRAD_* knobs and - where the
// instance depends on them - the operand alignments (pointers are looked at, never read through); the exported planners read it, the
// launchers launch from it.  What a launcher refuses is refused HERE, before any division: status != TGSR_OK, ws_elems == 0.
#pragma once
#include "tgsr_common.h"

namespace tgsr {

constexpr int kWWT = 8, kUWT = 16;   // wino: 2x2 output tiles per chunk; upwino: low-resolution pixels per chunk

struct WgradPlan {
  int status = TGSR_OK, family = 0, t[3] = {0, 0, 0};   // TGSR_WGRAD_FAMILY_* and its template integers (include/tgsr_hip.h); none for the image head
  int units = 0, per_wg = 0, nslots = 0, groups = 0;   // tiles | chunks; per workgroup; partial slabs = grid.x; channel groups = grid.y
  dim3 grid, block;
  int64_t slab = 0, ws_elems = 0;      // floats of one slab; of the workspace = nslots * slab
  int tiles_x = 0, tiles_y = 0, chunks_x = 0, cgroups_i = 0, CinPad = 0;   // what the kernels' Args structs copy
  int mfma = 0, rpw = 0, dgrad_tiles_y = 0;   // image head: matrix-core kernel, its rows per wave; the 16-row tiles of the data gradient
};

// Experiment knobs, read once per process.  TGSR_WGRAD_SPLIT_PCT scales how many partial slabs the split kernels produce (100 = the
// plan's own choice).  TGSR_WGRAD_TILE = 32 | 64 forces the DMA-staged Winograd kernel's 64 co x 32 ci (two workgroups per CU) or 64 x 64
// form on the Cout % 64 == 0, Cin % 64 == 0 layers (0 / unset: by layer size).  TGSR_WGRAD_DMA = 0 keeps the register-fetch kernel.
inline int wgrad_knob(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
inline int wgrad_split_pct() { static const int v = wgrad_knob("TGSR_WGRAD_SPLIT_PCT", 100); return v < 1 ? 100 : v; }
inline int wgrad_tile() { static const int v = wgrad_knob("TGSR_WGRAD_TILE", 0); return v; }
inline bool wgrad_dma_on() { static const bool on = [] { const char* e = getenv("TGSR_WGRAD_DMA"); return !(e && e[0] == '0'); }(); return on; }

// From the slabs wanted to the split that runs: `want` scaled by the knob and clamped to [1, units], one slab per workgroup and no
// empty workgroup; then the grid and the workspace.  units >= 1: the plan functions refuse an empty shape first.
inline void wgrad_split(WgradPlan& p, int units, int want, int block) {
  want = want * wgrad_split_pct() / 100;
  want = want < 1 ? 1 : (want > units ? units : want);
  p.units = units; p.per_wg = (units + want - 1) / want; p.nslots = (units + p.per_wg - 1) / p.per_wg;
  p.grid = dim3(p.nslots, p.groups); p.block = dim3(block);
  p.ws_elems = p.nslots * p.slab;
}

// conv3x3_wgrad_kernel<NCOB, NCIB, UP>: 32-channel blocks, tiles of 2 x 32 output pixels
inline WgradPlan wgrad_plan_direct(int B, int Cin, int H, int W, int Cout, int upsample) {
  if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return {TGSR_EINVAL};
  if (Cout % 32 != 0) return {TGSR_EUNSUPPORTED};
  WgradPlan p;
  const int up = upsample != 0, cb = Cout / 32, ib = (Cin + 31) / 32;
  const int ncob = cb % 4 == 0 ? 4 : (cb % 2 == 0 ? 2 : 1), ncib = ib % 2 == 0 ? 2 : 1;
  p.family = TGSR_WGRAD_FAMILY_DIRECT; p.t[0] = ncob; p.t[1] = ncib; p.t[2] = up;
  p.cgroups_i = ib / ncib; p.groups = (cb / ncob) * p.cgroups_i; p.CinPad = ib * 32;
  p.tiles_x = ((W << up) + 31) / 32; p.tiles_y = ((H << up) + 1) / 2; p.slab = (int64_t)9 * Cout * p.CinPad;
  // one partial slab per workgroup: ~256 CUs x 8 waves of workgroups in flight keeps the chip full while the slabs
  // (nslots x |dW|) stay ~75 MB for every layer shape
  wgrad_split(p, B * p.tiles_y * p.tiles_x, 2048 / (ncob * ncib) / p.groups, 64 * ncob * ncib);
  return p;
}

// wino_wgrad_kernel<NCI, NCOB> | wino_wgrad_dma_kernel<NCI>: 32-channel blocks, chunks of kWWT 2x2 tiles of one tile row
inline WgradPlan wgrad_plan_wino(const float* grad_out, const float* x, int64_t x_bstride, int B, int Cin, int H, int W, int Cout) {
  if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return {TGSR_EINVAL};
  if (Cout % 32 != 0 || Cin % 32 != 0) return {TGSR_EUNSUPPORTED};
  WgradPlan p;
  p.tiles_y = (H + 1) / 2; p.chunks_x = ((W + 1) / 2 + kWWT - 1) / kWWT;
  const int nchunks = B * p.tiles_y * p.chunks_x;
  // The 64 x 32 tile (two 4-wave workgroups per CU) measured 3-20 % faster than the 64 x 64 one on the 32^2 and 64^2 layers
  // (<= 2 048 chunks at batch 16: 47 -> 37, 35 -> 31, 83 -> 79, 57 -> 54 us) and 3 % slower on the 128^2 ones
  // (tools/exp_wgrad.py; TGSR_WGRAD_TILE=32 | 64 forces one of them).
  const bool both64 = Cin % 64 == 0 && Cout % 64 == 0;
  const bool use32 = both64 && W % 4 == 0 && (wgrad_tile() == 32 || (wgrad_tile() == 0 && nchunks <= 2048));
  const int nci = (Cin % 64 == 0 && !use32) ? 2 : 1, ncob = Cout % 64 == 0 ? 2 : 1;
  // the DMA-staged instance (at nci = 1: the 64 x 32 tile of a 64-ci-multiple layer): 16-byte aligned planes and rows
  const bool dma = wgrad_dma_on() && both64 && W % 4 == 0 && x_bstride % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  p.family = dma ? TGSR_WGRAD_FAMILY_WINO_DMA : TGSR_WGRAD_FAMILY_WINO; p.t[0] = nci; p.t[1] = dma ? 0 : ncob;
  p.cgroups_i = Cin / (32 * nci); p.groups = (Cout / (32 * ncob)) * p.cgroups_i; p.slab = (int64_t)16 * Cout * Cin;
  // one 8-wave workgroup per CU: fewer, longer K walks keep the slabs small; the 64 x 32 tile: two 4-wave workgroups per CU
  int want = (use32 ? 512 : 256) / p.groups;
  // the 32 x 32 layers (<= 512 chunks at batch 16) are slab-bound - 2-4 chunks of work per workgroup against a 64-KB..512-KB
  // slab written and re-read: half the split measured 5-20 % faster there, slower everywhere else (tools/exp_wgrad.py)
  if (nchunks <= 512 && want >= 64) want /= 2;
  wgrad_split(p, nchunks, want, 128 * nci * ncob);
  return p;
}

// upwino_wgrad_kernel<NCI>: 64-row co blocks only, chunks of kUWT low-resolution pixels of one row
inline WgradPlan wgrad_plan_upwino(const float* grad_out, int B, int Cin, int H, int W, int Cout) {
  if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return {TGSR_EINVAL};
  if (Cout % 64 != 0 || Cin % 32 != 0 || (reinterpret_cast<uintptr_t>(grad_out) & 7) != 0) return {TGSR_EUNSUPPORTED};
  WgradPlan p;
  const int nci = (Cin % 64 == 0) ? 2 : 1;
  p.family = TGSR_WGRAD_FAMILY_UPWINO; p.t[0] = nci; p.cgroups_i = Cin / (32 * nci); p.groups = (Cout / 64) * p.cgroups_i;
  p.chunks_x = (W + kUWT - 1) / kUWT; p.slab = (int64_t)9 * Cout * Cin;
  const int nchunks = B * H * p.chunks_x;
  int want = 512 / p.groups;                  // two workgroups per CU in flight; fewer, longer K walks keep the slabs small
  if (nchunks <= 1024 && want >= 64) want /= 2;   // the 32 x 32 upBlocks are slab-bound (tools/exp_wgrad.py: 54 -> 41 us, 46 -> 42)
  wgrad_split(p, nchunks, want, 128 * nci);
  return p;
}

// The image head, one slab per workgroup: conv_to3_wgrad_mfma_kernel<K, TANH, Cin / 16> where W % 16 == 0 and Cin in {16, 32, 48, 64},
// on tiles of 4 rpw rows x 64 pixels with rpw (rows per wave) the largest of 8, 4, 2, 1 that still gives >= 1024 workgroups; else
// conv_to3_wgrad_kernel<K, TANH> on the data gradient's 16 x 64 tiles.
inline WgradPlan wgrad_plan_to3(int B, int Cin, int H, int W, int K) {
  if (B < 1 || Cin < 1 || H < 1 || W < 1) return {TGSR_EINVAL};
  if ((K != 3 && K != 5) || Cin > 64) return {TGSR_EUNSUPPORTED};
  WgradPlan p;
  p.tiles_x = (W + 63) / 64; p.tiles_y = p.dgrad_tiles_y = (H + 15) / 16; p.mfma = W % 16 == 0 && Cin % 16 == 0;
  for (p.rpw = p.mfma ? 8 : 1; p.rpw > 1 && (int64_t)B * p.tiles_x * ((H + 4 * p.rpw - 1) / (4 * p.rpw)) < 1024;) p.rpw >>= 1;
  if (p.mfma) p.tiles_y = (H + 4 * p.rpw - 1) / (4 * p.rpw);
  p.units = p.nslots = B * p.tiles_x * p.tiles_y; p.per_wg = p.groups = 1; p.grid = dim3(p.nslots); p.block = dim3(256);
  p.slab = (int64_t)3 * Cin * K * K; p.ws_elems = p.nslots * p.slab;
  return p;
}

}  // namespace tgsr
