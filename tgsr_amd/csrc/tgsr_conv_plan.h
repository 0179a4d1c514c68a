// The host-side launch plan of the generator's fp32 forward 3x3 convolutions: tgsr_conv3x3.hip, tgsr_upconv.hip, tgsr_upwino.hip,
// tgsr_upwino4.hip, tgsr_winograd.hip and tgsr_winograd4.hip (both of its kernels).  A plan is computed ONCE per call from the sizes, the
// entry's selectors and - where the form asks an alignment - the operand addresses and batch strides (pointers are looked at, never
// read through); the exported planners read it (tgsr_conv3x3_form_plan, tgsr_conv3x3_fwd_plan, the *_stats_nslots), the launchers
// launch from it.  What a launcher refuses is refused HERE: status != TGSR_OK and nothing else filled, every TGSR_EINVAL found ahead
// of every TGSR_EUNSUPPORTED.
#pragma once
#include <climits>

#include "tgsr_common.h"

namespace tgsr {

constexpr int kConvStage = 4;         // input channels per K stage of every form (kConvCK, kUCK, ku4CK, kWCK, k4CK)
constexpr int kConvDirectWaves = 4;   // conv3x3_mfma_kernel's WV: a workgroup = 4 waves x R output rows

struct ConvPlan {
  int status = TGSR_OK, family = 0, t[4] = {0, 0, 0, 0};   // TGSR_CONV_FORM_* = the kernel family, and its template integers (include/tgsr_hip.h)
  dim3 grid, block;
  int tiles_x = 0, tiles_y = 0, tile_h = 0, tile_w = 0;    // workgroup tiles of an image (the Args structs copy them); their OUTPUT pixels
  int stages = 0, groups = 0, nslots = 0;                  // K stages of kConvStage channels; channel groups; statistics slots per channel
};

// One call: the operands and selectors of the entry point.  An entry without a residual passes NULL, one with a fixed epilogue its own.
struct ConvCall {
  const float* x; int64_t xbs; int B, Cin, H, W; const float* pack; int Cout;
  const float *scale, *shift, *res; int64_t rbs; float* out; int64_t obs;
  int epilogue, upsample, stats;       // upsample: read by the direct form only (the up forms always do, the others never)
};

// What differs between the forms' contracts, side by side.  An alignment of n bytes on x asks W % 4 == 0 and x_bstride % 4 == 0 with
// it (rows are fetched 16 bytes at a time); on out / residual, batch strides % (n / 4) == 0 (float2 | float4 stores); 0: any address.
// The register-fed forms read their pack straight from L2 in 16-byte fragments, the others copy it by LDS-DMA from any address.  The
// up-sample-aware Winograd forms index the 2H x 2W output, hence their smaller image.  Cin H W < 2^32 everywhere.
struct ConvForm {
  int cout_mod, cout_mod_glu, cin_mod, x_align, io_align, pack_align, pixel_bits;   // Cout % (with GLU), Cin %; bytes; H W < 2^pixel_bits
  bool up, gate_only, residual, stats;   // up-samples; GLU is its only epilogue; takes a residual; has the statistics epilogue
};
constexpr ConvForm kConvForms[TGSR_CONV_FORMS] = {
    //           Cout GLU Cin |  x out/res pack | H W < 2^ | up, gate only, residual, stats
    /* DIRECT  */ {32, 64, 1, 0, 0, 0, 28, false, false, true, false},      // (up: the call's `upsample`)
    /* UPCONV  */ {64, 64, 1, 0, 8, 0, 28, true, true, false, false},
    /* UPWINO  */ {64, 64, 4, 16, 8, 0, 26, true, false, false, false},
    /* UPWINO4 */ {64, 64, 8, 16, 16, 16, 26, true, false, false, false},   // Cin % 8: an even number of 4-channel stages
    /* WINO    */ {32, 32, 4, 16, 8, 0, 28, false, false, true, true},
    /* WINO4   */ {64, 64, 4, 16, 16, 0, 28, false, false, true, true},
    /* WINO4W  */ {64, 64, 8, 16, 16, 16, 28, false, false, true, true},    // Cin % 8: as upwino4
};

inline bool conv_aligned(const void* p, int64_t bstride, int bytes) {
  return bytes == 0 || ((reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0 && (bstride & (bytes / 4 - 1)) == 0);
}

// Tile choice of conv3x3_mfma_kernel<NOB, GLU, UP, R, 4> on a Ho x Wo output.  Candidates from most operand reuse (2 output blocks per
// workgroup, 8 accumulators per wave) to least (1 block, 4 rows); take the first that gives >= 2 workgroups per CU, else the first
// with >= 1 per CU, else the smallest tile: at B = 16 an idle CU costs more than the lost reuse.  (2-wave workgroups of 2 rows were
// measured: same MFMA chain per wave, no gain - the WV parameter stays for a K-split.)  As coded, a first pass that finds nothing
// ahead of the LAST candidate (1 block, 4 rows) leaves the choice to the second pass: a taller tile with >= 256 workgroups then wins
// over the 4-row tile with >= 512 (B = 1, 96 filters, 17 x 1345: 16 rows, 258 workgroups).  The shipped shapes were tuned with it;
// tests/test_infer_abi_host.py restates it.  nob = output blocks per workgroup (the kernel's NOB), rows = output rows per workgroup.
inline void conv_direct_tile(int B, int Ho, int Wo, int Cout, bool glu, int& nob, int& rows) {
  const int unit = glu ? 64 : 32;          // couts consumed per output block
  const int nob_max = (Cout % (2 * unit) == 0) ? 2 : 1;
  struct Cand { int nob, rows; };
  Cand cands[8];
  int nc = 0;
  for (int nb = nob_max; nb >= 1; --nb) {
    const int ncb = nb * (glu ? 2 : 1);
    if (ncb <= 2) cands[nc++] = {nb, 16};
    cands[nc++] = {nb, 8};
    cands[nc++] = {nb, 4};
  }
  auto reaches = [&](const Cand& c, int floor) {   // B x tiles x groups >= floor, without a product that could wrap
    const int g = Cout / (unit * c.nob);
    return (int64_t)B * ((Ho + c.rows - 1) / c.rows) * ((Wo + 31) / 32) >= (floor + g - 1) / g;
  };
  int pick = nc - 1;
  for (int pass = 0; pass < 2 && pick == nc - 1; ++pass)
    for (int i = 0; i < nc; ++i)
      if (reaches(cands[i], pass == 0 ? 512 : 256)) { pick = i; break; }
  nob = cands[pick].nob; rows = cands[pick].rows;
}

// The plan as far as the sizes and selectors decide it - everything but `stages`: what tgsr_conv3x3_fwd_plan and the *_stats_nslots
// answer from.  The statistics instance is the plain epilogue's (the *_stats_fwd entries pass TGSR_EPI_AFFINE and no affine).
inline ConvPlan conv_tiles(int form, int B, int H, int W, int Cout, int epilogue, int upsample, int stats) {
  if (form < 0 || form >= TGSR_CONV_FORMS || B < 1 || H < 1 || W < 1 || Cout < 1) return {TGSR_EINVAL};
  const ConvForm& f = kConvForms[form];
  const bool glu = epilogue == TGSR_EPI_AFFINE_GLU, st = stats && !glu, up = f.up || (form == TGSR_CONV_FORM_DIRECT && upsample);
  if ((!glu && epilogue != TGSR_EPI_AFFINE) || (f.gate_only && !glu) || (stats && !f.stats)) return {TGSR_EINVAL};
  if (Cout % (glu ? f.cout_mod_glu : f.cout_mod) != 0 || (int64_t)H * W >= (1ll << f.pixel_bits)) return {TGSR_EUNSUPPORTED};
  ConvPlan p;
  // a workgroup: tile_h x tile_w OUTPUT pixels x cpg filters, `block` threads, `slots` statistics slots; the groups in grid.y | grid.x
  int cpg = 64, block = 256, slots = 0, nob = 0, nh = 0, nb = 0;
  bool groups_in_y = false;
  p.family = form; p.t[0] = glu; p.tile_h = 4; p.tile_w = 64;
  switch (form) {
    case TGSR_CONV_FORM_DIRECT:    // conv3x3_mfma_kernel<NOB, GLU, UP, R, 4>: 4 waves x R rows x 32 columns x NOB blocks of 32 (GLU: 64) filters
      conv_direct_tile(B, H << up, W << up, Cout, glu, nob, p.tile_h);
      p.t[0] = nob; p.t[1] = glu; p.t[2] = up; p.t[3] = p.tile_h / kConvDirectWaves;
      p.tile_w = 32; cpg = (glu ? 64 : 32) * nob; block = 64 * kConvDirectWaves; groups_in_y = true;
      break;
    // upconv_glu_mfma_kernel: 4 source rows x 32 source columns, 32 values + their gates; upwino_kernel<GLU>: 2 source rows x 16 source
    // columns; upwino4_kernel<GLU>: 4 x 64 outputs
    case TGSR_CONV_FORM_UPCONV: p.t[0] = 0; p.tile_h = 8; groups_in_y = true; break;
    case TGSR_CONV_FORM_UPWINO: p.tile_w = 32; break;
    case TGSR_CONV_FORM_UPWINO4: break;
    // wino_conv3x3_kernel<GLU, NH, STATS>: NH = 2 cout halves where Cout % 64 == 0 (4 x 32 outputs x 64 filters), else 1 (8 x 32 x 32);
    // one slot per wave = per tile row of 2 x 32 outputs
    case TGSR_CONV_FORM_WINO:
      nh = Cout % 64 == 0 ? 2 : 1;
      p.t[1] = nh; p.t[2] = st; p.tile_h = 8 / nh; p.tile_w = 32; cpg = 32 * nh; slots = p.tile_h / 2;
      break;
    // wino4_conv3x3_kernel<GLU, STATS>: 8 x 64 outputs, 8 waves; one slot per tile row of 4 x 64
    case TGSR_CONV_FORM_WINO4: p.t[1] = st; p.tile_h = 8; block = 512; slots = 2; break;
    // wino4w_conv3x3_kernel<GLU, NB, STATS>: 4 x 64 outputs x NB blocks of 16 filters - 128-row groups (8 waves) where the layer has
    // them, else 64-row groups (4 waves); one slot per workgroup
    default:
      nb = Cout % 128 == 0 ? 8 : 4;
      p.t[1] = nb; p.t[2] = st; cpg = 16 * nb; block = 64 * nb; slots = 1;
  }
  p.tiles_x = ((W << up) + p.tile_w - 1) / p.tile_w; p.tiles_y = ((H << up) + p.tile_h - 1) / p.tile_h; p.groups = Cout / cpg;
  // a grid that does not fit is refused, not wrapped: tiles (< 2^31 x 2^26) first, so that no product below can leave an int64
  const int64_t tiles = (int64_t)B * p.tiles_x * p.tiles_y, gx_groups = groups_in_y ? 1 : p.groups;
  if (tiles > INT_MAX || tiles * gx_groups > INT_MAX || tiles * slots > INT_MAX) return {TGSR_EUNSUPPORTED};
  p.grid = dim3((unsigned)(tiles * gx_groups), groups_in_y ? (unsigned)p.groups : 1u); p.block = dim3(block); p.nslots = (int)(tiles * slots);
  return p;
}

// The plan of a call: the shared validation around conv_tiles.
inline ConvPlan conv_plan(int form, const ConvCall& c) {
  if (form < 0 || form >= TGSR_CONV_FORMS) return {TGSR_EINVAL};
  const ConvForm& f = kConvForms[form];
  if (!c.x || !c.pack || !c.out || c.Cin < 1 || (c.scale == nullptr) != (c.shift == nullptr)) return {TGSR_EINVAL};
  if (c.res && (c.epilogue == TGSR_EPI_AFFINE_GLU || !f.residual)) return {TGSR_EINVAL};
  ConvPlan p = conv_tiles(form, c.B, c.H, c.W, c.Cout, c.epilogue, c.upsample, c.stats);
  if (p.status != TGSR_OK) return p;
  if (c.Cin % f.cin_mod != 0 || (int64_t)c.Cin * c.H * c.W >= (1ll << 32)) return {TGSR_EUNSUPPORTED};
  if ((f.x_align && (c.W & 3)) || !conv_aligned(c.x, c.xbs, f.x_align) || !conv_aligned(c.out, c.obs, f.io_align) ||
      (c.res && !conv_aligned(c.res, c.rbs, f.io_align)) || !conv_aligned(c.pack, 0, f.pack_align))
    return {TGSR_EUNSUPPORTED};
  p.stages = (c.Cin - 1) / kConvStage + 1;     // the channels rounded up (Cin >= 1; Cin + 3 could wrap)
  return p;
}

// What every Args struct of these kernels holds under the same name
template <class Args>
inline void conv_fill(Args& a, const ConvCall& c, const ConvPlan& p) {
  a.x = c.x; a.xbs = c.xbs; a.B = c.B; a.Cin = c.Cin; a.H = c.H; a.W = c.W; a.Cout = c.Cout;
  a.scale = c.scale; a.shift = c.shift; a.out = c.out; a.obs = c.obs; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y;
}

// A pack launcher: the check, the grid (256-thread blocks, at most `cap`: the kernels stride) and the launch of kernel(w, pack, Cout,
// Cin, rest..., total)
template <class Kernel, class... Rest>
inline int launch_pack(Kernel kernel, const char* name, int cout_mod, int cap, int64_t total, void* stream, const float* w, float* pack,
                       int Cout, int Cin, Rest... rest) {
  if (!w || !pack || Cout < 1 || Cin < 1) return TGSR_EINVAL;
  if (Cout % cout_mod != 0) return TGSR_EUNSUPPORTED;
  const int64_t want = (total + 255) / 256;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, as_stream(stream), w, pack, Cout, Cin, rest..., total);
  return note_launch(hipGetLastError(), name);
}

}  // namespace tgsr
