/*
 * tgsr_hip.h - C ABI of libtgsr_hip.so: the MI355X (gfx950 / CDNA4) kernels of the TGSR
 * text-conditioned super-resolution hot path.
 *
 * The reference (cxm12/TGSR) has no FFI layer: its boundary is Python module/class names backed by stock
 * torch ops.  Each entry point below replaces the torch call sequence cited next to it (paths relative to
 * the reference root).  Conventions for every function:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless named host_*;
 *   - fp32, NCHW, dense inner (C,H,W) layout; the batch stride is explicit (in elements) so a kernel can read
 *     or write a channel slice of a wider buffer (this is how the reference's torch.cat, util.py:771/817,
 *     disappears);
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - never allocates, never synchronises, no global mutable state (the attention mask is an argument,
 *     not module state as in GlobalAttention.py:84-85), safe to capture into a hipGraph;
 *   - returns TGSR_OK (0) or a negative TGSR_E* code; nothing throws.
 */
#ifndef TGSR_HIP_H
#define TGSR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGSR_OK 0
#define TGSR_EINVAL (-1)       /* bad pointer / size / flag combination */
#define TGSR_EUNSUPPORTED (-2) /* shape outside what the kernels tile for (see each function) */
#define TGSR_ELAUNCH (-3)      /* hipLaunch reported an error; see tgsr_last_error() */

/* Epilogue selectors for tgsr_conv3x3_fwd. */
#define TGSR_EPI_AFFINE 0     /* y = conv*scale + bias                        (conv3x3 + BatchNorm2d eval) */
#define TGSR_EPI_AFFINE_GLU 1 /* y = a[:C/2] * sigmoid(a[C/2:]), a = affine   (+ GLU, util.py:45-53)       */

/* Activation selectors for tgsr_conv_to3_fwd. */
#define TGSR_ACT_NONE 0 /* y = conv                                  (GET_IMAGE_G_noAct, util.py:909-919) */
#define TGSR_ACT_TANH_AXPY 1 /* y = tanh(conv) + alpha * addend      (conv_output + a*SRb, model.py:224,280) */
#define TGSR_ACT_IDENT_AXPY 2 /* y = conv + alpha * addend           (useAct=False, model.py:226; tgsr_lp_conv_to3_map_fwd only) */

/* ABI version of this header; tgsr_abi_version() must return the same number. */
#define TGSR_ABI_VERSION 2
int tgsr_abi_version(void);
/* Static string describing the last launch error seen by this process (debug aid). */
const char* tgsr_last_error(void);

/*
 * Re-lay a conv weight [Cout][Cin][K][K] (torch layout) as [ceil(Cin/4)][K*K][4][Cout] with zero-filled
 * channel padding: the order tgsr_conv3x3_fwd streams it into LDS.  Replaces nothing in the reference (layout
 * only); done once per weight version.  wpack must hold tgsr_packed_weight_elems(Cout,Cin,K) floats.
 */
int64_t tgsr_packed_weight_elems(int Cout, int Cin, int K);
int tgsr_pack_conv_weight(const float* w, float* wpack, int Cout, int Cin, int K, void* stream);
/* The pack of the DATA-GRADIENT convolution straight from the forward conv's weight: w is [Cin][Cout][K][K] (the forward
 * layer maps Cout -> Cin channels) and the packed filter is w'[co][ci][ky][kx] = w[ci][co][K-1-ky][K-1-kx] - what
 * autograd's conv_transpose of a stride-1 "same" convolution computes; no flip / transpose / copy kernels. */
int tgsr_pack_conv_weight_dgrad(const float* w, float* wpack, int Cout, int Cin, int K, void* stream);

/*
 * BatchNorm2d (eval) as a per-channel affine: scale = weight / sqrt(running_var + eps),
 * bias' = bias - running_mean * scale.  Replaces nn.BatchNorm2d.eval() at util.py:77,116,119.
 */
int tgsr_bn_fold(const float* weight, const float* bias, const float* running_mean, const float* running_var,
                 float eps, float* scale, float* shift, int C, void* stream);

/*
 * Fused 3x3 convolution (stride 1, zero pad 1, no bias), fp32 on the MFMA units.
 * Replaces, in one launch:
 *   conv3x3 -> BatchNorm2d(eval) -> GLU                 ResBlock.block[0..2] util.py:114-117, im2f util.py:741-744,
 *                                                       convin/residual24/48 model.py:228-232
 *   conv3x3 -> BatchNorm2d(eval) [+ residual]           ResBlock.block[3..4] + `out += residual` util.py:118-129
 *   Upsample(x2, nearest) -> conv3x3 -> BN -> GLU       upBlock util.py:74-80 (upsample=1: the x2 gather is folded
 *                                                       into the LDS tile read, the 4x larger tensor never exists)
 * x        [B][Cin][H][W], batch stride x_bstride elements
 * wpack    from tgsr_pack_conv_weight(K=3)
 * scale/shift [Cout] affine applied to the conv result (NULL,NULL = identity)
 * residual NULL or [B][Cout_out][Ho][Wo] (batch stride res_bstride) added after the affine; only with
 *          TGSR_EPI_AFFINE
 * out      [B][Cout_out][Ho][Wo], Ho = H*(upsample?2:1); Cout_out = Cout/2 with GLU else Cout
 * Supported: Cout % 32 == 0 (Cout % 64 == 0 with GLU); any B, Cin, H, W >= 1 with H W < 2^28 and Cin H W < 2^32 (TGSR_EUNSUPPORTED
 * beyond, as in every convolution below; the up-sample-aware Winograd forms stop at H W < 2^26).  No alignment is asked of x, out or
 * residual and any batch stride will do; wpack is read 16 bytes at a time.  TGSR_EINVAL: a NULL x / wpack / out, a size < 1, scale
 * without shift (or the reverse), an unknown epilogue, GLU with a residual.
 */
int tgsr_conv3x3_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* wpack, int Cout,
                     const float* scale, const float* shift, const float* residual, int64_t res_bstride, float* out,
                     int64_t out_bstride, int epilogue, int upsample, void* stream);
/*
 * The tile tgsr_conv3x3_fwd takes at this shape: host arithmetic only (no launch, no device access), the very function the
 * launcher calls.  The kernel instance is conv3x3_mfma_kernel<*nob, GLU, upsample != 0, *rows_per_wave, 4>: a workgroup = 4 waves
 * x *rows_per_wave (4, 2 or 1) output rows x 32 columns x *nob (2 or 1) blocks of 32 (GLU: 64) filters; grid.y = *groups.
 * Returns what tgsr_conv3x3_fwd returns for these sizes and selectors (TGSR_EINVAL: a size < 1 or an unknown epilogue;
 * TGSR_EUNSUPPORTED: Cout % 32 (GLU: % 64) != 0 or H W >= 2^28); the outputs (any may be NULL) are written only with TGSR_OK.
 */
int tgsr_conv3x3_fwd_plan(int B, int H, int W, int Cout, int epilogue, int upsample, int* nob, int* rows_per_wave, int* groups);

/*
 * upBlock (util.py:74-80) by sub-pixel decomposition: Upsample(x2, nearest) -> conv3x3 -> affine (BN eval) -> GLU
 * computed as four 2x2 convolutions on the PRE-upsample tensor with pre-summed taps: 4*Cin MACs per output instead
 * of 9*Cin, same result up to the rounding of the weight sums (tgsr_conv3x3_fwd(upsample=1) is the 9-tap form, kept
 * for the training path).  wpack from tgsr_pack_upconv_weight (tgsr_packed_upconv_weight_elems floats).
 * x [B][Cin][H][W] (batch stride), out [B][Cout/2][2H][2W] (8-byte aligned with an even batch stride); Cout % 64 == 0.
 */
int64_t tgsr_packed_upconv_weight_elems(int Cout, int Cin);
int tgsr_pack_upconv_weight(const float* w, float* wpack, int Cout, int Cin, void* stream);
int tgsr_upconv3x3_glu_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* wpack, int Cout,
                           const float* scale, const float* shift, float* out, int64_t out_bstride, void* stream);

/*
 * The same upBlock by Winograd F(2x2, 3x3) on the up-sampled image with the up-sampling folded into the input
 * transform: the doubled rows / columns zero 7 of the 16 Winograd positions, leaving 9 products per 2x2 outputs =
 * 2.25 multiplies per output (sub-pixel form above: 4, direct: 9).  fp32; the transforms only add / subtract.
 * upack from tgsr_pack_upwino_weight (tgsr_packed_upwino_weight_elems floats; glu = 1 groups value channels with
 * their gates and must match the entry point used).  Cout % 64 == 0, Cin % 4 == 0,
 * W % 4 == 0, x 16-byte aligned (batch stride % 4 == 0), out 8-byte aligned with an even batch stride.
 */
int64_t tgsr_packed_upwino_weight_elems(int Cout, int Cin);
int tgsr_pack_upwino_weight(const float* w, float* upack, int Cout, int Cin, int glu, void* stream);
int tgsr_upwino_glu_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack, int Cout,
                        const float* scale, const float* shift, float* out, int64_t out_bstride, void* stream);
/* The same without GLU: out [B][Cout][2H][2W] = affine(conv3x3(upsample(x))) (scale/shift may be NULL: the raw
 * convolution BatchNorm's batch statistics are taken of in training).  Pack with glu = 0. */
int tgsr_upwino_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack, int Cout,
                    const float* scale, const float* shift, float* out, int64_t out_bstride, void* stream);

/*
 * upBlock by Winograd F(4x4, 3x3) on the up-sampled grid with the x2 folded into the input transform: 25 multiplies per
 * 16 outputs (tgsr_upwino_glu_fwd: 36) - the third transformed row / column vanishes and the fifth is -1/3 of the fourth,
 * so 5 x 5 positions carry products and their B operands come from 16 values per tile (tgsr_upwino4.hip).  `glu` != 0:
 * out [B][Cout/2][2H][2W] = GLU(affine(conv3x3(upsample(x)))), else [B][Cout][2H][2W] without the gate (scale/shift may be
 * NULL).  upack from tgsr_pack_upwino4_weight(glu) (tgsr_packed_upwino4_weight_elems floats, per-wave fragment order: the A
 * operands go from L2 straight into registers).  Cout % 64 == 0, Cin % 8 == 0, W % 4 == 0, x / out / upack 16-byte aligned
 * with batch strides % 4 == 0.  Numerics: F(4x4)'s (see
 * tgsr_wino4_conv3x3_fwd); callers route by output size (tgsr_amd.ops.upwino4_wanted).
 */
int64_t tgsr_packed_upwino4_weight_elems(int Cout, int Cin);
int tgsr_pack_upwino4_weight(const float* w, float* upack, int Cout, int Cin, int glu, void* stream);
int tgsr_upwino4_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack, int Cout,
                     const float* scale, const float* shift, float* out, int64_t out_bstride, int glu, void* stream);

/*
 * The same fused 3x3 convolution as tgsr_conv3x3_fwd (upsample = 0) by Winograd F(2x2, 3x3): 16 multiplies per 4
 * outputs instead of 36.  fp32 throughout; the transforms only use {0, +-1, +-1/2} (end-to-end error on the shipped
 * checkpoint indistinguishable from the direct fp32 form).  upack from tgsr_pack_wino_weight
 * (tgsr_packed_wino_weight_elems floats; `glu` != 0 groups each value channel block with its gate block and must
 * match the epilogue the pack is used with).  Cout % 32 == 0 (64-channel groups when Cout % 64 == 0, else 32), Cin % 4 == 0, W % 4 == 0, x 16-byte
 * aligned (batch stride % 4 == 0), out / residual 8-byte aligned with even batch strides; same epilogue selectors and residual rule as tgsr_conv3x3_fwd.
 */
int64_t tgsr_packed_wino_weight_elems(int Cout, int Cin);
int tgsr_pack_wino_weight(const float* w, float* upack, int Cout, int Cin, int glu, void* stream);
/* Winograd pack of the data-gradient convolution from the forward weight [Cin][Cout][3][3] (see
 * tgsr_pack_conv_weight_dgrad); plain channel order (no GLU grouping). */
int tgsr_pack_wino_weight_dgrad(const float* w, float* upack, int Cout, int Cin, void* stream);
int tgsr_wino_conv3x3_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack, int Cout,
                          const float* scale, const float* shift, const float* residual, int64_t res_bstride,
                          float* out, int64_t out_bstride, int epilogue, void* stream);

/*
 * The same convolution by Winograd F(4x4, 3x3): 36 multiplies per 16 outputs (1.78x fewer than F(2x2), 4x fewer than the
 * direct form), for the large layers of the inference path - ResBlock.block util.py:110-130 at 128^2 and above.  fp32
 * throughout; the transforms hold 4, 5, 8 and 1/24, so its rounding error is ~15x that of the other two forms per layer
 * (3e-5 on unit-scale data): on the shipped checkpoint the finest image stays at 3.0e-5 (max, against fp64) with the 128^2
 * and 64^2 layers on this kernel, 2.1e-4 with the 32^2 layers on it too (profiles/HISTORY.md 3.1e) - callers route by layer size.  upack from
 * tgsr_pack_wino4_weight (tgsr_packed_wino4_weight_elems floats; U = G g G^T computed in double, rounded once; `glu` must
 * match the epilogue).  Cout % 64 == 0, Cin % 4 == 0, W % 4 == 0; x, out, residual 16-byte aligned with batch strides
 * % 4 == 0; same epilogue selectors and residual rule as tgsr_conv3x3_fwd.
 */
int64_t tgsr_packed_wino4_weight_elems(int Cout, int Cin);
int tgsr_pack_wino4_weight(const float* w, float* upack, int Cout, int Cin, int glu, void* stream);
/* F(4x4) pack of the data-gradient convolution from the forward weight [Cin][Cout][3][3] (see tgsr_pack_conv_weight_dgrad). */
int tgsr_pack_wino4_weight_dgrad(const float* w, float* upack, int Cout, int Cin, void* stream);
int tgsr_wino4_conv3x3_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack, int Cout,
                           const float* scale, const float* shift, const float* residual, int64_t res_bstride,
                           float* out, int64_t out_bstride, int epilogue, void* stream);

/* The register-fed form of the same kernel: the A operands straight from L2 in per-wave fragment order.  Cout % 128 == 0: a
 * workgroup = one tile row x 128 accumulator rows (the input transform amortised over twice the channels); else 64-row groups
 * in 4-wave workgroups, two independent per CU.  Same contract with Cin % 8 == 0; its own pack layout
 * (tgsr_packed_wino4_weight_elems floats, 16-byte aligned). */
int tgsr_pack_wino4_wide_weight(const float* w, float* upack, int Cout, int Cin, int glu, void* stream);
/* ... of the data-gradient convolution, from the forward weight [Cin][Cout][3][3] (see tgsr_pack_conv_weight_dgrad) */
int tgsr_pack_wino4_wide_weight_dgrad(const float* w, float* upack, int Cout, int Cin, void* stream);
/* ... with the statistics epilogue of tgsr_wino4_conv3x3_stats_fwd (training forward): one pair per channel and workgroup (4 x 64
 * outputs).  Like the other two *_stats_nslots: the plan's nslots, 0 for sizes the launcher refuses (a size < 1, Cout % 64, H W >= 2^28). */
int tgsr_wino4_wide_stats_nslots(int B, int H, int W, int Cout);
int tgsr_wino4_wide_conv3x3_stats_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack,
                                      int Cout, float* out, int64_t out_bstride, float* stat_partial, void* stream);
int tgsr_wino4_wide_conv3x3_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack, int Cout,
                                const float* scale, const float* shift, const float* residual, int64_t res_bstride,
                                float* out, int64_t out_bstride, int epilogue, void* stream);
/* tgsr_wino4w_set_persist(cap): how many workgroups a register-fed launch starts for the workgroup tiles of its plan (the plan's
 * grid stays the tile count).  -1 (the default): as many as the device holds at once - one 8-wave or two 4-wave workgroups per
 * CU - each walking tiles id, id + n, ...; 0: one tile per workgroup; n > 0: at most n workgroups.  TGSR_WINO4W_PERSIST in the
 * environment selects the same values at load.  The outputs are bit-identical whatever the value.  Returns the previous value. */
int tgsr_wino4w_set_persist(int cap);

/*
 * The planner of the seven forms above.  Every launch of theirs is planned once, by one host function (csrc/tgsr_conv_plan.h, which
 * also holds the table of what the forms ask of their operands); tgsr_conv3x3_form_plan is that very function.  Host arithmetic
 * only: the pointers are looked at for NULL and for their alignment and never read through.  `form` = TGSR_CONV_FORM_*, the rest as
 * the form's entry point takes it: `pack` its wpack / upack, `epilogue` TGSR_EPI_AFFINE_GLU for tgsr_upconv3x3_glu_fwd,
 * tgsr_upwino_glu_fwd and tgsr_upwino4_fwd(glu != 0), `residual` NULL for the entries that take none, `upsample` read by
 * TGSR_CONV_FORM_DIRECT only, `stats` != 0 for the *_stats_fwd entries (which pass no scale / shift / residual and TGSR_EPI_AFFINE).
 * It returns what the entry point returns for these operands ahead of its launch (TGSR_EINVAL: an unknown form, a NULL x / pack /
 * out, a size < 1, scale without shift, an unknown epilogue, a residual with GLU or for a form without one, an epilogue or `stats`
 * the form has no kernel for; TGSR_EUNSUPPORTED: channel counts, image sizes, alignments or a grid beyond 2^31 - 1 workgroups) and,
 * with TGSR_OK only, fills plan[TGSR_CONV_PLAN_FIELDS] (may be NULL):
 *     [0] the kernel family = form     [1..4] its template integers, 0 where it has fewer:
 *         DIRECT conv3x3_mfma_kernel<NOB, GLU, UP, R, 4>, UPCONV upconv_glu_mfma_kernel, UPWINO upwino_kernel<GLU>, UPWINO4
 *         upwino4_kernel<GLU>, WINO wino_conv3x3_kernel<GLU, NH, STATS>, WINO4 wino4_conv3x3_kernel<GLU, STATS>, WINO4W
 *         wino4w_conv3x3_kernel<GLU, NB, STATS>
 *     [5] grid.x     [6] grid.y     [7] block.x     [8] tiles_x     [9] tiles_y: workgroup tiles of an image
 *     [10] [11] rows and columns of a workgroup tile in OUTPUT pixels     [12] K stages of 4 input channels     [13] channel groups
 *     [14] nslots: statistics slots per channel (the forms with a *_stats_fwd entry; what their *_stats_nslots answer)
 */
#define TGSR_CONV_FORM_DIRECT 0
#define TGSR_CONV_FORM_UPCONV 1
#define TGSR_CONV_FORM_UPWINO 2
#define TGSR_CONV_FORM_UPWINO4 3
#define TGSR_CONV_FORM_WINO 4
#define TGSR_CONV_FORM_WINO4 5
#define TGSR_CONV_FORM_WINO4W 6
#define TGSR_CONV_FORMS 7
#define TGSR_CONV_PLAN_FIELDS 15
int tgsr_conv3x3_form_plan(int form, const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* pack, int Cout,
                           const float* scale, const float* shift, const float* residual, int64_t res_bstride, const float* out,
                           int64_t out_bstride, int epilogue, int upsample, int stats, int* plan);

/*
 * tgsr_conv_to3_set_pipe(on): the streaming form of tgsr_conv_to3_fwd with its LDS copies two stages ahead in a ring of three buffers
 * (counted waits) and the filter in LDS - on by default where W % 4 == 0 and the filter takes <= 16 KB (TGSR_TO3_PIPE=0 in the
 * environment turns it off); the images are bit-identical either way.  Returns the previous setting.
 */
int tgsr_conv_to3_set_pipe(int on);

/*
 * KxK convolution (K = 3 or 5, stride 1, zero pad K/2, no bias) to 3 output channels + optional epilogue.
 * Replaces GET_IMAGE_G_noAct.img (util.py:913-915; K=3, TGSR_ACT_NONE) and
 * conv_output = conv5x5 + Tanh followed by `one*. + a*SRb` (model.py:224, 280/288/297; K=5, TGSR_ACT_TANH_AXPY).
 * x [B][Cin][H][W] (batch stride x_bstride), w [3][Cin][K][K] (torch layout), addend NULL or [B][3][H][W] dense,
 * out [B][3][H][W] dense.  No alignment is required (tgsr_conv_to3_plan names the kernel the operands get).  TGSR_EUNSUPPORTED: K
 * other than 3 or 5; TGSR_EINVAL: a NULL x / w / out, a size < 1, an `act` other than the two above, an addend with TGSR_ACT_NONE.
 */
int tgsr_conv_to3_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* w, int K,
                      int act, const float* addend, float alpha, float* out, void* stream);
/*
 * The kernel tgsr_conv_to3_fwd takes for these operands: host arithmetic only (no launch, no device access; the pointers are
 * inspected for alignment, never dereferenced), the very function the launchers call.  *form:
 *   TGSR_TO3_FORM_MFMA    conv_to3_mfma_kernel: K = 5, Cin % 16 == 0, W % 64 == 0, H % 8 == 0, >= 512 tiles of 8 x 64, x 16-byte
 *                         aligned with x_bstride % 4 == 0
 *   TGSR_TO3_FORM_PIPE    conv_to3_pipe_kernel: the 16-byte copy form below with the filter (<= 16 KB) in LDS, unless
 *                         tgsr_conv_to3_set_pipe(0) is in force (the plan follows that setting)
 *   TGSR_TO3_FORM_VEC4    conv_to3_kernel, 16-byte copies: W % 4 == 0, x_bstride % 4 == 0, x / out / addend 16-byte aligned
 *   TGSR_TO3_FORM_SCALAR  conv_to3_kernel, 4-byte copies and stores: everything else
 * *tile_rows = output rows per workgroup: 16 while B ceil(W / 64) ceil(H / 16) >= 512, else 8 while that count at 8 rows is >= 512,
 * else 4 (the input channels split over 1 / 2 / 4 thread groups); 8 for the MFMA form.  Returns what tgsr_conv_to3_fwd returns
 * for these arguments with a filter, a known `act` and an addend `act` permits; form / tile_rows (either may be NULL) are
 * written only with TGSR_OK.
 */
#define TGSR_TO3_FORM_MFMA 0
#define TGSR_TO3_FORM_PIPE 1
#define TGSR_TO3_FORM_VEC4 2
#define TGSR_TO3_FORM_SCALAR 3
int tgsr_conv_to3_plan(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, int K, const float* addend,
                       const float* out, int* form, int* tile_rows);

/*
 * The closing launch of the fp32 inference step: tgsr_conv_to3_fwd(act = TGSR_ACT_NONE) of the LAST low-frequency head and the
 * `+ a * SRb` of every NetG_highweight head (tgsr_axpy_images) in one launch.  n = 1..3 triples (fine[k], t[k], s[k]) of numel[k]
 * dense floats; the last one (k = n - 1) is this head's scale: numel[n - 1] == B * 3 * H * W and s[n - 1] is not read, it is `out`.
 *   out         = conv(x)                       exactly the image of tgsr_conv_to3_fwd
 *   fine[n - 1] = fmaf(alpha, out, t[n - 1])    from the accumulators, in the same epilogue
 *   fine[k]     = fmaf(alpha, s[k], t[k])       k < n - 1, in extra workgroups behind the tiles
 * - the fma of tgsr_axpy_images, bit for bit.  Only the streaming form with 16-byte copies takes it: TGSR_EUNSUPPORTED where
 * W % 4 != 0, x_bstride % 4 != 0, x / out / a triple's pointer is not 16-byte aligned, numel[k] % 4 != 0, n > 3, the filter takes
 * more than 16 KB, the shape goes to the matrix-pipe form (K = 5 on large images) or tgsr_conv_to3_set_pipe(0) is in force;
 * TGSR_EINVAL for a missing pointer, n < 1 or a last triple of another size.  A refused call writes nothing.
 */
int tgsr_conv_to3_finish_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* w, int K, float* out,
                             int n, float* const* fine, const float* const* t, const float* const* s, const int64_t* numel,
                             float alpha, void* stream);

/*
 * Word-level attention of the generator (GlobalAttentionGeneral.forward, GlobalAttention.py:87-130) in two
 * launches: the 1x1 projection of the word embeddings (:100-102) and a fused QK^T -> mask -> softmax over words
 * -> PV kernel on MFMA (:107-128).
 * h        [B][idf][Q] (batch stride h_bstride), idf in {32,64,128}
 * words    [B][cdf][T] dense, T <= 32;  w_ctx [idf][cdf]
 * mask     NULL or uint8 [B][T], non-zero = padded word (captions == 0, trainer_objective.py:136-140)
 * mask_mode 0 = reference behaviour: score row b*Q+q is masked with mask[(b*Q+q) % B]
 *               (`mask.repeat(queryL,1)`, GlobalAttention.py:111); 1 = per-sample masking (mask[b])
 * src_ws   workspace, B*idf*32 floats (the projected words, zero padded to 32).  With words == w_ctx == NULL the
 *          projection is skipped and src_ws is read as the output of tgsr_word_project_fwd.
 * With `words` the projection stages one sample's words in LDS, cdf * 128 bytes: cdf <= 1024 (TGSR_EUNSUPPORTED beyond; above
 * cdf = 512 the launcher opts the kernel in to more than 64 KB of dynamic LDS, once per device).  w_ctx needs no more than its
 * 4-byte alignment: its rows are read as float4 only where w_ctx is 16-byte aligned and cdf % 4 == 0, one float at a time otherwise
 * (the same products in the same order: the same bits).
 * c_code   [B][idf][Q] (batch stride c_bstride);  attn [B][T][Q] dense (may be NULL: not written)
 */
int tgsr_word_attention_fwd(const float* h, int64_t h_bstride, const float* words, const float* w_ctx,
                            const uint8_t* mask, int mask_mode, int B, int idf, int cdf, int T, int Q, float* src_ws,
                            float* c_code, int64_t c_bstride, float* attn, void* stream);

/*
 * The projection alone, for up to 4 conv_context weight sets over the same words in one launch (the generator's
 * stages share the word embeddings): src_out[set][B][idf][32] = w_ctx[set] [idf][cdf] x words [B][cdf][T], zero padded
 * to 32 words.  w_ctx: HOST array of nsets device pointers.  idf % 32 == 0, T <= 32.
 */
int tgsr_word_project_fwd(const float* words, const float* const* w_ctx, int nsets, int B, int idf, int cdf, int T,
                          float* src_out, void* stream);

/*
 * Bidirectional 1-layer LSTM text encoder, eval mode (RNN_ENCODER.forward util.py:233-260: Embedding ->
 * pack_padded_sequence -> LSTM -> pad_packed_sequence -> transpose; final hidden = sentence code).
 * captions int64 [B][width]; cap_lens int32 [B] (each 1..Tmax <= width); emb [ntoken][ninput];
 * w_ih [2][4H][ninput], w_hh [2][4H][H], b_ih/b_hh [2][4H]  (direction 0 = forward, 1 = reverse; gate order i,f,g,o)
 * gates_ws workspace B*Tmax*2*4H floats.
 * words_emb [B][2H][Tmax] (zero beyond each length), sent_emb [B][2H].   H <= 256, 4H % 64 == 0.
 *
 * What holds for every entry point of this family (LSTM and GRU, forward and backward; tests/test_hip_rnn_abi.py):
 *   - alignment: w_hh of a FORWARD call must be 16-byte aligned wherever a register kernel runs it - H in {32, 64, 128}, LSTM and
 *     GRU, whose threads read their w_hh rows as float4; a w_hh that is not is refused with TGSR_EUNSUPPORTED (tgsr_last_error()
 *     says so) before anything is launched.  The LSTM forward at any other H and both backwards read w_hh by single floats.  Every
 *     other float / int32 operand, outputs and workspaces included, needs 4-byte alignment only (captions: 8), and the results do
 *     not depend on it.
 *   - lengths: cap_lens[b] is clamped into [0, Tmax]: a length above Tmax acts as Tmax; a length <= 0 gives a sample whose
 *     words_emb rows and sent_emb row are all zero (and, in the backwards, all-zero gradient and hprev rows).
 *   - tokens: a caption entry outside [0, ntoken) reads row 0 of emb / of the table.
 *   - acts (training forms): the rows of the steps t >= cap_lens[b] are neither written by the forward nor read by the
 *     backward; the caller need not clear them.
 *   - the gate workspace is written before it is read: the results do not depend on what it held.
 */
int tgsr_bilstm_fwd(const int64_t* captions, int width, const int32_t* cap_lens, int B, int Tmax, const float* emb,
                    int ntoken, int ninput, const float* w_ih, const float* w_hh, const float* b_ih,
                    const float* b_hh, int H, float* gates_ws, float* words_emb, float* sent_emb, void* stream);

/*
 * Eval-mode form of the same encoder: with frozen weights the input projection depends on the token only, so
 * tgsr_lstm_gate_table builds table[ntoken][2][4H] = emb[tok] . w_ih[d]^T + b_ih[d] + b_hh[d] once per weight version
 * (the same GEMM kernel, same arithmetic per row) and tgsr_bilstm_table_fwd runs the recurrence reading its gate
 * pre-activations through the caption: one launch per batch instead of two, bit-identical to tgsr_bilstm_fwd.
 */
int tgsr_lstm_gate_table(const float* emb, int ntoken, int ninput, const float* w_ih, const float* b_ih,
                         const float* b_hh, int H, float* table, void* stream);
int tgsr_bilstm_table_fwd(const int64_t* captions, int width, const int32_t* cap_lens, int B, int Tmax,
                          const float* table, int ntoken, const float* w_hh, int H, float* words_emb, float* sent_emb,
                          void* stream);

/*
 * Which recurrence kernel the three LSTM forwards above and below (tgsr_bilstm_fwd, tgsr_bilstm_table_fwd,
 * tgsr_bilstm_train_fwd) run for (H, Tmax): one of TGSR_LSTM_RECURRENT_*, or TGSR_EUNSUPPORTED (H < 1, H > 256 or
 * 4H % 64 != 0).  Host only, launches nothing; the launcher switches on the same answer.  Every instance but
 * TGSR_LSTM_RECURRENT_GENERIC reads w_hh as float4 (the alignment rule above).  The environment variable TGSR_LSTM_ONE_ROW
 * (an A/B switch of the tools, read once per process) sends H = 128 to TGSR_LSTM_RECURRENT_128 at every Tmax.
 */
#define TGSR_LSTM_RECURRENT2_128 1    /* lstm_recurrent2_kernel<128, 24, 4>: H == 128, Tmax <= 24 (its steps are staged in LDS) */
#define TGSR_LSTM_RECURRENT_128 2     /* lstm_recurrent_kernel<128>: H == 128, Tmax > 24 */
#define TGSR_LSTM_RECURRENT_64 3      /* lstm_recurrent_kernel<64> */
#define TGSR_LSTM_RECURRENT_32 4      /* lstm_recurrent_kernel<32> */
#define TGSR_LSTM_RECURRENT_GENERIC 5 /* lstm_recurrent_generic_kernel: every other H, 4H threads */
int tgsr_lstm_recurrent_plan(int H, int Tmax);

/*
 * The GRU branch of RNN_ENCODER (util.py:207-211: `nn.GRU(ninput, nhidden, 1, batch_first=True, bidirectional=True)` when
 * cfg.RNN_TYPE == 'GRU'; forward util.py:233-260, sent_emb = the final hidden states, :257), eval mode, same packed-sequence
 * semantics.  Gate order r, z, n.  tgsr_gru_gate_table: table[ntoken][2][3H] = emb[tok] . w_ih[d]^T + b_ih[d] + b_hh_rz[d], where
 * b_hh_rz [2][3H] = b_hh with its n third zeroed (b_hn enters inside r * (W_hn h + b_hn)); tgsr_bigru_table_fwd: the recurrence
 * through the caption, b_hn [2][H].  words_emb [B][2H][Tmax] (zero behind a caption), sent_emb [B][2H].  H in {32, 64, 128}.
 * w_hh [2][3H][H] 16-byte aligned; lengths, tokens and every other operand as stated at tgsr_bilstm_fwd.
 */
int tgsr_gru_gate_table(const float* emb, int ntoken, int ninput, const float* w_ih, const float* b_ih, const float* b_hh_rz,
                        int H, float* table, void* stream);
int tgsr_bigru_table_fwd(const int64_t* captions, int width, const int32_t* cap_lens, int B, int Tmax, const float* table,
                         int ntoken, const float* w_hh, const float* b_hn, int H, float* words_emb, float* sent_emb,
                         void* stream);

/*
 * Training path of the GRU branch (the reference trains whichever cell cfg.RNN_TYPE names, pretrain_DAMSM.py:49-98 through
 * util.py:233-260).  tgsr_bigru_train_fwd: x [B][Tmax][ninput] = the embedded, dropped-out captions; gates_ws [B*Tmax][2][3H]
 * workspace; acts [B][Tmax][2][4][H] = (r, z, n, W_hn h + b_hn) of every step.  tgsr_bigru_bwd walks every (sample, direction) back
 * through time from d_words [B][2H][Tmax] and d_sent [B][2H] (NULL = zero): dgx / dgh [B][Tmax][2][3H] = the gradients at the
 * input-side (x W_ih^T + b_ih) and hidden-side (h W_hh^T + b_hh) gate pre-activations, hprev [B][Tmax][2][H] = h of the previous
 * step, dbias [2][2][3H] = (d b_ih, d b_hh) (NULL: skipped).  The caller's GEMMs give dW_ih = dgx^T x, dW_hh = dgh^T hprev,
 * dx = dgx W_ih.  Fixed summation orders.  H in {32, 64, 128}.  dgx, dgh and hprev are zero at the steps behind a caption;
 * acts rows of those steps are not written by the forward and not read by the backward.  w_hh: 16-byte aligned for the forward.
 */
int tgsr_bigru_train_fwd(const float* x, const int32_t* cap_lens, int B, int Tmax, int ninput, const float* w_ih,
                         const float* w_hh, const float* b_ih, const float* b_hh_rz, const float* b_hn, int H, float* gates_ws,
                         float* acts, float* words_emb, float* sent_emb, void* stream);
int tgsr_bigru_bwd(const int32_t* cap_lens, int B, int Tmax, int H, const float* w_hh, const float* acts, const float* words_emb,
                   const float* d_words, const float* d_sent, float* dgx, float* dgh, float* hprev, float* dbias, void* stream);

/*
 * Training path of the same encoder.  tgsr_bilstm_train_fwd takes the already embedded (and dropped-out) inputs
 * x [B][Tmax][ninput] and additionally saves acts [B][Tmax][2][5][H] (i, f, g, o activations and the cell state of
 * every step).  tgsr_bilstm_bwd walks every (sample, direction) back through time from d_words [B][2H][Tmax] and
 * d_sent [B][2H] (may be NULL) and emits the pre-activation gate gradients dgates [B][Tmax][2][4H] (zero past the
 * caption), hprev [B][Tmax][2][H] (the hidden state entering each step) and dbias [2][4H] (= d b_ih = d b_hh; may be
 * NULL).  The weight / input gradients are plain GEMMs on those (tgsr_linear_fwd):
 *   dW_ih[d] = dgates[:, :, d]^T x,   dW_hh[d] = dgates[:, :, d]^T hprev[:, :, d],   dx = dgates W_ih.
 * H in {32, 64, 128} for the backward.  hprev is zero past the caption as dgates is; acts rows of the steps past a caption
 * are not written by the forward and not read by the backward; alignment, lengths as stated at tgsr_bilstm_fwd.
 */
int tgsr_bilstm_train_fwd(const float* x, const int32_t* cap_lens, int B, int Tmax, int ninput, const float* w_ih,
                          const float* w_hh, const float* b_ih, const float* b_hh, int H, float* gates_ws, float* acts,
                          float* words_emb, float* sent_emb, void* stream);
int tgsr_bilstm_bwd(const int32_t* cap_lens, int B, int Tmax, int H, const float* w_hh, const float* acts,
                    const float* words_emb, const float* d_words, const float* d_sent, float* dgates, float* hprev,
                    float* dbias, void* stream);

/*
 * DAMSM word/region attention for the whole (image, caption) grid in one launch: func_attention
 * (GlobalAttention.py:33-74) as driven by words_loss (losses.py:73-113) - the B-iteration Python loop, word.repeat,
 * both softmaxes, the two bmm and the cosine / exp / sum / log tail.
 * words [B][ndf][Tw] dense (Tw <= 32), cap_lens int32 [B] (NULL = Tw for all; a length outside [1, Tw] is clamped into it, here and
 * in tgsr_damsm_words_bwd), ctx [B][ndf][S] dense (S = 17*17 <= 320), ndf % 32 == 0, ndf <= 512.
 * sim      [B_img][B_cap] = log sum_{w < len} exp(gamma2 * cos(word_w, region-context_w))   (losses.py:102-109;
 *          the caller multiplies by gamma3 and applies the class mask / cross entropy)
 * att_diag NULL or [B][Tw][S]: attention of image i on caption i, rows >= cap_lens[i] zero       (losses.py:93)
 */
int tgsr_damsm_words_fwd(const float* words, const int32_t* cap_lens, const float* ctx, int B, int ndf, int Tw, int S,
                         float gamma1, float gamma2, float* sim, float* att_diag, void* stream);

/*
 * Backward of tgsr_damsm_words_fwd (the attention maps carry no gradient, like in the reference): grad_sim
 * [B_img][B_cap] -> grad_words32 [B][ndf][32] (word axis padded to 32; the caller keeps [:Tw]) and grad_ctx
 * [B][ndf][S].  Each (image, caption) pair is recomputed by one workgroup; the per-pair gradients are summed in a
 * fixed order (deterministic).  ws: tgsr_damsm_words_bwd_ws_elems(B, ndf, S) floats.  ndf % 32 == 0, ndf <= 256,
 * Tw <= 32, S <= 320.
 */
int64_t tgsr_damsm_words_bwd_ws_elems(int B, int ndf, int S);
int tgsr_damsm_words_bwd(const float* words, const int32_t* cap_lens, const float* ctx, const float* grad_sim, int B,
                         int ndf, int Tw, int S, float gamma1, float gamma2, float* ws, float* grad_words32,
                         float* grad_ctx, void* stream);

/*
 * Stand-alone func_attention(query, context, gamma1) (GlobalAttention.py:33-74): pair p attends query p to context p.
 * query [B][ndf][L] (L <= 32), context [B][ndf][S] (S <= 320) -> weighted_context [B][ndf][L], attn [B][L][S].
 */
int tgsr_func_attention_fwd(const float* query, const float* context, int B, int ndf, int L, int S, float gamma1,
                            float* weighted_context, float* attn, void* stream);

/*
 * Text-image retrieval (csrc/tgsr_retrieval.hip): N images scored against a candidate list of captions each.  Evaluation only, no
 * backward.  No allocation, no synchronisation, no atomics (the same bits on every run); everything on `stream`, capturable.
 * cand int32 [N][K] holds caption indices into a pool of M, or is NULL (then K must equal M and cand[n][k] = k).  A cand entry
 * outside [0, M) is an EMPTY slot: nothing is read for it and sim = -inf.  N, M, K >= 1.
 *
 * tgsr_damsm_gallery_fwd  sim[n][k] = words_similarity of image n and caption cand[n][k] (losses.py:251-287, one entry per pair;
 *     the value tgsr_damsm_words_fwd gives the pair, before gamma3).  words [M][ndf][Tw], cap_lens int32 [M] or NULL (= Tw; clamped
 *     into [1, Tw] like tgsr_damsm_words_fwd), ctx [N][ndf][S].  Limits as tgsr_damsm_words_fwd: ndf % 32 == 0, 32 <= ndf <= 512,
 *     Tw <= 32, S <= 320 (TGSR_EUNSUPPORTED otherwise).  One workgroup scores two neighbouring columns of a row; two captions of at
 *     most 16 words share one MFMA tile.  sim for an (image, caption) pair is the same bits wherever the pair stands in cand.
 * tgsr_sent_gallery_fwd   sim[n][k] = gamma3 * <cnn[n], rnn[c]> / max(|cnn[n]| * |rnn[c]|, eps), c = cand[n][k]  (losses.py:234-250);
 *     cnn [N][ndf], rnn [M][ndf], ndf >= 1.
 * tgsr_retrieval_ranks    rank[n] = #{k : sim[n][k] > sim[n][t]} + #{k < t : sim[n][k] == sim[n][t]}, t = target[n]: the position of
 *     column t in a stable descending sort of row n; target[n] outside [0, K) -> rank[n] = -1.  sim [N][K] row-major, K >= 1.
 */
int tgsr_damsm_gallery_fwd(const float* words, const int32_t* cap_lens, const float* ctx, const int32_t* cand, int N, int M,
                           int K, int ndf, int Tw, int S, float gamma1, float gamma2, float* sim, void* stream);
int tgsr_sent_gallery_fwd(const float* cnn, const float* rnn, const int32_t* cand, int N, int M, int K, int ndf, float eps,
                          float gamma3, float* sim, void* stream);
int tgsr_retrieval_ranks(const float* sim, const int32_t* target, int N, int K, int32_t* rank, void* stream);

/*
 * Distribution distances (csrc/tgsr_featdist.hip): the statistics behind the Frechet and the kernel distance of two feature sets
 * (tgsr_amd/featdist.py finishes them).  Evaluation only, no backward.  Features are float32 and are widened to fp64 on read
 * (exact; the product of two widened values is exact in fp64); every sum is an fp64 sum on v_mfma_f64_16x16x4_f64 or an fp64 add
 * in an order the shapes alone fix.  No allocation, no synchronisation, no atomics: the same bits on every run; everything on
 * `stream`, capturable.
 *
 * tgsr_feat_moments_add   sum[i] += sum_r x[r][i],   outer[i][j] += sum_r x[r][i] x[r][j]   (X^T X, the contraction over the rows).
 *     x float32 [n][D] with row stride ldx >= D floats, sum fp64 [D], outer fp64 [D][D] row-major; any n >= 1, D >= 1 (D <= 64 *
 *     65535).  DEFINED ELEMENTS OF outer: the block-upper part, i / 64 <= j / 64 (it contains the upper triangle i <= j); the
 *     elements below the block diagonal are neither read nor written.  A reader mirrors the upper triangle (featdist.py does).
 *     One launch: a read-modify-write of the block-upper part, each element owned by one lane.
 * tgsr_poly_mmd_sums      S subsets of m rows each: subset s takes rows ix[s][0..m) of x and iy[s][0..m) of y (int32 tables
 *     [S][m]; x float32 [nx][D] stride ldx, y float32 [ny][D] stride ldy).  With k(a, b) = (<a, b> / D + 1)^3 in fp64:
 *       out[s][0] = sum_{i != j} k(x_i, x_j),   out[s][1] = sum_{i != j} k(y_i, y_j),   out[s][2] = sum_{i, j} k(x_i, y_j),
 *     i, j POSITIONS in the subset (a row listed twice is two items).  out fp64 [S][3], written completely.  The m x m kernel
 *     matrix is never stored: each 64 x 64 tile leaves one partial in `work` (tgsr_poly_mmd_ws_elems(S, m) doubles; 0 = a
 *     shape the entry refuses), a second launch adds a sum's partials in tile order.  out[s] depends on the subset's rows alone,
 *     not on s or on the other subsets.  Any m >= 2, S >= 1 (<= 65535), D >= 1.  A table entry outside [0, nx) / [0, ny) is
 *     outside the contract and is checked on the host, where the table is made (ops.poly_mmd_sums); the kernel forms no
 *     address from it and scores the item as a row of zeros.
 * Both return TGSR_EINVAL without launching (and without touching an output) for a NULL pointer, n < 1, nx < 1, ny < 1, S < 1, m < 2,
 * D < 1 or a row stride below D.
 */
int tgsr_feat_moments_add(const float* x, int n, int D, int64_t ldx, double* sum, double* outer, void* stream);
int64_t tgsr_poly_mmd_ws_elems(int S, int m);
int tgsr_poly_mmd_sums(const float* x, int nx, int64_t ldx, const float* y, int ny, int64_t ldy, const int32_t* ix,
                       const int32_t* iy, int S, int m, int D, double* work, double* out, void* stream);

/*
 * The two trainable heads of CNN_ENCODER (util.py:300-301, 364-367) as fp32 MFMA GEMMs with bias:
 * tgsr_conv1x1_fwd : emb_features, conv1x1 Cin -> Cout on [B][Cin][S] (S = ih*iw, 17*17) -> out [B][Cout][S]
 * tgsr_linear_fwd  : emb_cnn_code, out[b][o] = sum_k w[o][k] x[b][k] + bias[o]; x [B][K], w [Cout][K]
 * bias may be NULL.  (The Inception-v3 trunk that produces their inputs is third-party torchvision arithmetic.)
 */
int tgsr_conv1x1_fwd(const float* x, int B, int Cin, int S, const float* w, const float* bias, int Cout, float* out,
                     void* stream);
int tgsr_linear_fwd(const float* x, int B, int K, const float* w, const float* bias, int Cout, float* out,
                    void* stream);

/*
 * The discriminators' logit heads (nn.Conv2d(8 ndf, 1, kernel_size=4, stride=4) on a 4x4 map, called by
 * losses.py:292-316 / 359-366 as netD.COND_DNET / UNCOND_DNET): out[b] = sum_k x[b][k] w[k] + bias[0], one workgroup
 * per sample, fixed-order reduction.  Backward: dx[b][k] = dy[b] w[k] (dx may be NULL), dw[k] = sum_b dy[b] x[b][k]
 * (dw may be NULL).  Forward: x, w 16-byte aligned, at every K - one off is refused with TGSR_EUNSUPPORTED, also where K % 4 != 0
 * and the kernel would read single floats.  The backward reads and writes single floats: a float's alignment is enough.
 */
int tgsr_rowdot_fwd(const float* x, const float* w, const float* bias, float* out, int B, int K, void* stream);

/*
 * CA_NET.forward (util.py:372-400) in one launch: x = fc(sent_emb) (w [4 ncf][tdim], bias [4 ncf]); GLU halves;
 * mu = h[:ncf], logvar = h[ncf:] ([B][ncf] each); c_code = eps * exp(0.5 * logvar) + mu with eps [B][ncf] standard
 * normals drawn by the caller (the reference draws them from torch's generator, util.py:388-396).  c_code and eps may
 * both be NULL (the x8 generators discard c_code, model.py:51-52).
 * Two kernels, chosen by tdim and by the alignment of sent_emb and w (every other operand is read by single floats):
 *   tdim % 16 == 0, and for tdim % 64 == 0 sent_emb and w both 16-byte aligned: the MFMA form (16 samples x 4 channels per
 *     workgroup; float4 operand loads when tdim % 64 == 0, single floats otherwise) - the form tgsr_text_tail_fwd runs;
 *   every other tdim, and tdim % 64 == 0 with sent_emb or w off 16 bytes: the row-per-thread form, which keeps tdim + 4 ncf + 8
 *     floats in LDS and is refused with TGSR_EUNSUPPORTED when (tdim + 4 ncf) * 4 bytes exceed 60 KB; it reads w by float4 when
 *     tdim % 8 == 0 and w is 16-byte aligned, by single floats otherwise.
 * The two forms sum in different orders: the same values within rounding, not the same bits.
 */
int tgsr_ca_net_fwd(const float* sent_emb, const float* w, const float* bias, const float* eps, int B, int tdim, int ncf,
                    float* c_code, float* mu, float* logvar, void* stream);
int tgsr_rowdot_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int K, void* stream);

/*
 * The text tail of an inference step in ONE launch (trainer_objective.py:134-146 between the text encoder and the
 * generator): the conv_context projections of tgsr_word_project_fwd (src_out [nsets][B][idf][32]), CA_NET's mu / logvar
 * [B][ncf] of tgsr_ca_net_fwd (same arithmetic; c_code is not produced - the x8 / x16 generators discard it,
 * model.py:51-52) and mask[B][T] = (captions[b][t] == 0) as bytes 0 / 1 (trainer_objective.py:136-140; torch.bool storage).
 * captions int64 [B][width], width >= T.  tdim % 16 == 0 (sent_emb / ca_w 16-byte aligned when tdim % 64 == 0); other
 * limits as tgsr_word_project_fwd.
 */
int tgsr_text_tail_fwd(const float* words, const float* const* w_ctx, int nsets, int B, int idf, int cdf, int T,
                       float* src_out, const float* sent_emb, const float* ca_w, const float* ca_b, int tdim, int ncf,
                       float* mu, float* logvar, const int64_t* captions, int width, uint8_t* mask, void* stream);

/*
 * tgsr_text_tail_fwd that ALSO leaves what the reduced-precision generators need to attend to the words inside the kernels
 * that produce h (tgsr_lp_stem_att_fwd, tgsr_lp_upconv_glu_att_fwd): `att_pack`, tgsr_lp_att_pack_bytes(nsets, B) bytes,
 * 16-byte aligned =
 *     [nsets][B][4 fragments][64 lanes][8] elements of `lp_dtype`: the projections src_out rounded once and laid out as
 *         the MFMA 32x32x16 A fragments of the scores GEMM (0, 1) and the context GEMM (2, 3);
 *     [B] uint32: bit t = (captions[b][t] == 0), t < T.
 * idf must be 32 (the generators' ngf).  src_out / mu / logvar / mask as tgsr_text_tail_fwd, bit-identical.
 * Fragment f, lane l, element j holds src[i][t] with (i, t) = (16 f + 8 (l >> 5) + j, l & 31) for f < 2 and
 * (l & 31, 16 (f - 2) + 8 (j >> 2) + 4 (l >> 5) + (j & 3)) for f >= 2; every element and every mask word is written.
 */
int64_t tgsr_lp_att_pack_bytes(int nsets, int B);
int tgsr_text_tail_lp_fwd(const float* words, const float* const* w_ctx, int nsets, int B, int idf, int cdf, int T,
                          float* src_out, const float* sent_emb, const float* ca_w, const float* ca_b, int tdim, int ncf,
                          float* mu, float* logvar, const int64_t* captions, int width, uint8_t* mask, int lp_dtype,
                          void* att_pack, void* stream);

/*
 * n <= 16 dense device-to-device copies in one launch: dst / src / nbytes are HOST arrays; sizes and addresses must be
 * multiples of 4 bytes.  (GraphedStep.replay: the new inputs of every lane go into the captured step's static buffers
 * with one launch instead of three hipMemcpyAsync per lane.)
 */
int tgsr_multi_copy(int n, void* const* dst, const void* const* src, const int64_t* nbytes, void* stream);

/*
 * The gradient collective of the data-parallel path behind the C ABI (`allreduce_flat`, an RCCL wrapper; the
 * reference has no collective - trainer_objective.py:31 is single-process).  tgsr_allreduce_flat: buf[i] = scale * sum over ranks
 * of buf[i], in place, n floats, asynchronous on `stream` (ncclAllReduce, then one scaling launch unless scale == 1) - what
 * tgsr_amd.parallel.FlatGradBucket.all_reduce_mean does through torch.distributed by default.  Communicators: rank 0 calls
 * tgsr_comm_unique_id(id) (128 bytes), the caller carries those bytes to every rank, every rank calls tgsr_comm_init(&comm, id,
 * rank, world) with its device current; tgsr_comm_destroy(comm) at the end.  librccl is opened lazily (dlopen): where it is absent
 * tgsr_comm_available() returns 0 and the other four return TGSR_EUNSUPPORTED - the rest of the library is unaffected.
 */
int tgsr_comm_available(void);
int tgsr_comm_unique_id(void* id128);
int tgsr_comm_init(void** comm, const void* id128, int rank, int world);
int tgsr_allreduce_flat(void* comm, float* buf, int64_t n, float scale, void* stream);
int tgsr_comm_count(void* comm, int* world, int* rank); /* ncclCommCount / ncclCommUserRank of a communicator: what RCCL itself says */
int tgsr_comm_destroy(void* comm);

/*
 * out[i] = t[i] + alpha * s[i] for n <= 4 dense fp32 images in one launch (host arrays of device pointers; numel[i] a
 * multiple of 4, pointers 16-byte aligned).  The second half of NetG_highweight's heads (model.py:280, 288, 297:
 * `ims = one * conv_output(out) + a * SRb`): the caller computes t = tanh(conv5x5(out)) with tgsr_conv_to3_fwd(addend = NULL)
 * on the high-frequency branch's own stream - it needs nothing of G_SR_NET_low - and only this axpy waits for the
 * low-frequency images.  fma(alpha, s, t), exactly what tgsr_conv_to3_fwd's epilogue evaluates when given the addend.
 */
int tgsr_axpy_images(int n, float* const* out, const float* const* t, const float* const* s, const int64_t* numel, float alpha,
                     void* stream);

/*
 * NetG_highweight(weightmap=True) (model.py:235-245, 276-297; models16.py:119-125, 149-178): `ims_k = one_k * conv_output(out) +
 * a_k * SRb_k` with a_k a trainable [H, W] map (initial value 1) broadcast over batch and channels.
 *   fwd: out[bc][p] = t[bc][p] + amap[p] * s[bc][p]     (t = conv_output(out): tgsr_conv_to3_fwd without addend)
 *   bwd: ds = amap * dy (ds may be NULL), damap[p] = sum_bc dy[bc][p] * s[bc][p] (damap may be NULL), planes added in index order.
 * BC = B * 3 planes of HW pixels, dense; HW % 4 == 0, pointers 16-byte aligned (else TGSR_EUNSUPPORTED).
 */
/* ------------------------------------------------------------------------------------------------------------------
 * CNN_ENCODER's frozen Inception-v3 trunk (util.py:263-368, every parameter `requires_grad = False`, util.py:274-275; run by
 * generator_loss for the DAMSM ranking term, losses.py:375-389): forward and the gradient with respect to the image.
 *
 * tgsr_gconv: a convolution of any KH x KW (KH KW <= 64), stride 1 | 2, zero padding, as one implicit GEMM on the fp32 MFMA.
 *   dgrad = 0  forward.  A = w' [M = Cout][K = Cin KH KW] (tgsr_gconv_pack(dgrad = 0): the filter times the folded BatchNorm scale),
 *              S = x based at its first channel, [B] samples `s_bstride` floats apart, Hs x Ws pixels; pixel grid PH x PW = the
 *              OUTPUT size; out[b][m][PH][PW] (+)= relu?(sum + bias[m]) based at the output's channel slice, samples
 *              `o_bstride` apart (a block's branches write straight into their slices of its concatenation).
 *   dgrad = 1  data gradient.  A = w'T [M = Cin][K = Cout KH KW] (tgsr_gconv_pack(dgrad = 1)), S = g = d(loss)/d(pre-activation) with
 *              the forward's OUTPUT size Hs x Ws, pixel grid PH x PW = the forward's INPUT size; out = dx (accumulate = 1: +=,
 *              a block input collects its branches' gradients one after the other).  bias / relu must be 0.
 *   mask (nullable; laid out like `out`, same batch stride): the contribution is kept where mask > 0 and dropped elsewhere - the
 *              ReLU of the tensor whose gradient is being written (a 0 / 1 factor distributes over the sum of a tensor's consumers,
 *              so every consumer applies it to its own contribution and no separate mask pass runs).  Also on the pool backwards.
 *   ws: tgsr_gconv_ws_elems(B, M, PH, PW, K) floats (0 when the shape is not split over K: NULL is accepted).  Deterministic (slabs
 *              summed in order).
 *   Alignment: every operand - A, S, bias, mask, out, ws, and tgsr_gconv_pack's w, scale, out - needs 4 bytes.  The three-piece form
 *              (tgsr_gconv_set_form) loads A 16 bytes at a time: an A off 16 bytes is served by the fp32 MFMA (dword loads); S, mask and
 *              out are read and written by dwords in both forms, so a channel slice and an odd batch stride need no more.
 * tgsr_maxpool3s2_*: F.max_pool2d(x, 3, stride 2); the backward routes dy to the FIRST maximum of a window (torch's rule).
 * tgsr_avgpool3: F.avg_pool2d(x, 3, 1, 1) (count_include_pad); symmetric, so it is also its own backward (accumulate = 1).
 * tgsr_plane_mean(_bwd): the 8 x 8 global average (F.avg_pool2d(x, 8) on an 8 x 8 map).  tgsr_relu_mask: out = dy * (y > 0).
 * tgsr_bilinear_*: nn.Upsample(size = (OH, OW), mode = 'bilinear') (align_corners = False), util.py:310, on dense planes.
 * Alignment: the pools, tgsr_relu_mask, tgsr_interleave2x2, tgsr_plane_mean(_bwd) and tgsr_bilinear_* read and write by dwords: every
 * pointer needs 4 bytes, every batch stride may be odd.  (tgsr_sum_stack: 16 bytes, below.)
 */
/*
 * tgsr_gconv_set_form: 1 (default; TGSR_GCONV_SPLIT=0 in the environment turns it off): tgsr_gconv / tgsr_gconv_stats run on the bf16
 * matrix pipe with exact three-piece fp32 operands where K % 16 == 0, KH KW <= 25 taps, the data gradient at stride 1, A 16-byte
 * aligned and S within 2^31 bytes; 0: fp32 MFMA everywhere.  Returns the old value.  Process-wide, and it is one of TWO switches in
 * front of that form: tgsr_dconv_set_split(0) takes the generic taps off it as well.
 */
int tgsr_gconv_set_form(int split);
/*
 * tgsr_sum_stack: out[k] = ((parts[0][k] + parts[1][k]) + ...) over n dense tensors of m floats stacked back to back (m % 4 == 0, 16-byte aligned):
 * the branches' contributions to a Mixed block's input gradient (util.py:281-298's blocks), each written by its own branch's stream,
 * summed in the order a one-stream walk accumulates them.
 */
int tgsr_sum_stack(const float* parts, int n, int64_t m, float* out, void* stream);

/*
 * dx[b][c][2Y + py][2X + px] (+)= t_{py px}[b][c][Y][X] over `planes` = B * C dense planes of H x W: weaves the four parity classes of
 * a stride-2 convolution's data gradient - each a stride-1 data gradient over its own taps (tgsr_gconv), dense at half resolution,
 * ceil((H - py) / 2) x ceil((W - px) / 2) pixels - into the gradient of the input (util.py:281-298's stride-2 layers: a quarter of the
 * products of the direct form).  mask (dense, like dx) keeps the value where mask > 0; accumulate != 0 adds.
 */
int tgsr_interleave2x2(const float* t00, const float* t01, const float* t10, const float* t11, float* dx, int64_t planes, int H, int W,
                       int accumulate, const float* mask, void* stream);

/* The planners of tgsr_gconv (host arithmetic, reads of the one launch plan): the K slabs the fill heuristic asks for at GEMM size
 * M x N x K (1 = no split; TGSR_GCONV_FILL) and the workspace they take.  They depend on neither switch. */
int tgsr_gconv_nsplit(int M, int N, int K);
int64_t tgsr_gconv_ws_elems(int B, int M, int PH, int PW, int K);
int tgsr_gconv(int dgrad, const float* A, const float* S, int64_t s_bstride, int B, int Hs, int Ws, int M, int K, int PH, int PW,
               int KH, int KW, int stride, int padh, int padw, const float* bias, int relu, int accumulate, const float* mask,
               float* out, int64_t o_bstride, float* ws, void* stream);
int tgsr_gconv_pack(const float* w, const float* scale, float* out, int Cout, int Cin, int KK, int dgrad, void* stream);
/*
 * Training mode (pretrain_DAMSM.py:49-51 runs the frozen trunk with batch-statistics BatchNorm), one conv + BN + ReLU layer in two
 * launches (three where K is split):
 * tgsr_gconv_stats: tgsr_gconv(dgrad = 0, bias = NULL, relu = 0, accumulate = 0, mask = NULL) - the raw convolution, bit-identical to
 *   that call in the same arithmetic form, into its channel slice - that also writes stat_partial [M][nslots][2]: per output channel
 *   and slot of slot_px pixels (the GEMM's N tile, or 2048 pixels when K is split and the slab finish takes them; the last slot holds
 *   the rest) the pair (sum, sum of squared deviations from the slot's mean), pixels past N excluded, fixed slots and order (no
 *   atomics).  nslots / slot_px = tgsr_gconv_stats_nslots / tgsr_gconv_stats_slot_pixels(B, M, PH, PW, K); ws as for tgsr_gconv.
 * tgsr_bn_train_relu_slice_from_stats: in place over C channels of HW pixels based at the slice (samples bstride floats apart):
 *   y = relu((y - mean) * scale + beta) with the batch statistics combined from stat_partial (Chan's formula, double precision, a
 *   fixed order); writes stats [4][C] (mean,
 *   invstd, scale, shift), updates running_mean / running_var (momentum, unbiased variance; both NULL: none) and
 *   num_batches_tracked (nullable) once.  Alignment: stat_partial (read a (sum, M2) pair at a time) and num_batches_tracked 8 bytes,
 *   else TGSR_EUNSUPPORTED; y, gamma, beta, the running statistics and stats 4 bytes.  tgsr_gconv_stats itself writes stat_partial by
 *   dwords.
 */
int tgsr_gconv_stats_nslots(int B, int M, int PH, int PW, int K);
int tgsr_gconv_stats_slot_pixels(int B, int M, int PH, int PW, int K);
int tgsr_gconv_stats(const float* A, const float* S, int64_t s_bstride, int B, int Hs, int Ws, int M, int K, int PH, int PW, int KH,
                     int KW, int stride, int padh, int padw, float* out, int64_t o_bstride, float* ws, float* stat_partial,
                     void* stream);
int tgsr_bn_train_relu_slice_from_stats(float* y, int64_t bstride, int B, int C, int HW, const float* gamma, const float* beta,
                                        float eps, float momentum, float* running_mean, float* running_var,
                                        const float* stat_partial, int nslots, int slot_px, float* stats,
                                        int64_t* num_batches_tracked, void* stream);
int tgsr_maxpool3s2_fwd(const float* x, int64_t x_bstride, int B, int C, int H, int W, float* out, int64_t o_bstride, void* stream);
int tgsr_maxpool3s2_bwd(const float* x, int64_t x_bstride, const float* dy, int64_t dy_bstride, int B, int C, int H, int W, float* dx,
                        int64_t dx_bstride, int accumulate, const float* mask, void* stream);
int tgsr_avgpool3(const float* x, int64_t x_bstride, int B, int C, int H, int W, float* out, int64_t o_bstride, int accumulate,
                  const float* mask, void* stream);
int tgsr_plane_mean(const float* x, float* out, int64_t planes, int HW, void* stream);
int tgsr_plane_mean_bwd(const float* dy, float* dx, int64_t planes, int HW, void* stream);
int tgsr_relu_mask(const float* dy, int64_t dy_bstride, const float* y, int64_t y_bstride, float* out, int64_t o_bstride, int B,
                   int64_t per_sample, void* stream);
int tgsr_bilinear_fwd(const float* x, int64_t planes, int H, int W, int OH, int OW, float* out, void* stream);
int tgsr_bilinear_bwd(const float* dy, int64_t planes, int H, int W, int OH, int OW, float* dx, void* stream);

/*
 * The adversarial terms of discriminator_loss / generator_loss (losses.py:290-316, 358-371) in one launch: out[0] = sum_i
 * weight[i] * BCEWithLogits(l[i], target[i]) over l = [a (na logits); b (nb logits, may be NULL / 0)] - the reference's up to five
 * mean-reduced nn.BCEWithLogitsLoss calls with their 1/n means and /2, /3 combination folded into `weight`.  One workgroup, fixed
 * summation order.  bwd: da / db = dy[0] * weight * (sigmoid(l) - target) (either may be NULL).
 */
int tgsr_weighted_bce_fwd(const float* a, int na, const float* b, int nb, const float* target, const float* weight, float* out,
                          void* stream);
int tgsr_weighted_bce_bwd(const float* dy, const float* a, int na, const float* b, int nb, const float* target, const float* weight,
                          float* da, float* db, void* stream);

/*
 * Adam over flat fp32 buffers (torch.optim.Adam's update, trainer_objective.py's optimizers: no amsgrad; weight_decay = L2 added to
 * the gradient), one pass: param, grad, exp_avg, exp_avg_sq are dense buffers of n floats, 16-byte aligned.  state = 3 device
 * floats [step, 1 - beta1^step, sqrt(1 - beta2^step)]: advance != 0 first bumps the step and recomputes the two corrections on the
 * device (a one-thread launch: the count survives hipGraph replays); a caller with several parameter ranges advances once and
 * passes advance = 0 for the others.  The hyper-parameters arrive as the doubles the caller holds: 1 - beta is rounded to fp32 from
 * the double difference, as torch does (1.f - 0.999f is 4.7e-5 away from 0.001f).
 */
int tgsr_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* state, int64_t n, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int advance, void* stream);

int tgsr_axpy_map_fwd(const float* t, const float* s, const float* amap, float* out, int BC, int HW, void* stream);
int tgsr_axpy_map_bwd(const float* dy, const float* s, const float* amap, float* ds, float* damap, int BC, int HW, void* stream);

/*
 * Eval-mode BatchNorm2d + activation on a raw convolution output, dense NCHW: out = act(raw * scale[c] + shift[c]) with
 * scale / shift from tgsr_bn_fold (running statistics) - downBlock / Block3x3_leakRelu under .eval() (util.py:92-98; the
 * train-mode form is tgsr_bn_train_fwd).  act: 0 none, 2 LeakyReLU(0.2) (the selector values of tgsr_bn_train_fwd's `glu`).
 * bwd: draw = dy * act'(out) * scale[c] (out = the forward output; may be NULL for act 0).  HW % 4 == 0, 16-byte aligned.
 */
int tgsr_affine_act_fwd(const float* raw, const float* scale, const float* shift, float* out, int B, int C, int HW, int act,
                        void* stream);
int tgsr_affine_act_bwd(const float* dy, const float* out, const float* scale, float* draw, int B, int C, int HW, int act,
                        void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training path (BatchNorm2d batch statistics + backward).  The reference trains through torch autograd over
 * nn.Conv2d / nn.BatchNorm2d(train) / GLU / nn.Upsample (util.py:74-80, 110-130); these entry points are the
 * hand-written forward/backward of the same blocks.
 * ------------------------------------------------------------------------------------------------------------------ */

/* Number of partial-sum splits tgsr_bn_train_* use for (B, C, HW); partial_ws must hold C * nsplit * 4 floats. */
/*
 * Small layers (one workgroup per channel covers the batch: B * HW < 8192, no GLU - the discriminators' 16^2 .. 4^2 maps) run the
 * statistics / reduce pass INSIDE the normalise / apply kernel: one launch instead of two, bit-identical results.
 * tgsr_bn_set_fuse_small(on): default on (TGSR_BN_FUSE_SMALL=0 in the environment turns it off); returns the previous setting.
 */
int tgsr_bn_set_fuse_small(int on);
int tgsr_bn_train_nsplit(int B, int C, int HW);

/*
 * nn.BatchNorm2d in training mode (+ GLU | + residual) on the raw conv output: batch mean / biased variance per
 * channel over (B, H, W), running statistics updated in place with `momentum` and the unbiased variance (either
 * both NULL or both given), y = GLU(bn(raw)) (glu=1, C even, out has C/2 channels) or bn(raw) (+ residual).
 * `glu` is the activation selector: 0 = none (+ residual), 1 = GLU, 2 = LeakyReLU(0.2) (downBlock util.py:92-98 and
 * the discriminators' conv3x3 -> BN -> LeakyReLU blocks; no residual).
 * raw [B][C][HW] dense, HW % 4 == 0.  Saves mean/invstd/scale/shift [C] for the backward.  num_batches_tracked (device
 * int64 scalar, may be NULL) is incremented by one, as nn.BatchNorm2d.forward does in training mode.
 */
int tgsr_bn_train_fwd(const float* raw, int B, int C, int HW, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, int glu, const float* residual,
                      int64_t res_bstride, float* partial_ws, float* mean, float* invstd, float* scale, float* shift,
                      float* out, int64_t out_bstride, int64_t* num_batches_tracked, void* stream);

/*
 * The statistics pass folded into the producing convolution.  tgsr_wino_conv3x3_stats_fwd = tgsr_wino_conv3x3_fwd with the
 * plain epilogue (no affine, no residual: the raw output BatchNorm's batch statistics are taken of) that also writes
 * stat_partial [Cout][nslots][2]: one (sum, sum of squares) pair per channel and wave tile, nslots =
 * tgsr_wino_stats_nslots(B, H, W, Cout).  tgsr_bn_train_fwd_from_stats = tgsr_bn_train_fwd without its pass over the raw
 * tensor: it combines those pairs (double precision, fixed order) instead.
 */
int tgsr_wino_stats_nslots(int B, int H, int W, int Cout);
int tgsr_wino_conv3x3_stats_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack,
                                int Cout, float* out, int64_t out_bstride, float* stat_partial, void* stream);
/* The same for the F(4x4, 3x3) kernel (training forward of the 128 x 128 layers): one pair per channel and 4 x 64 wave tile. */
int tgsr_wino4_stats_nslots(int B, int H, int W, int Cout);
int tgsr_wino4_conv3x3_stats_fwd(const float* x, int64_t x_bstride, int B, int Cin, int H, int W, const float* upack,
                                 int Cout, float* out, int64_t out_bstride, float* stat_partial, void* stream);
int tgsr_bn_train_fwd_from_stats(const float* raw, int B, int C, int HW, const float* gamma, const float* beta, float eps,
                                 float momentum, float* running_mean, float* running_var, int glu, const float* residual,
                                 int64_t res_bstride, const float* stat_partial, int nslots, float* mean, float* invstd,
                                 float* scale, float* shift, float* out, int64_t out_bstride, int64_t* num_batches_tracked,
                                 void* stream);

/*
 * Backward of the above: dout [B][C or C/2][HW] dense -> draw [B][C][HW] (gradient wrt the raw conv output),
 * dgamma, dbeta [C].  The gradient wrt a residual input is dout itself.  sums_ws: no longer used (the apply pass combines
 * the partials itself); any non-NULL pointer, e.g. partial_ws.
 */
int tgsr_bn_train_bwd(const float* dout, const float* raw, int B, int C, int HW, const float* scale,
                      const float* shift, const float* mean, const float* invstd, int glu, float* partial_ws,
                      float* sums_ws, float* draw, float* dgamma, float* dbeta, void* stream);

/*
 * The discriminators' convolutions: downBlock's nn.Conv2d(Cin, Cout, 4, 2, 1, bias=False) (util.py:92-98) and the 3x3
 * stride-1 pad-1 convolutions of their 4x4-pixel, 512...2048-channel blocks, as one fp32 MFMA implicit-GEMM kernel
 * (128 x 128 x 16 LDS tiles, operands gathered from the NCHW tensors by index arithmetic - no im2col buffer; the
 * reduction is split into slabs where M x N alone cannot fill the chip, summed in a fixed order: reproducible, no
 * float atomics).  H, W = INPUT size (even for the 4x4 form); out / dy [B][Cout][H/2][W/2] (4x4) or [B][Cout][H][W]
 * (3x3), dense; w in torch layout.  BatchNorm + LeakyReLU behind it = tgsr_bn_train_fwd(glu = 2); `act` = 1 applies
 * LeakyReLU(0.2) in the epilogue (the discriminators' first layer has no BatchNorm).
 *   *_fwd   out = conv(x, w)              *_dgrad  dx = conv_transpose(dy, w)          *_wgrad  dw = sum_pixels dy x_gather
 * ws: *_ws_elems(op, ...) floats with op = 0 forward, 1 data gradient, 2 weight gradient (slabs; for the 4x4 data
 * gradient also the per-parity-class weight regrouping, rebuilt by every call: weights change per step).
 * Alignment: every operand - x, w, dy, ws, out / dx / dw - needs 4 bytes; no call is refused for an address.  The three-piece form
 * (tgsr_dconv_set_split) loads its A operand 16 bytes at a time - w and the head of ws (forward, 4x4 data gradient), dy (weight
 * gradients); the 3x3 data gradient reads w by dwords - and a call whose A is off 16 bytes is served by the fp32 MFMA, all dword
 * accesses, with the bits of tgsr_dconv_set_split(0); the 4x4 data gradient then also regroups the weight one float at a time (the
 * same packed bits).  The gathered tensor and the output are dword accesses in both forms.  The image layer's data gradient
 * (Cin <= 4) stores dx in pairs where dx is 8-byte aligned and one float at a time where not: the same bits.
 * The generator's 3x3 convolutions (32 ... 128 channels on 32^2 ... 256^2 pixels) are tgsr_wino_conv3x3_fwd /
 * tgsr_conv3x3_fwd, not these.
 * tgsr_leaky_relu: out = x > 0 ? x : 0.2 x, or with y_for_bwd != NULL the backward out = x * (y > 0 ? 1 : 0.2); dword accesses.
 * tgsr_dconv_set_split(on): on != 0 (the default; TGSR_DCONV_SPLIT=0 in the environment turns it off) lets the GEMMs of both
 * forms run on the bf16 matrix pipe with every fp32 operand split exactly into three bf16 pieces and six of the nine piece
 * products accumulated in fp32 (what is left out is <= 2^-26 of a product; measured error against fp64: below the fp32 MFMA's) -
 * fp32 in, fp32 out, 2.4x the fp32 MFMA rate; shapes it does not take (K % 16 != 0, ...) and on == 0 use the fp32 MFMA.
 * Returns the previous setting.  Process-wide; not meant to be flipped while launches are being issued from other threads.
 * on == 0 also takes the Inception trunk's generic taps (tgsr_gconv, tgsr_gconv_stats) off that form: it is the same kernel.
 */
int tgsr_dconv_set_split(int on);
/* 1 when tgsr_conv4x4s2_{fwd (op 0), dgrad (1), wgrad (2)} takes the split form for this shape under the current setting: what a
 * caller's bookkeeping needs to price a launch.  These and *_ws_elems read the launchers' own plan, evaluated for 16-byte aligned
 * operands (the calls themselves test w and ws - forward, 4x4 data gradient - or dy - weight gradient - and serve an operand off 16
 * bytes on the fp32 MFMA: see "Alignment" above) and bounding the convolution's tensors, not the kernel's operands, by 4 GB.
 * An op outside 0..2 or a shape the calls refuse: split_form 0, ws_elems 0. */
int tgsr_conv4x4s2_split_form(int op, int B, int Cin, int H, int W, int Cout);
int tgsr_conv3x3_gemm_split_form(int op, int B, int Cin, int H, int W, int Cout);
int64_t tgsr_conv4x4s2_ws_elems(int op, int B, int Cin, int H, int W, int Cout);
int tgsr_conv4x4s2_fwd(const float* x, int B, int Cin, int H, int W, const float* w, int Cout, int act, float* ws,
                       float* out, void* stream);
int tgsr_conv4x4s2_dgrad(const float* dy, int B, int Cin, int H, int W, const float* w, int Cout, float* ws, float* dx,
                         void* stream);
int tgsr_conv4x4s2_wgrad(const float* dy, const float* x, int B, int Cin, int H, int W, int Cout, float* ws, float* dw,
                         void* stream);
int64_t tgsr_conv3x3_gemm_ws_elems(int op, int B, int Cin, int H, int W, int Cout);
int tgsr_conv3x3_gemm_fwd(const float* x, int B, int Cin, int H, int W, const float* w, int Cout, float* ws, float* out,
                          void* stream);
int tgsr_conv3x3_gemm_dgrad(const float* dy, int B, int Cin, int H, int W, const float* w, int Cout, float* ws, float* dx,
                            void* stream);
int tgsr_conv3x3_gemm_wgrad(const float* dy, const float* x, int B, int Cin, int H, int W, int Cout, float* ws, float* dw,
                            void* stream);
int tgsr_leaky_relu(const float* x, const float* y_for_bwd, float* out, int64_t n, void* stream);

/*
 * GLU.forward (util.py:45-53) as a stand-alone op - inside the conv blocks it is the producing kernel's epilogue; the
 * module itself is callable upstream (CA_NET, util.py:381).  x viewed as [outer][2][half] (the two channel halves of
 * [B, 2C, ...]: outer = B, half = C * inner), dense fp32.  dy == NULL: out[outer][half] = x[.][0][.] * sigmoid(x[.][1][.]);
 * dy [outer][half] != NULL: the backward, out = dx [outer][2][half].
 */
int tgsr_glu(const float* x, const float* dy, float* out, int64_t outer, int64_t half, void* stream);

/*
 * Backward of nn.Upsample(scale_factor=2, 'nearest'): out[bc][y][x] = sum of in[bc][2y..2y+1][2x..2x+1], x dense [BC][2H][2W],
 * out dense [BC][H][W].  x needs no more than a float's alignment: the kernel reads pairs with 8-byte loads where x is 8-byte
 * aligned and single floats where it is not, (x00 + x01) + (x10 + x11) either way - the same bits.
 */
int tgsr_sumpool2x2(const float* x, int64_t BC, int H, int W, float* out, void* stream);

/*
 * uint8 image epilogue of the reference's caller (trainer_objective.py:153-155):
 * out[i] = round(clip((x[i] + 1) * 127.5, 0, 255)), float32 arithmetic and round-half-to-even exactly as the numpy
 * expression, so the bytes equal the host-side result.  x, out dense, n elements.
 */
int tgsr_to_uint8(const float* x, uint8_t* out, int64_t n, void* stream);

/*
 * The image pyramid of the reference's data loader on the GPU (datasets.py:151-197 get_imgs_blur, :236-278), byte-
 * identical to the Pillow arithmetic it delegates to.  Images are planar uint8 [N][H][W] (N = batch x 3 planes).
 *   tgsr_resize_bilinear_u8  transforms.Resize on a PIL image = PIL resize(BILINEAR): horizontal then vertical pass of
 *       a triangle filter in 22-bit fixed point.  hbounds / vbounds: int32 [out][2] = (first input index, tap count);
 *       hcoef / vcoef: int32 [out][hk | vk] taps (the host computes both in double exactly like Pillow's
 *       precompute_coeffs; a pass whose size does not change is skipped and its tables may be NULL).  tmp: exactly
 *       N*Hin*Wout bytes when both passes run, unused (may be NULL) otherwise.  With neither pass `out` is a copy of `in`.
 *       Checked (TGSR_EINVAL, nothing written): in, out non-NULL; N and every size >= 1; the tables of a pass that runs
 *       non-NULL and its hk | vk >= 1; tmp non-NULL when both passes run; the bytes of `in` and `out` do not overlap, and
 *       when both passes run those of `tmp` overlap neither.  The caller's duty: the device tables are trusted - for every
 *       output index, first >= 0, first + count <= the input size of that axis and 0 <= count <= hk | vk; the taps may be
 *       any int32 (the sum of at most count products 255 x tap must fit int32; the result is clipped to [0, 255]).
 *   tgsr_gaussian_blur_u8    ImageFilter.GaussianBlur(radius): `passes` extended-box-blur passes per axis with integer
 *       radius, centre weight ww and far-pixel weight fw in 24-bit fixed point (radius 2, 3 passes: 1, 4473924, 1677722);
 *       clamped borders.  tmp: exactly N*H*W bytes.
 *       Checked (TGSR_EINVAL, nothing written): in, tmp, out non-NULL; N, H, W, passes >= 1; radius >= 0;
 *       (2 radius + 1) ww + 2 fw <= 2^24 in 64-bit arithmetic (what keeps the kernel's uint32 sum from wrapping; Pillow's
 *       weights add up to 2^24 or one less) and radius < 2^23; no two of `in`, `tmp`, `out` share a byte.
 *   tgsr_u8_normalize        ToTensor + Normalize(0.5, 0.5): float32 (u8 / 255 - 0.5) / 0.5 (datasets.py:286-288).
 *       Checked: in, out non-NULL, n >= 1.  out is float32, 4-byte aligned.
 * The uint8 operands need no alignment: the kernels load and store single bytes, so `in`, `tmp` and `out` may start at any
 * address.  The int32 tables are 4-byte aligned.
 */
int tgsr_resize_bilinear_u8(const uint8_t* in, int N, int Hin, int Win, int Hout, int Wout, const int32_t* hbounds,
                            const int32_t* hcoef, int hk, const int32_t* vbounds, const int32_t* vcoef, int vk,
                            uint8_t* tmp, uint8_t* out, void* stream);
int tgsr_gaussian_blur_u8(const uint8_t* in, int N, int H, int W, int radius, uint32_t ww, uint32_t fw, int passes,
                          uint8_t* tmp, uint8_t* out, void* stream);
int tgsr_u8_normalize(const uint8_t* in, float* out, int64_t n, void* stream);

/*
 * The transform chain in front of that pyramid, for a ragged batch in one call (datasets.py:115-123 bounding-box crop,
 * transforms.Resize + RandomCrop + RandomHorizontalFlip of test1.py:184-186, Resize + CenterCrop of datasets.py:1558-1560):
 * per image byte-identical to Pillow's
 *     img.crop((x1, y1, x2, y2)).resize((ow, oh), BILINEAR).crop((left, top, left + S, top + S))   [mirrored if flip]
 * of which only the S x S window is computed.
 *   tgsr_augment_u8     packed: B decoded images back to back, each interleaved uint8 [H][W][3]; nbytes: size of that buffer
 *       (< 2^31).  table: int32 [B][12] = (byte offset, H, W, x1, y1, x2, y2, oh, ow, top, left, flip), once in host memory
 *       (table_host, checked here) and once in device memory (table_dev, what the kernels read - they skip an image whose
 *       descriptor fails the same checks, so no read leaves `packed`).  TGSR_EINVAL unless for every image: H, W in [1, 4096];
 *       offset >= 0 and offset + 3 H W <= nbytes; 0 <= x1 < x2 <= W, 0 <= y1 < y2 <= H; S <= oh, ow <= 65536;
 *       0 <= top <= oh - S, 0 <= left <= ow - S; x2 - x1 <= 16 ow and y2 - y1 <= 16 oh (at most 33 taps); flip in {0, 1}.
 *       ws: tgsr_augment_ws_elems(B, S) int32 (the taps of the window's rows and columns, computed on the device in fp64
 *       exactly like Pillow's precompute_coeffs).  out: planar uint8 [B][3][S][S].  1 <= S <= 4096, B <= 65535.
 *       Two launches on `stream`, plain loads and stores only.
 *   tgsr_resize_coeffs  that coefficient step on its own: bounds int32 [out_size][2] = (first input index, tap count),
 *       taps int32 [out_size][ksize] in 22-bit fixed point, zero behind the count; ksize must be Pillow's
 *       2 ceil(max(in_size / out_size, 1)) + 1.  Sizes in [1, 65536], in_size <= 16 out_size.  Both device memory.
 * Alignment: packed and out may start at any byte; table_host, table_dev, ws, bounds and taps start on 4 bytes (TGSR_EUNSUPPORTED
 * otherwise).  Workspace: ws has exactly tgsr_augment_ws_elems words and what ws holds before a call does not matter - every word the
 * second launch reads the first has written.  Outputs: out, bounds and taps are written whole, the zeros behind a tap count too;
 * the out bytes of an image the kernels skip keep their prior contents.  Refusals (TGSR_EINVAL: a NULL pointer, nbytes outside
 * [1, 2^31), B, S or a host descriptor outside the rules above, a size or ksize tgsr_resize_coeffs does not take):
 * nothing is launched or written.
 */
int64_t tgsr_augment_ws_elems(int B, int S);
int tgsr_augment_u8(const uint8_t* packed, int64_t nbytes, const int32_t* table_host, const int32_t* table_dev, int B, int S,
                    int32_t* ws, uint8_t* out, void* stream);
int tgsr_resize_coeffs(int in_size, int out_size, int ksize, int32_t* bounds, int32_t* taps, void* stream);

/*
 * Image quality of SR output against ground truth, on uint8 images as the reference's caller saves them.
 *   tgsr_sr_metrics  sr, hr: dense NCHW [B][3][H][W], each independently float32 (sr_f32 / hr_f32 != 0: quantised in the kernel
 *       by tgsr_to_uint8's rule) or uint8.  shave >= 0 pixels are removed from every border first; the crop must be at least
 *       11 x 11.  out: float64 [B][3] = (SSE over RGB, SSE over Y, sum of the SSIM values of the crop's (Hc - 10)(Wc - 10) windows).
 *       Y is the reference's rgb2y (trainer_objective.py:168-174) byte for byte; the SSEs are exact integers, so that
 *       rmse = sqrt(sse / n), psnr = 20 log10(255 / rmse) on the host equal the reference's psnr() (:177-181) bit for bit.
 *       SSIM on Y: Wang et al. 2004 as in ssim.m - 11 x 11 Gaussian window of sigma 1.5, 'valid' filtering, K1 = 0.01, K2 = 0.03,
 *       L = 255, fp64.  ws: tgsr_sr_metrics_ws_elems(...) float64 (per-tile partial sums, added in tile order): exactly that
 *       many are written, each before it is read - what ws held before the call does not matter.
 *       Two launches on `stream`, no atomics, no host synchronisation: capturable, and the same bits on every run.
 *   tgsr_rgb_to_y_u8  rgb uint8 [B][3][H][W] -> y uint8 [B][H][W], the same Y.
 * Alignment: a uint8 image (sr, hr, rgb, y) may start at any byte, a float32 image on 4 bytes, ws and out on 8; nothing more.
 * TGSR_EINVAL, nothing launched: a NULL pointer, B outside [1, 65535] (tgsr_rgb_to_y_u8: B < 1), H or W < 1, shave < 0, a crop
 * under 11 on either side (tgsr_sr_metrics_ws_elems returns 0 for those shapes).
 */
int64_t tgsr_sr_metrics_ws_elems(int B, int H, int W, int shave);
int tgsr_sr_metrics(const void* sr, int sr_f32, const void* hr, int hr_f32, int B, int H, int W, int shave, double* ws,
                    double* out, void* stream);
int tgsr_rgb_to_y_u8(const uint8_t* rgb, int B, int H, int W, uint8_t* y, void* stream);

/*
 * No-reference image quality (csrc/tgsr_niqe.hip): the block features of NIQE (Mittal, Soundararajan and Bovik 2013) as MATLAB's
 * niqe / computefeature and BasicSR's calculate_niqe define them; tgsr_amd/niqe.py fits the pristine model and scores.  The head
 * of the kernel file and DESIGN.md 3.17 state the arithmetic; everything is fp64.  Evaluation only, no backward.
 *   img: dense NCHW [B][3][H][W], float32 (is_f32 != 0: quantised in the kernel by tgsr_to_uint8's rule) or uint8; the plane is
 *   the Y of tgsr_sr_metrics.  shave >= 0 pixels leave every border, the rest is cropped at the top-left to whole 96 x 96 blocks:
 *   nblk = floor((H - 2 shave) / 96) floor((W - 2 shave) / 96), row-major.
 *   gam, r_gam: fp64 [n_gam] ON THE DEVICE - the shape grid of the generalised Gaussian fit (np.arange(0.2, 10.001, 0.001), numpy's
 *   own values) and r_gam[k] = G(2 / gam[k])^2 / (G(1 / gam[k]) G(3 / gam[k])), strictly increasing; the fit takes
 *   argmin_k (r_gam[k] - rn)^2 by a binary search and one neighbour comparison, the lower index on a tie, index 0 for a NaN rn.
 *   feats: fp64 [B][nblk][36], scale 1 first; per scale (alpha, (beta_l + beta_r) / 2) of the MSCN block, then for the shifts
 *   (0,1), (1,0), (1,1), (1,-1) (alpha, (beta_r - beta_l) G(2 / alpha) / G(1 / alpha), beta_l, beta_r) of the block times its circular
 *   shift.  sharp: fp64 [B][nblk], the mean of the scale-1 local deviation sigma over the block (the model fit selects blocks by it).
 *   A block without a negative or without a positive element, or with mean(x^2) = 0, gives NaN by IEEE arithmetic (alpha is then
 *   gam[0]); nothing traps.  ws: tgsr_niqe_ws_elems(...) float64 (the moments of every (image, block, scale); 0 = a shape the
 *   entry refuses).  Two launches on `stream`, no atomics, no host synchronisation: capturable, and the same bits on every run.
 * TGSR_EINVAL without launching for a NULL pointer, B < 1 (or > 65535), shave < 0, n_gam < 1 or fewer than 96 pixels on a side after
 * shaving.
 */
int64_t tgsr_niqe_ws_elems(int B, int H, int W, int shave);
int tgsr_niqe_features(const void* img, int is_f32, int B, int H, int W, int shave, const double* gam, const double* r_gam, int n_gam,
                       double* ws, double* feats, double* sharp, void* stream);

/*
 * Learned perceptual distance (csrc/tgsr_lpips.hip): the tail of LPIPS v0.1 (Zhang, Isola, Efros, Shechtman and Wang 2018), one tapped
 * layer per call, and the 2 x 2 max pool of its VGG16 trunk; tgsr_amd/lpips.py walks the trunk on tgsr_gconv.  The head of the kernel
 * file and DESIGN.md 3.18 state the arithmetic.
 * tgsr_maxpool2s2_*: F.max_pool2d(x, 2) for any H, W >= 2 (floor), the signatures of tgsr_maxpool3s2_*: x dense planes with a batch
 *   stride, out / dy based at a channel slice.  The backward routes dy to the FIRST maximum of a window in row-major order (torch's
 *   rule), adds where accumulate != 0, keeps the value where mask > 0 (mask nullable, laid out like dx with dx's batch stride) and
 *   with accumulate = 0 writes dx whole - the zeros of an odd trailing row or column included: no memset.
 * tgsr_lpips_layer_fwd: f0, f1 fp32 [B][C][HW] (samples f0_bstride / f1_bstride floats apart), w fp32 [C] >= 0;
 *   partial fp64 [B][nslots], nslots = tgsr_lpips_nslots(C, HW) (0 = a shape the entries refuse): slot k of image b holds
 *   sum_p sum_c w[c] (n(f0) - n(f1))^2 over the slot's pixels, n(f) = f / (sqrt(sum_c f^2) + 1e-10), not yet divided by HW.  Each
 *   feature is read once; the five channel sums of a pixel are fp64 sums of exactly widened floats.
 *   nslots = ceil(tiles / t): tiles of 16 (HW <= 1024) or 64 pixels, t = ceil(tiles / 512) tiles per slot, at least 4 where
 *   HW >= 32768 (there a wave takes whole tiles: a tile per wave).
 * tgsr_lpips_finish: one launch for L <= 8 taps (partial, nslots <= 512, HW: HOST arrays of L entries, copied into the launch):
 *   per_layer[l][b] = (the tap's slots summed in index order) / HW[l] (fp32 [L][B], nullable), total[b] = their sum in tap order.
 * tgsr_lpips_layer_bwd: df0[b] (+)= g[b] d(d_l[b]) / d(f0[b]) (g fp32 [B] ON THE DEVICE; df0 laid out like f0 with its own batch
 *   stride; mask nullable, like df0: kept where mask > 0 - a tap's own ReLU is applied by passing f0).  accumulate = 0 writes every
 *   element of df0; a pixel whose whole f0 column is 0 gets 0 (autograd: NaN).
 * No atomics, fixed slots and orders: the same bits on every run; no host synchronisation and no allocation: capturable.
 * Alignment: every pointer 4 bytes (all accesses are dwords), partial 8 bytes; else TGSR_EUNSUPPORTED.  TGSR_EINVAL for a NULL
 * pointer, B < 1 (the tail: B > 65535), C < 1, HW < 1, H or W < 2 (the pool), L outside 1..8.  A refusal launches and writes nothing.
 */
int tgsr_maxpool2s2_fwd(const float* x, int64_t x_bstride, int B, int C, int H, int W, float* out, int64_t o_bstride, void* stream);
int tgsr_maxpool2s2_bwd(const float* x, int64_t x_bstride, const float* dy, int64_t dy_bstride, int B, int C, int H, int W, float* dx,
                        int64_t dx_bstride, int accumulate, const float* mask, void* stream);
int tgsr_lpips_nslots(int C, int HW);
int tgsr_lpips_layer_fwd(const float* f0, int64_t f0_bstride, const float* f1, int64_t f1_bstride, const float* w, int B, int C, int HW,
                         double* partial, void* stream);
int tgsr_lpips_finish(const double* const* partial, const int* nslots, const int* HW, int L, int B, float* per_layer, float* total,
                      void* stream);
int tgsr_lpips_layer_bwd(const float* g, const float* f0, int64_t f0_bstride, const float* f1, int64_t f1_bstride, const float* w, int B,
                         int C, int HW, float* df0, int64_t df0_bstride, int accumulate, const float* mask, void* stream);

/*
 * Attention panels (csrc/tgsr_attnviz.hip): one tile per caption word, the word's attention map thresholded, expanded, blurred,
 * stretched to bytes and pasted over the image - build_super_imagesall / build_super_images2 (miscc/utils.py:202-451) on the
 * device.  The arithmetic is stated in tgsr_amd/attnviz.py and DESIGN.md 3.12.
 *   att [B][T][h][w] fp32; cap_lens int32 [B] ON THE DEVICE (the caller checks its host copy; the kernels clamp into [1, T]); words
 *   at and behind cap_lens[b] are not read.  img [B][3][Vh][Vw], (Vh, Vw) = (u h, u w): fp32 in [-1, 1] (img_f32 != 0; quantised
 *   ((v + 1) / 2) * 255, round half to even, clamp) or uint8.  Mh [Vh][h], Mw [Vw][w] fp64: the resize-then-blur operators (the
 *   identity for u = 1).  Per word j < n = cap_lens[b]: thresh = 2 / n in fp64, conf[b][j] = sum x [x > 2 thresh] (0 behind the
 *   caption), x <- x [x > thresh], tile = Mh . x . Mw^T on the fp64 MFMA, byte = trunc((tile - min) / (max - min) * 255), black where
 *   max == min.  panel uint8 [B][Vh][K (Vw + 2)][3]: slot s of row b shows word order[b][s] for s < min(K, n), blended by Pillow's
 *   paste through the constant mask alpha (t = m alpha + i (255 - alpha) + 128; ((t >> 8) + t) >> 8), followed by two black columns;
 *   slots at and behind min(K, n) are black.  by_conf != 0: slots by descending conf, ties to the HIGHER word index; else slot = word.
 *   order int32 [B][T]: the word of every slot s < n (also those at and behind K), -1 behind.  maps_or_null: uint8 [B][T][Vh][Vw],
 *   the un-blended map bytes (black behind the caption).  ws: tgsr_attn_panels_ws_elems(...) float64.
 * Two launches on `stream`, no atomics, no host synchronisation: capturable, the same bits on every run.  Refused before any launch:
 * TGSR_EINVAL for a missing pointer, B, T, K < 1, K > T, u < 1, alpha outside [0, 255]; TGSR_EUNSUPPORTED for h or w outside
 * [2, 128], Vh or Vw > 512, T > 64 (tgsr_attn_panels_ws_elems returns 0 for those shapes).
 * Alignment: panel, maps and a uint8 img may start at any byte (the kernel stores 16 bytes at a time where the address allows and
 * single bytes at the ends of a row group); att, cap_lens, order and a float32 img start on 4 bytes; Mh, Mw, ws and conf start on
 * 8 bytes (TGSR_EUNSUPPORTED otherwise, after the checks above).  Workspace: ws has exactly tgsr_attn_panels_ws_elems doubles;
 * the tile and the min / max pairs of a word behind its caption are neither written nor read, what ws holds before a call does not
 * matter.  Outputs: conf and order are written whole (0 and -1 behind the caption), panel and maps whole.  On a refusal
 * nothing is launched or written.
 */
int64_t tgsr_attn_panels_ws_elems(int B, int T, int h, int w, int u);
int tgsr_attn_panels(const float* att, const int32_t* cap_lens, const void* img, int img_f32, const double* Mh, const double* Mw,
                     int B, int T, int h, int w, int u, int alpha, int K, int by_conf, double* ws, uint8_t* panel,
                     uint8_t* maps_or_null, double* conf, int32_t* order, void* stream);

/*
 * Whole-image inference by overlapping tiles (SRPipeline.upscale; the reference's arbitrary-size example path,
 * datasets.py:200-278, followed by the fully convolutional generators): the cut and the reassembly of a tile batch.
 * table: int32 [Tb][6] = (y0, x0, oy0, oy1, ox0, ox1) in LR pixels, once in host memory (table_host, checked here) and once in
 * device memory (table_dev, what the kernels read - they skip a row that fails the same checks, so no access leaves an
 * image; what such a row would have written - its block of out / out2, its owned rectangle of every dst - keeps what it held:
 * nothing is zeroed).  Window t is rows [y0, y0 + th) x columns [x0, x0 + tw) of the H x W image; the rectangle it OWNS is
 * [oy0, oy1) x [ox0, ox1).  TGSR_EINVAL unless 1 <= th <= min(H, 4096), 1 <= tw <= min(W, 4096), H, W <= 2^20, Tb in [1, 65535]
 * and for every row 0 <= y0 <= H - th, 0 <= x0 <= W - tw, y0 <= oy0 < oy1 <= y0 + th, x0 <= ox0 < ox1 <= x0 + tw.
 *   tgsr_tile_gather  img (and img2 unless NULL; out2 is NULL exactly when img2 is): planar [3][H][W], both uint8 (is_u8 != 0:
 *       normalised by tgsr_u8_normalize's arithmetic, (u8 / 255 - 0.5) / 0.5 in float32 division, subtraction, division) or both
 *       float32 (a bit copy).  out / out2: float32 [Tb][3][th][tw].  One launch for both images.
 *   tgsr_tile_stitch  n <= TGSR_STITCH_MAX outputs of the tile batch in one launch (host arrays of n entries): src[e] float32
 *       [Tb][C[e]][s th][s tw] with s = scale[e] in [1, 64], a dense (C, s th, s tw) block per tile and src_stride[e] elements
 *       between tiles (so a channel crop of a wider buffer is taken in place); dst[e]: [C[e]][s H][s W], float32 (out_u8[e] == 0:
 *       a bit copy) or uint8 (tgsr_to_uint8's rule, the same bytes).  Only each tile's owned rectangle (times s) is written:
 *       where the owned rectangles partition the image (tgsr_amd.tiles.plan_tiles) every output pixel has exactly one source -
 *       no blending, no atomics, the same bits on every run; a pixel no row owns keeps what dst[e] held.  Two rows may name the
 *       same window (a padded last batch): their pixels are written twice with the same values.  src_stride[e] below the block
 *       size is TGSR_EINVAL when Tb > 1; with Tb == 1 it is not used and may be anything.  TGSR_EINVAL too for n outside
 *       [1, TGSR_STITCH_MAX], a NULL list or list entry, C[e] outside [1, 65535], scale[e] outside [1, 64].
 * Rows move as 16-byte accesses where the bases, the row pitches and the rectangle's first column are multiples of 4
 * elements, element by element otherwise (any H, W, offsets): no operand needs more than its element's alignment - a uint8
 * image or destination may start at any byte.  Plain loads and stores; capturable.
 */
#define TGSR_STITCH_MAX 12
int tgsr_tile_gather(const void* img, const void* img2, int is_u8, int H, int W, const int32_t* table_host,
                     const int32_t* table_dev, int Tb, int th, int tw, float* out, float* out2, void* stream);
int tgsr_tile_stitch(int n, const float* const* src, const int64_t* src_stride, void* const* dst, const int* C,
                     const int* scale, const int* out_u8, int H, int W, const int32_t* table_host, const int32_t* table_dev,
                     int Tb, int th, int tw, void* stream);

/*
 * Geometric self-ensemble, x8 (csrc/tgsr_ensemble.hip; SRPipeline.upscale(ensemble=8), SRPipeline.self_ensemble): the network runs
 * on the eight flips and rotations of a window, the eight outputs are mapped back and averaged.
 * THE TRANSFORM.  Variant k = 0..7 has bits b0 = k & 1 (mirror the columns), b1 = k & 2 (mirror the rows), b2 = k & 4 (transpose,
 * applied first).  For a window `win` of th x tw, variant k has shape (th', tw') = b2 ? (tw, th) : (th, tw); its pixel (i, j) is
 * win[y][x] with
 *     i' = b1 ? th' - 1 - i : i        j' = b0 ? tw' - 1 - j : j        (y, x) = b2 ? (j', i') : (i', j').
 * Outputs at scale s follow the same rule with every size multiplied by s.  The ensemble value of an output pixel is
 *     (((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125f       in float32, one rounding per operation,
 * v_k = variant k's output at the position that maps back to the pixel, summed in ascending k: the same bits on every run.
 * The window table and its rules are tgsr_tile_gather's (above), applied to every one of the N images; the same TGSR_EINVAL for
 * each of them, for a missing pointer, N outside [1, 4096] and the cases named below.
 *   tgsr_d8_gather  img (and img2 unless NULL; out2 is NULL exactly when img2 is): [N][3][H][W], both uint8 (is_u8 != 0:
 *       tgsr_u8_normalize's arithmetic) or both float32 (a bit copy).  Variants k0 .. k0 + nk - 1, (k0, nk) one of (0, 8) - which
 *       needs th == tw -, (0, 4), (4, 4).  out / out2: float32 [N][Tb][nk][3][th'][tw'] - the variants of a window are
 *       consecutive rows of the pipeline batch; (4, 4) gives the transposed group, [N][Tb][4][3][tw][th].  One launch for both.
 *   tgsr_d8_merge   n <= TGSR_STITCH_MAX outputs of the variant batch in one launch (host arrays of n entries; n N <= 65535).
 *       nk = 8: srcA[e] float32 [N][Tb][8][C[e]][s th][s tw] (th == tw), srcB NULL or srcB[e] NULL.  nk = 4: srcA[e] holds
 *       variants 0..3 as [N][Tb][4][C[e]][s th][s tw] and srcB[e] the transposed group 4..7 as [N][Tb][4][C[e]][s tw][s th];
 *       a srcB[e] that is present with nk = 8 or missing with nk = 4 is TGSR_EINVAL.  A batch row is a dense (C, rows, columns)
 *       block; src_stride[e] >= its size: elements between consecutive batch rows of srcA[e] and of srcB[e].  s = scale[e] in
 *       [1, 64].  dst[e]: [N][C[e]][s H][s W], float32 (out_u8[e] == 0: the mean) or uint8 (tgsr_to_uint8's rule applied to the
 *       float32 mean).  Only each window's owned rectangle (times s) is written, each pixel once - a pixel no row owns, and the
 *       rectangle of a row of table_dev that fails the checks, keep what dst[e] held; two rows that name the same window (a
 *       padded last batch) write the same values twice.  src_stride[e] below the block size is TGSR_EINVAL whatever Tb.  No
 *       atomics, no workspace.
 * Layout: a workgroup owns a 32 x 32 block on the window's side; every global access runs along rows of its image, as aligned
 * 16-byte quads where the bases, the row pitches and the row strides are multiples of 4 elements, element by element otherwise
 * (any H, W, offsets; no operand needs more than its element's alignment); the mirrors and the transpose happen between a
 * padded LDS block and registers.  Plain loads and stores; capturable.
 */
int tgsr_d8_gather(const void* img, const void* img2, int is_u8, int N, int H, int W, const int32_t* table_host,
                   const int32_t* table_dev, int Tb, int th, int tw, int k0, int nk, float* out, float* out2, void* stream);
int tgsr_d8_merge(int n, const float* const* srcA, const float* const* srcB, const int64_t* src_stride, void* const* dst,
                  const int* C, const int* scale, const int* out_u8, int nk, int N, int H, int W, const int32_t* table_host,
                  const int32_t* table_dev, int Tb, int th, int tw, void* stream);

/*
 * Weight gradient of tgsr_conv3x3_fwd: dw[Cout][Cin][3][3] = sum over (b, y, x) of grad_out * shifted input
 * (upsample=1: the input is read through the folded nearest-x2, H/W are the PRE-upsample sizes).
 * grad_out [B][Cout][Ho][Wo] dense; x [B][Cin][H][W] with batch stride; Cout % 32 == 0.
 * ws must hold tgsr_conv3x3_wgrad_ws_elems(...) floats (per-workgroup partial slabs, summed in a fixed order).
 * The data gradient is tgsr_conv3x3_fwd on the flipped / transposed weights (+ tgsr_sumpool2x2 for upsample=1).
 *
 * The planners of this and of the next two weight gradients.  Every launch is planned once, by one host function
 * (csrc/tgsr_wgrad_plan.h); tgsr_conv3x3_wgrad_plan is that very function, for `kind` = TGSR_WGRAD_DIRECT (tgsr_conv3x3_wgrad),
 * TGSR_WGRAD_WINO (tgsr_wino_wgrad; `upsample` is not read) or TGSR_WGRAD_UPWINO (tgsr_upwino_wgrad; likewise).  Host
 * arithmetic only: grad_out and x are looked at for their alignment and never read through.  It returns what the launcher
 * returns for these sizes and alignments (TGSR_EINVAL: a size < 1 or an unknown kind; TGSR_EUNSUPPORTED: the channel counts or
 * an alignment the kernel does not take) and fills out[TGSR_WGRAD_PLAN_FIELDS] (may be NULL):
 *     [0] the kernel family, TGSR_WGRAD_FAMILY_*     [1..3] its template integers, 0 where it has fewer:
 *         DIRECT conv3x3_wgrad_kernel<NCOB, NCIB, UP>, WINO wino_wgrad_kernel<NCI, NCOB>, WINO_DMA wino_wgrad_dma_kernel<NCI>
 *         (16-byte aligned operands, W % 4 == 0, x_bstride % 4 == 0 on a Cout % 64 == 0, Cin % 64 == 0 layer), UPWINO
 *         upwino_wgrad_kernel<NCI>
 *     [4] units: 2 x 32-pixel tiles (direct) or chunks of 8 tiles / 16 pixels (wino / upwino)     [5] units per workgroup
 *     [6] nslots = partial slabs = grid.x     [7] channel groups = grid.y     [8] floats per slab     [9] ws_elems = [6] x [8]
 * all 0 where the status is not TGSR_OK.  Each *_ws_elems below is "plan, then ws_elems" for operands of any alignment (the
 * workspace does not depend on it): 0 for every shape its launcher refuses.
 */
#define TGSR_WGRAD_DIRECT 0
#define TGSR_WGRAD_WINO 1
#define TGSR_WGRAD_UPWINO 2
#define TGSR_WGRAD_FAMILY_DIRECT 0
#define TGSR_WGRAD_FAMILY_WINO 1
#define TGSR_WGRAD_FAMILY_WINO_DMA 2
#define TGSR_WGRAD_FAMILY_UPWINO 3
#define TGSR_WGRAD_PLAN_FIELDS 10
int tgsr_conv3x3_wgrad_plan(int kind, const float* grad_out, const float* x, int64_t x_bstride, int B, int Cin, int H, int W,
                            int Cout, int upsample, int64_t* out);
int64_t tgsr_conv3x3_wgrad_ws_elems(int B, int Cin, int Cout, int H, int W, int upsample);
int tgsr_conv3x3_wgrad(const float* grad_out, const float* x, int64_t x_bstride, int B, int Cin, int H, int W, int Cout,
                       int upsample, float* ws, float* dw, void* stream);

/*
 * The same weight gradient for the upBlock convolution (upsample = 1) in the domain of the up-sample-aware Winograd
 * form: dU'[p] = sum over LOW-resolution pixels of dM[p] (x) V[p] for the 9 positions, then dW = G'^T dU' G' - 4x fewer
 * multiplies than the direct form.  grad_out [B][Cout][2H][2W] dense (8-byte aligned), x [B][Cin][H][W] with batch
 * stride; Cout % 64 == 0, Cin % 32 == 0.  ws: tgsr_upwino_wgrad_ws_elems floats (per-workgroup partial slabs, summed
 * in a fixed order; 0 for a shape the launcher refuses: plan, then ws_elems).  dw [Cout][Cin][3][3].
 */
int64_t tgsr_upwino_wgrad_ws_elems(int B, int Cin, int Cout, int H, int W);
int tgsr_upwino_wgrad(const float* grad_out, const float* x, int64_t x_bstride, int B, int Cin, int H, int W, int Cout,
                      float* ws, float* dw, void* stream);

/*
 * Weight gradient of the plain conv3x3 (upsample = 0) in the Winograd F(2x2,3x3) domain: dU[p] = sum over 2x2 output
 * tiles of dM[p] (x) V[p] for the 16 positions, then dW = G^T dU G - 2.25x fewer multiplies than tgsr_conv3x3_wgrad.
 * grad_out [B][Cout][H][W] dense, x [B][Cin][H][W] with batch stride; Cout % 32 == 0, Cin % 32 == 0.
 * ws: tgsr_wino_wgrad_ws_elems floats (per-workgroup partial slabs, summed in a fixed order; 0 for a shape the launcher
 * refuses: plan, then ws_elems).  dw [Cout][Cin][3][3].
 */
int64_t tgsr_wino_wgrad_ws_elems(int B, int Cin, int Cout, int H, int W);
int tgsr_wino_wgrad(const float* grad_out, const float* x, int64_t x_bstride, int B, int Cin, int H, int W, int Cout,
                    float* ws, float* dw, void* stream);

/*
 * Backward of tgsr_word_attention_fwd (the attention map output carries no gradient).  P is recomputed from h and
 * src.  dc [B][idf][Q] dense -> dh [B][idf][Q] dense and dsrc_part [B][nchunks][idf][32] (nchunks =
 * tgsr_word_attention_bwd_chunks(Q)); the caller sums the chunks and maps dsrc to conv_context.weight / words:
 * dW_ctx[i][c] = sum_{b,t} dsrc[b][i][t] words[b][c][t].   idf in {32, 64}, T <= 32.
 */
int tgsr_word_attention_bwd_chunks(int Q);
int tgsr_word_attention_bwd(const float* h, int64_t h_bstride, const float* src, const uint8_t* mask, int mask_mode,
                            int B, int idf, int T, int Q, const float* dc, float* dh, float* dsrc_part, void* stream);

/*
 * Backward of tgsr_conv_to3_fwd.  g = dy * (1 - t^2), t = out - alpha*addend for act = TGSR_ACT_TANH_AXPY (out = the
 * forward output), g = dy otherwise.  dx (may be NULL) [B][Cin][H][W] dense needs w; dw (may be NULL) [3][Cin][K][K]
 * needs x and ws = tgsr_conv_to3_bwd_ws_elems(...) floats.  d(addend) = alpha * dy is left to the caller.
 * TGSR_EUNSUPPORTED: K not in {3, 5}, Cin > 64.
 * tgsr_conv_to3_bwd_plan is the function the launcher plans the weight gradient with (host arithmetic): it returns the
 * launcher's status for these sizes and fills out[TGSR_TO3_BWD_PLAN_FIELDS] (may be NULL): [0] 1: conv_to3_wgrad_mfma_kernel<K,
 * TANH, Cin / 16> (W % 16 == 0, Cin % 16 == 0), 0: conv_to3_wgrad_kernel<K, TANH>; [1] rows per wave of the MFMA tile (4 [1] x 64
 * pixels per workgroup: the largest of 8, 4, 2, 1 that gives >= 1024 workgroups; 1 for the other kernel's 16 x 64 tile); [2] slabs
 * = workgroups; [3] ws_elems = [2] x 3 Cin K K - all 0 where the status is not TGSR_OK.  tgsr_conv_to3_bwd_ws_elems is "plan,
 * then ws_elems": 0 for every shape the launcher refuses.
 */
#define TGSR_TO3_BWD_PLAN_FIELDS 4
int tgsr_conv_to3_bwd_plan(int B, int Cin, int H, int W, int K, int64_t* out);
int64_t tgsr_conv_to3_bwd_ws_elems(int B, int Cin, int H, int W, int K);
int tgsr_conv_to3_bwd(const float* dy, const float* out, const float* addend, float alpha, const float* x,
                      int64_t x_bstride, const float* w, int B, int Cin, int H, int W, int K, int act, float* dx,
                      float* ws, float* dw, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Reduced-precision inference path (BASELINE.json configs[4]: "bf16 ... MFMA bf16 attention + fused conv").
 * Storage type `dtype` = TGSR_DT_BF16 or TGSR_DT_F16 (2-byte elements), MFMA operands in that type, fp32 accumulation,
 * fp32 epilogue arithmetic, one round-to-nearest-even per stored element.  Activation layout ("lp image"):
 *     [B][H + 2][W + 2][cpitch]  channels-last with a one-pixel ZERO border that no kernel ever writes
 * (allocate the buffer zeroed once).  `cpitch` is the channel pitch of the buffer, `coff` the first channel a call
 * reads / writes: two producers writing channel ranges [0,32) and [32,64) of one cpitch-64 image replace the
 * reference's torch.cat((h_code, c_code), 1) (util.py:771, 817).  All pointers are to element [0][0][0][0] of the
 * padded image.  Shapes: W % 32 == 0, H % 4 == 0 (every layer of the x8 / x16 generators at LR >= 32).
 *
 * What holds for every entry of this section (tests/test_hip_lp_abi.py calls each one on operands in a guarded arena):
 *   - an lp image, a weight pack and `att_pack` are 16-byte aligned (the c_img of tgsr_lp_word_attention_fwd: 8-byte); channel
 *     pitches and offsets are multiples of 8 elements unless an entry says 4; an offset is >= 0 and offset + width <= pitch.
 *     An entry returns TGSR_EUNSUPPORTED for what breaks these rules, TGSR_EINVAL for a NULL that may not be NULL, a size < 1
 *     or an unknown dtype / epilogue / act / mask_mode - always in front of the launch, no operand touched;
 *   - a call writes the interior pixels x the channel range it names and nothing else: the border, the channels of the image
 *     outside [coff, coff + width) and every input keep their bits.  Every element of the written range is written;
 *   - per-sample images stay below 2 GiB: (H + 2) (W + 2) cpitch 2 < 2^31 for every image of a call (the residual's included);
 *   - fp32 operands (scale, shift, addend, amap, src, attn, head_partial, low, high) are dense and 4-byte aligned unless an
 *     entry says 16.
 */
#define TGSR_DT_BF16 1
#define TGSR_DT_F16 2

/* fp32 NCHW [B][C][H][W] <-> channels [coff, coff + C) of an lp image (interior pixels only).  Element by element: any H, W,
 * cpitch and coff (2-byte aligned image, 4-byte aligned fp32 tensor); coff < 0 or coff + C > cpitch is TGSR_EINVAL.  One
 * round-to-nearest-even per element on the way in, exact on the way out. */
int tgsr_lp_from_nchw(int dtype, const float* x, void* out, int B, int C, int H, int W, int cpitch, int coff,
                      void* stream);
int tgsr_lp_to_nchw(int dtype, const void* x, float* out, int B, int C, int H, int W, int cpitch, int coff,
                    void* stream);

/* An lp image (any shape; the whole buffer incl. its zero border, n_elems % 8 == 0, 16-byte aligned) from one 2-byte type
 * to the other: TGSR_DT_F16 -> TGSR_DT_BF16 (one round-to-nearest-even) or back (exact while |x| < 65504).  Used where a
 * section of a generator runs with f16 operands inside the bf16 configuration (NetG_highweight's 32x32 trunk: the six
 * chained ResBlocks of model.py:258-262 are where 8-bit mantissas cost the finest image 7 dB; profiles/HISTORY.md 3.8d).
 * Every refusal (NULL, n_elems < 8 or not a multiple of 8, equal or unknown types, a misaligned pointer) is TGSR_EINVAL. */
int tgsr_lp_convert(int src_dtype, const void* src, int dst_dtype, void* dst, int64_t n_elems, void* stream);

/* conv weight [Cout][Cin][3][3] (fp32, torch layout) -> MFMA fragment order
 * [kernel row dy 3][k16 Cin/16][kernel column dx 3][cb Cout/32][lane l 64][j 8], rounded to `dtype`
 * (tgsr_lp_packed_conv3x3_elems 2-byte elements): element j of lane l = w[cb*32 + (l & 31)][k16*16 + 8 (l >> 5) + j][dy][dx].
 * Cout % 32 == 0, Cin % 16 == 0 (else TGSR_EUNSUPPORTED).  Every element of the pack is written. */
int64_t tgsr_lp_packed_conv3x3_elems(int Cout, int Cin);
int tgsr_lp_pack_conv3x3_weight(int dtype, const float* w, void* wpack, int Cout, int Cin, void* stream);

/*
 * The fused blocks of tgsr_conv3x3_fwd on lp images (same reference sites: ResBlock.block util.py:110-130, upBlock
 * util.py:74-80, residual24/48 model.py:229-232):
 *   out = epilogue(scale * conv3x3(upsample ? nearest_x2(x) : x) + shift), epilogue = TGSR_EPI_AFFINE (+ residual when
 *   `residual` != NULL) or TGSR_EPI_AFFINE_GLU (Cout/2 output channels).
 * H, W are the OUTPUT size (x is H/2 x W/2 when upsample != 0; only with TGSR_EPI_AFFINE_GLU).  scale / shift fp32
 * [Cout] (NULL, NULL = identity).  (Cin, Cout) in {(64,128), (64,64), (32,64), (32,32)}: the generator's layers (GLU needs
 * Cout >= 64; another pair, or `upsample` without GLU, is TGSR_EUNSUPPORTED; a residual with GLU is TGSR_EINVAL).
 * x: channels [0, Cin) of an image of pitch x_cpitch >= Cin are read, the rest of it is not.  residual: channels [res_coff,
 * res_coff + Cout) of an image of the output's size, which may be a third image.  out: channels [out_coff, out_coff + Cout or
 * Cout/2) of every interior pixel are written; out must not be x (tiles read their neighbours' halo).
 * tgsr_lp_conv3x3_plan: the output rows one workgroup of this entry takes at (B, H, W) - 8 where B (H/8) (W/32) >= 512 and
 * H % 8 == 0, else 4 - or the TGSR_E code the entry gives for these sizes.  Host only; the launcher itself asks it.
 */
int tgsr_lp_conv3x3_plan(int B, int H, int W);
int tgsr_lp_conv3x3_fwd(int dtype, const void* x, int x_cpitch, int B, int Cin, int H, int W, const void* wpack,
                        int Cout, const float* scale, const float* shift, const void* residual, int res_cpitch,
                        int res_coff, void* out, int out_cpitch, int out_coff, int epilogue, int upsample,
                        void* stream);

/*
 * The two ResBlocks of a generator stage (util.py:110-130 as called by INIT_STAGE_GImgup / NEXT_STAGE_G, util.py:773, :818) on
 * 64-channel lp images in ONE launch: four dependent convolutions
 *     tmp = GLU(affine0(conv(x, w0)));  a = affine1(conv(tmp, w1)) + x;  tmp = GLU(affine2(conv(a, w2)));  b = affine3(conv(tmp, w3)) + a
 * each computed per tile by the very code of tgsr_lp_conv3x3_fwd (bit-identical results); a tile's dependence on its neighbours'
 * previous layer is guarded by per-tile flags in device memory instead of a kernel boundary (what a dependent launch costs in a
 * replayed graph is more than these layers' work at 32^2 and 64^2).  wpack / scale / shift: HOST arrays of 4 device pointers
 * (packs of [128,64,3,3], [64,64,3,3], [128,64,3,3], [64,64,3,3]; scale / shift NULL together = identity).  x, tmp, a_out, b_out:
 * four distinct images [B][H+2][W+2][cpitch >= 64], channels [0, 64).  flags: tgsr_lp_resblocks_flag_elems(B, H, W) uint32,
 * zeroed ONCE by the caller and then owned by this function across launches (one buffer per set of images: concurrent launches
 * on different streams need different flag buffers); its last word is set to 1 if a wait ever timed out (results invalid).
 * W % 32 == 0, H % 4 == 0.
 */
int64_t tgsr_lp_resblocks_flag_elems(int B, int H, int W);
int tgsr_lp_resblocks_fwd(int dtype, const void* x, int x_cpitch, int B, int H, int W, const void* const* wpack,
                          const float* const* scale, const float* const* shift, void* tmp, int tmp_cpitch, void* a_out,
                          int a_cpitch, void* b_out, int b_cpitch, unsigned* flags, void* stream);

/*
 * upBlock (util.py:74-80: Upsample(x2, nearest) -> conv3x3 -> BN -> GLU) on lp images by sub-pixel decomposition: each
 * output phase (row & 1, column & 1) is a 2x2 convolution of the LOW-resolution image with taps pre-summed in fp32 and
 * rounded once to `dtype` - 16 products per low-res pixel instead of 36 (tgsr_lp_conv3x3_fwd(upsample = 1) is the
 * direct 9-tap form on the same layout).  H, W = size of the LOW-resolution input x; out [B][2H+2][2W+2][out_cpitch]
 * receives Cout/2 = 32 channels at out_coff.  Cout == 64, Cin in {32, 64}, W % 32 == 0, H % 4 == 0.
 * The pack: [k16 Cin/16][column group 2][combo 8][cb 2][lane l 64][j 8]; combo = 4 a + 2 b + dys for row phase a, column
 * phase b; it holds, for output channel cb*32 + (l & 31) and input channel k16*16 + 8 (l >> 5) + j, the fp32 sum - rows
 * first, then columns - of the 3x3 taps that fall on low-res row offset a + dys - 1 and column offset (group 0: 2 b - 1;
 * group 1: 0) of phase (a, b) (a = 0: rows {-1: w0, 0: w1 + w2}; a = 1: rows {0: w0 + w1, +1: w2}; the same for columns),
 * rounded once.  Every element is written.  scale / shift NULL, NULL = identity.
 */
int64_t tgsr_lp_packed_upconv_elems(int Cout, int Cin);
int tgsr_lp_pack_upconv_weight(int dtype, const float* w, void* wpack, int Cout, int Cin, void* stream);
int tgsr_lp_upconv_glu_fwd(int dtype, const void* x, int x_cpitch, int B, int Cin, int H, int W, const void* wpack,
                           int Cout, const float* scale, const float* shift, void* out, int out_cpitch, int out_coff,
                           void* stream);

/*
 * upBlock WITH the image head that reads its output, in one launch (the feature image of the last stage - consumed by
 * nothing but its head: GET_IMAGE_G_noAct util.py:909-919 behind G_SR_NET_low.h_net3, conv_output model.py:224 behind
 * NetG_highweight.upscale8x - then never goes to HBM).  Arguments of tgsr_lp_upconv_glu_fwd, plus:
 *   out           may be NULL: the 32-channel feature image is not written;
 *   head_wpack    tgsr_lp_pack_to3_weight of the head's [3][32][K][K] filter, head_k = K in {3, 5};
 *   head_partial  tgsr_lp_head_partial_elems(B, 2H, 2W, K) floats: a workgroup tile (8 x 64 outputs) holds only its own
 *                 pixels, so it writes the PARTIAL head sums of the (8 + 2P) x (64 + 2P) outputs they reach, layout
 *                 [B][2H/8][2W/64][3][8 + 2P][64 + 2P], P = K/2.  EVERY element is written (zero contributions included):
 *                 the combine reads all of it.  head_wpack NULL or head_k outside {3, 5} is TGSR_EINVAL.
 * The feature image, where written, holds the bits tgsr_lp_upconv_glu_fwd gives.
 * tgsr_lp_head_combine adds the <= 4 partials of every pixel in a fixed order (tile rows, then columns: reproducible, no
 * float atomics) for up to 4 scales in ONE launch and finishes both generators' heads:
 *   low[s]  = sum of partial_low[s] (3x3 heads)  [tanh when low_tanh: GET_IMAGE_G of models16, util.py:894-905]
 *   high[s] = tanh(sum of partial_high[s] (5x5 heads)) + alpha * low[s]        (model.py:280, 288, 297)
 * H[s], W[s] = image size of scale s (multiples of 8 / 64); partial_low[s] == NULL: low[s] is an input (already
 * computed); partial_high[s] == NULL: high[s] is not produced (high[s] may then be NULL).  low / high fp32 [B][3][H][W]
 * dense, 16-byte aligned.  H, W, partial_low, partial_high, low, high: HOST arrays of nscales entries; 1 <= nscales <= 4.
 */
int64_t tgsr_lp_head_partial_elems(int B, int H, int W, int K);
int tgsr_lp_upconv_glu_head_fwd(int dtype, const void* x, int x_cpitch, int B, int Cin, int H, int W, const void* wpack,
                                int Cout, const float* scale, const float* shift, void* out, int out_cpitch, int out_coff,
                                const void* head_wpack, int head_k, float* head_partial, void* stream);
int tgsr_lp_head_combine(int nscales, int B, const int* H, const int* W, const float* const* partial_low,
                         const float* const* partial_high, float* const* low, float* const* high, int low_tanh,
                         float alpha, void* stream);

/*
 * tgsr_lp_head_combine for NetG_highweight's other three forms (model.py:212-298: weightmap x useAct):
 *   high[s] = act(sum of partial_high[s]) + a[s] * low[s],   act = tanh (high_tanh != 0) or the identity (useAct=False,
 *   model.py:226);  a[s] = amap[s][y][x] (weightmap=True: model.py:277, 286, 294, broadcast over batch and channels) or
 *   alpha where amap == NULL or amap[s] == NULL.
 * amap: HOST array of nscales device pointers (or NULL), each a dense fp32 [H[s]][W[s]] map, 16-byte aligned.  Every other
 * argument and rule as tgsr_lp_head_combine; with amap == NULL and high_tanh = 1 the results are its results bit for bit.
 * Replaces `one * conv_output(out_k) + a_k * SRb_k` with a_k a map (model.py:277-297) and the bare-conv heads of useAct=False.
 */
int tgsr_lp_head_combine_map(int nscales, int B, const int* H, const int* W, const float* const* partial_low,
                             const float* const* partial_high, float* const* low, float* const* high,
                             const float* const* amap, int low_tanh, int high_tanh, float alpha, void* stream);

/*
 * The two 3-channel stems on the fp32 LR image: conv3x3 3 -> 2C + BatchNorm(eval) affine + GLU, written as C channels
 * of an lp image (im2f util.py:741-744, convin model.py:228).  x [B][3][H][W] fp32 dense, w [2C][3][3][3] fp32 (torch
 * layout, NOT rounded: 27 MACs per output run on the VALU), scale / shift [2C], neither may be NULL.  C % 8 == 0,
 * 8 <= C <= 64.  tgsr_lp_stem_fwd takes ANY H and W (a last column tile of W % 32 pixels writes those pixels only).
 */
int tgsr_lp_stem_fwd(int dtype, const float* x, int B, int H, int W, const float* w, int C, const float* scale,
                     const float* shift, void* out, int out_cpitch, int out_coff, void* stream);

/*
 * Word attention fused into the kernel that PRODUCES h (GlobalAttention.py:87-130 called at util.py:768-771 on im2f's output
 * and at util.py:814-817 on the previous stage's upBlock output; c_code[:, q] depends only on h[:, q] and the words):
 *   tgsr_lp_stem_att_fwd        = tgsr_lp_stem_fwd (C = 32, W % 32 == 0) + the first stage's attention;
 *   tgsr_lp_upconv_glu_att_fwd  = tgsr_lp_upconv_glu_fwd (head_partial NULL) / tgsr_lp_upconv_glu_head_fwd (head_k = 3)
 *                                 of a 64 -> 64 upBlock + the NEXT stage's attention on its output.
 * Same arithmetic as tgsr_lp_word_attention_fwd on the stored h (one shared device function: bit-identical results):
 * c_code -> channels [c_coff, c_coff + 32) of the same pixels of `out` (must not overlap [out_coff, out_coff + 32)),
 * attn [B][T][H_out * W_out] fp32 or NULL.  att_pack / att_nsets: what tgsr_text_tail_lp_fwd wrote for this batch; att_set:
 * which projection this stage attends through; use_mask 0: no mask; mask_mode as tgsr_word_attention_fwd (0 or 1, else
 * TGSR_EINVAL).  c_coff % 4 == 0, >= 0, c_coff + 32 <= out_cpitch.  1 <= T <= 32.  The stem form needs scale / shift.
 * The stand-alone attention launches - and their re-read of h - leave G_SR_NET_low's dependent chain.
 */
int tgsr_lp_stem_att_fwd(int dtype, const float* x, int B, int H, int W, const float* w, int C, const float* scale,
                         const float* shift, void* out, int out_cpitch, int out_coff, const void* att_pack, int att_nsets,
                         int att_set, int use_mask, int mask_mode, int T, int c_coff, float* attn, void* stream);
int tgsr_lp_upconv_glu_att_fwd(int dtype, const void* x, int x_cpitch, int B, int Cin, int H, int W, const void* wpack,
                               int Cout, const float* scale, const float* shift, void* out, int out_cpitch, int out_coff,
                               const void* head_wpack, int head_k, float* head_partial, const void* att_pack, int att_nsets,
                               int att_set, int use_mask, int mask_mode, int T, int c_coff, float* attn, void* stream);

/*
 * The image heads on an lp image (tgsr_conv_to3_fwd's reference sites: GET_IMAGE_G_noAct util.py:913-915; conv_output
 * + `one*. + a*SRb` model.py:224, 280/288/297).  w [3][32][K][K] fp32 -> wpack (K*512 2-byte elements: one 16-row MFMA
 * fragment per kernel row whose rows are the (output channel, kernel column) pairs); x = channels [0, 32) of an lp image; addend / out fp32 [B][3][H][W] dense.
 * Cin == 32, K in {3, 5}, W % 32 == 0, H % 8 == 0.  The pack [kernel row dy K][lane l 64][j 8]: element j of lane l =
 * w[c][8 (l >> 4) + j][dy][dx] for row (l & 15) = c K + dx < 3 K, else 0; every element written.  act = TGSR_ACT_NONE
 * (addend ignored) or TGSR_ACT_TANH_AXPY; addend NULL under TANH_AXPY: out = tanh(conv).  x_cpitch >= 32.
 */
int tgsr_lp_pack_to3_weight(int dtype, const float* w, void* wpack, int Cin, int K, void* stream);
int tgsr_lp_conv_to3_fwd(int dtype, const void* x, int x_cpitch, int B, int Cin, int H, int W, const void* wpack, int K,
                         int act, const float* addend, float alpha, float* out, void* stream);

/*
 * tgsr_lp_conv_to3_fwd for NetG_highweight's other forms (model.py:212-298: weightmap x useAct), the stand-alone head:
 *   out = act(conv) + a * addend,  act = tanh (TGSR_ACT_TANH_AXPY) or the identity (TGSR_ACT_IDENT_AXPY, useAct=False,
 *   model.py:226);  a = amap[y][x] (weightmap=True: model.py:277, 286, 294) or alpha when amap == NULL.
 * amap: dense fp32 [H][W] (broadcast over batch and channels) or NULL; act = TGSR_ACT_NONE takes no map.  Every other
 * argument and rule as tgsr_lp_conv_to3_fwd; with amap == NULL and act in {NONE, TANH_AXPY} the results are its results bit
 * for bit.
 */
int tgsr_lp_conv_to3_map_fwd(int dtype, const void* x, int x_cpitch, int B, int Cin, int H, int W, const void* wpack, int K,
                             int act, const float* addend, float alpha, const float* amap, float* out, void* stream);

/*
 * GlobalAttentionGeneral.forward (GlobalAttention.py:87-130) on lp images: h = channels [0, idf) of an lp image,
 * src = the fp32 word projection [B][idf][32] of tgsr_word_project_fwd (rounded to `dtype` inside), mask / mask_mode as
 * in tgsr_word_attention_fwd (0 = the reference's mask.repeat row order, GlobalAttention.py:109-116; 1 = per sample).
 * Writes c_code (rounded) to channels [c_coff, c_coff + idf) of c_img - normally the same image h lives in, which is
 * the reference's torch.cat((h_code, c_code), 1) - and the fp32 softmax to attn [B][T][H*W] (NULL = not needed).
 * idf == 32, T <= 32, W % 32 == 0 (any H).  c_cpitch % 4 == 0, c_coff % 4 == 0, c_coff >= 0, c_img 8-byte aligned.  c_img == h
 * with c_coff < 32 - c_code over the channels other tiles still read - is TGSR_EUNSUPPORTED, as in the fused forms; a
 * mask_mode outside {0, 1} is TGSR_EINVAL.  src holds zeros at words t >= T.  A mask row with EVERY word masked is outside
 * the contract (the softmax of an empty set: NaN, as in the reference).  mask [B][T] bytes, any alignment, any B (mode 0
 * reads row (b H W + q) % B for pixel q of sample b).
 */
int tgsr_lp_word_attention_fwd(int dtype, const void* h, int h_cpitch, const float* src, const uint8_t* mask,
                               int mask_mode, int B, int idf, int T, int H, int W, void* c_img, int c_cpitch, int c_coff,
                               float* attn, void* stream);

/*
 * The objectives that read the generator's word-attention maps (the reference's miscc/losses.py; tgsr_attn_losses.hip).
 *
 * tgsr_attn_confidence - the per-word weights of words_reweight_loss (:150-163): att fp32 [B][T][Q] dense (any 4-byte aligned base),
 * cap_lens int32 [B] ON THE DEVICE (no launch argument depends on the lengths), conf fp32 [B][T]:
 *   conf[b][t] = the fp32 sum of the values of att[b][t] strictly above (float)(2.0 * (2.0 / (double)cap_lens[b]))   for t < cap_lens[b],
 *              = 0 without reading the map                                                                          for t >= cap_lens[b];
 *   a row whose cap_lens[b] lies outside [1, T] is written as zeros.  One workgroup per map, a fixed reduction tree.
 *   B <= 65535, T <= 255, Q >= 1.
 *
 * tgsr_weight_mse_fwd - one scale of weight_MSE (:792-804): fake, label fp32 [B][C][H][W], att fp32 [B][T][h][w], all dense,
 * H = r h and W = r w for one integer r >= 1, T <= 255.
 *   wmax[b][y][x] = max_t att[b][t][y][x],  widx = the word that holds it (the lowest on a tie),
 *   loss[0]       = sum_{b,c,Y,X} (T wmax[b][Y / r][X / r]) (fake - label)^2 / (H W B C),
 *   wlast         = NULL, or fp32 [B][1][H][W]: wmax at (Y / r, X / r) - nn.Upsample(size=(H, W)) of the maximum, bit for bit.
 *   ws: tgsr_weight_mse_ws_elems(...) floats (0 = a shape the entry refuses); the workgroups' partial sums, added in index order.
 * tgsr_weight_mse_bwd - grad fp32 [1] on the device (the gradient reaching loss[0]); writes whichever of these is not NULL (one at least):
 *   d_fake  = grad 2 T wmax[Y / r][X / r] (fake - label) / (H W B C),   d_label = -d_fake,
 *   d_att fp32 [B][T][h][w], written completely: grad T / (H W B C) sum_{c, r x r} (fake - label)^2 at widx, 0 at the other words.
 * 16 bytes per lane where every pointer is 16-byte aligned, w % 4 == 0 and r in {1, 2, 4}; element by element otherwise.  No atomics.
 * Every entry returns TGSR_EINVAL without launching (and without touching an output) for a NULL pointer, a size < 1, T > 255,
 * H % h != 0, W % w != 0 or H / h != W / w.
 */
int tgsr_attn_confidence(const float* att, const int32_t* cap_lens, int B, int T, int Q, float* conf, void* stream);
int64_t tgsr_weight_mse_ws_elems(int B, int C, int T, int H, int W, int h, int w);
int tgsr_weight_mse_fwd(const float* fake, const float* label, const float* att, int B, int C, int T, int H, int W, int h, int w,
                        float* ws, float* loss, float* wmax, uint8_t* widx, float* wlast, void* stream);
int tgsr_weight_mse_bwd(const float* grad, const float* fake, const float* label, const float* wmax, const uint8_t* widx, int B, int C,
                        int T, int H, int W, int h, int w, float* d_fake, float* d_label, float* d_att, void* stream);

/*
 * The cycle-consistency objective (the reference's miscc/losses.py, CycleMSE :785-790; tgsr_cycle_mse.hip): every SR image of a
 * pyramid resized back to the LR size with torch's bicubic rule and held to the LR input by a mean squared error.
 *   sr   HOST array of n DEVICE pointers, sr[i] fp32 [B][C][H[i]][W[i]] dense (any 4-byte aligned base); H, W HOST arrays of n ints;
 *   lr   fp32 [B][C][h][w] dense.  1 <= n <= 8; H[i] / h and W[i] / w are arbitrary and independent (down, identity, up).
 *   Per axis, in float32 as torch computes it (align_corners=False, no antialiasing, A = -0.75):
 *     scale = (float)H / h,  src = scale (y + 0.5f) - 0.5f (not clamped at 0),  t = src - floor(src),
 *     taps floor(src) - 1 .. floor(src) + 2 clamped to [0, H - 1].
 *
 * tgsr_cycle_mse_fwd - one kernel launch for all n scales + one finish launch:
 *   diff fp32 [n][B][C][h][w] = resized_i - lr (what the backward reads),
 *   terms fp32 [n]:  terms[i] = sum(diff_i^2) / (B C h w)   (the partials added in index order in fp64, one fp32 division),
 *   loss fp32 [1]:   loss[0] = terms[0] + terms[1] + ... in fp32, in that order (the reference's `+=`).
 *   ws: tgsr_cycle_mse_ws_elems(...) floats (0 = a shape the entries refuse).
 * tgsr_cycle_mse_bwd - one kernel launch for all scales, gather form; grad fp32 [1] ON THE DEVICE (the gradient reaching loss[0]):
 *   d_sr HOST array of n DEVICE pointers (the array or any entry may be NULL: that gradient is not written),
 *     d_sr[i][b][c][Y][X] = grad 2 / (B C h w) sum_{y, x} WY(y, Y) WX(x, X) diff_i[b][c][y][x],   WY(y, Y) = the sum of the weights of
 *     output y whose clamped tap is Y - written completely, zeros where no tap lands (no memset);
 *   d_lr NULL, or fp32 [B][C][h][w] = -grad 2 / (B C h w) sum_i diff_i.   One of the outputs at least.
 *   16-byte stores into d_sr[i] where it is 16-byte aligned and W[i] % 4 == 0, element by element otherwise.
 * No atomics: the same bits on every run.  Every entry returns TGSR_EINVAL without launching (and without touching an output) for a
 * NULL required pointer (the arrays and every sr[i] included), a size < 1 or > 65536, n outside [1, 8], or a backward call that asks
 * for no output.
 */
int64_t tgsr_cycle_mse_ws_elems(const int* H, const int* W, int n, int B, int C, int h, int w);
int tgsr_cycle_mse_fwd(const float* const* sr, const int* H, const int* W, int n, const float* lr, int B, int C, int h, int w,
                       float* ws, float* diff, float* loss, float* terms, void* stream);
int tgsr_cycle_mse_bwd(const float* grad, const float* diff, const int* H, const int* W, int n, int B, int C, int h, int w,
                       float* const* d_sr, float* d_lr, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TGSR_HIP_H */
