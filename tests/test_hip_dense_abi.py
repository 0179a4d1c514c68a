"""GPU: the GEMM, CA_NET, loss, optimizer and pointwise kernels (tgsr_amd/csrc/tgsr_gemm.hip, tgsr_text_tail.hip, tgsr_misc.hip, and
tgsr_sumpool2x2 of tgsr_bn.hip) held to their C ABI contract, called directly through ctypes.

    tgsr_conv1x1_fwd   tgsr_linear_fwd   tgsr_rowdot_fwd   tgsr_rowdot_bwd   tgsr_ca_net_fwd   tgsr_text_tail_fwd (+ tgsr_word_project_fwd)
    tgsr_glu   tgsr_bn_fold   tgsr_to_uint8   tgsr_multi_copy   tgsr_axpy_images   tgsr_axpy_map_fwd / _bwd   tgsr_affine_act_fwd / _bwd
    tgsr_weighted_bce_fwd / _bwd   tgsr_adam_flat   tgsr_sumpool2x2
    (tgsr_pack_conv_weight(_dgrad), the one other launcher of tgsr_misc.hip, is held by tests/test_hip_infer_abi.py.)

The rest of the suite reaches them through the Python wrappers only: dense allocator memory, the GEMM at M % 32 == 0 and K % 64 == 0,
the row dot product at K = 512, CA_NET at aligned tdim in {256, 64, 48, 16} (ca_net_kernel never launched), the pointwise kernels at
sizes where no grid-stride loop makes a second trip, every NULL-able operand present.  Here every operand of a call lies in a
guarded arena (tests/arena.py): outputs prefilled with a pattern no arithmetic produces, in-place operands (Adam's) placed as such,
captions `width = T + 3` wide, guard bands around everything.  After a call the guard bands and the inputs hold their bits, every
output word is written and finite, a second call gives the same bits, and the values hold against the same operation in fp64 on
the CPU.

TABLE has one row per (entry point, kernel instance or code branch, dispatch condition copied from the launcher, case); refusals
are rows with case None (test_refusals).  tests/test_dense_abi_host.py checks the table against the kernel launches in the source,
the launch arithmetic restated here (every case named for a short last block, a second trip or an idle wave has one), the inputs,
and that every tolerance tells a right result from the wrong one a kernel bug would give.

Caps.  The suite's own where one exists: conv1x1 atol 5e-5 rtol 1e-4 and linear 1e-4 / 1e-4 (test_cnn_encoder_heads), CA_NET 1e-5 /
1e-5 (test_text_tail_equals_its_parts), the bce value 2e-6 max(1, |ref|) and its gradients 1e-7 / 1e-5 (tests/test_hip_gan.py), Adam
p 2e-7 / 2e-6, m 1e-8 / 1e-5, v 1e-10 / 1e-5 (tests/test_hip_optim.py).  Where none exists the cap comes from the operation's
length, with u = 2^-24 the unit roundoff of fp32:
  * a sum of n products, each partial sum rounded once, is within n u sum|a_k b_k| of the exact one in ANY order (dot_cap); where
    the kernel's order is fixed and shorter than n - the row dot product's 256 lanes and 8-level tree - n is the longest chain of
    roundings one product passes through (rowdot_depth);
  * a result that is one fma, one product or one copy is the fp64 value correctly rounded: within 0.5 ulp (half_ulp) or the same
    bits.  LeakyReLU's negative side is a second operation on the rounded value, in the kernel as in the reference's BatchNorm
    followed by LeakyReLU: 0.5 ulp of 0.2f x that rounded value;
  * GLU and bn_fold are a few correctly rounded operations and a library exponential: a relative cap of that many u, stated where
    the cap is defined.
The GEMMs, both row dot products and CA_NET also carry the ratio bound of tests/test_hip_parity_margin.py: max |kernel - f64| over
max |torch CPU fp32 - f64| over a case's outputs, R below.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24            # unit roundoff of fp32

# max |kernel - f64| / max |torch CPU fp32 - f64| over a case's outputs: 1.5 x the largest measured ratio of the group, rounded up to
# one decimal (the rule of R_* in tests/test_hip_rnn_abi.py).  Measured on the MI355X over every case of the group (the DENSE_RATIO
# lines this file prints; profiles/HISTORY.md).
R = {
    "gemm_nn": 1.5,       # measured 0.33 .. 1.00 over 5 cases (1.00: the exact tile and 1 / 1 / 1, the CPU run's bits in the worst element)
    "gemm_nt": 5.9,       # measured 1.00 .. 3.92 over 5 cases (largest: 256 / 2048 at B = 5, 2.8e-6: one chain of 2048 products per output)
    "rowdot_fwd": 1.5,    # measured 0.08 .. 1.00 over 7 cases (smallest: K = 8192, 256 lanes and a tree; 1.00 at K = 4 and K = 1)
    "rowdot_bwd": 1.7,    # measured 1.00 .. 1.08 over 5 cases, dx and dw together (dx alone is the CPU's bits: 1.00)
    "ca_mfma": 2.0,       # measured 0.83 .. 1.30 over 5 cases (largest: tdim = 48, the scalar-operand loop)
    "ca_rows": 2.5,       # measured 0.48 .. 1.66 over 5 cases (largest: tdim = 40, ncf = 130, two float4 accumulators per row)
}

CONV1X1, LINEAR, ROWDOT, ROWDOT_BWD = "tgsr_conv1x1_fwd", "tgsr_linear_fwd", "tgsr_rowdot_fwd", "tgsr_rowdot_bwd"
CA_NET, TAIL = "tgsr_ca_net_fwd", "tgsr_text_tail_fwd"
GLU, BN_FOLD, TO_U8, MULTI_COPY, AXPY = "tgsr_glu", "tgsr_bn_fold", "tgsr_to_uint8", "tgsr_multi_copy", "tgsr_axpy_images"
MAP_FWD, MAP_BWD, AFF_FWD, AFF_BWD = "tgsr_axpy_map_fwd", "tgsr_axpy_map_bwd", "tgsr_affine_act_fwd", "tgsr_affine_act_bwd"
BCE_FWD, BCE_BWD, ADAM, SUMPOOL = "tgsr_weighted_bce_fwd", "tgsr_weighted_bce_bwd", "tgsr_adam_flat", "tgsr_sumpool2x2"

K_NN, K_NT = "gemm_bias_kernel<false>", "gemm_bias_kernel<true>"
K_ROWDOT, K_ROWDOT_BWD, K_CA_ROWS, K_CA_MFMA, K_TAIL = ("rowdot_fwd_kernel", "rowdot_bwd_kernel", "ca_net_kernel", "ca_net_mfma_kernel",
                                                        "text_tail_kernel")
K_GLU, K_FOLD, K_U8, K_COPY, K_AXPY = "glu_kernel", "bn_fold_kernel", "to_uint8_kernel", "multi_copy_kernel", "axpy_images_kernel"
K_MAP, K_MAP_BWD, K_AFF, K_AFF_BWD = "axpy_map_kernel", "axpy_map_bwd_kernel", "affine_act_kernel", "affine_act_bwd_kernel"
K_BCE, K_BCE_BWD, K_ADV, K_ADAM, K_POOL = ("weighted_bce_kernel", "weighted_bce_bwd_kernel", "adam_advance_kernel", "adam_flat_kernel",
                                           "sumpool2x2_kernel")


# ----------------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------------
def _g(Cout, K, N, B=1, bias=True, skew=False):
    """A GEMM case: conv1x1 Cout / Cin = K / S = N on B samples; linear Cout / K on N = B rows (its B field stays 1)."""
    return dict(Cout=Cout, K=K, N=N, B=B, bias=bias, skew=skew)


def _r(K, B, bias=True):
    return dict(K=K, B=B, bias=bias)


def _rb(K, B, dx=True, dw=True, skew=False):
    return dict(K=K, B=B, dx=dx, dw=dw, skew=skew)


def _ca(tdim, ncf, B, c_code=True, sat=False, skew_w=False, skew_s=False):
    return dict(tdim=tdim, ncf=ncf, B=B, c_code=c_code, sat=sat, skew_w=skew_w, skew_s=skew_s)


def _t(B, T, idf, cdf, nsets, tdim, ncf):
    return dict(B=B, T=T, idf=idf, cdf=cdf, nsets=nsets, tdim=tdim, ncf=ncf, width=T + 3)


NN_TAILS, NN_TILE, NN_ONE, NN_MODEL = _g(40, 70, 130, B=2), _g(32, 64, 32, bias=False), _g(1, 1, 1), _g(256, 768, 289)
NN_SKEW = _g(40, 70, 130, B=2, skew=True)
NT_33, NT_130, NT_MODEL, NT_ONE, NT_NOBIAS = _g(40, 70, 33), _g(40, 70, 130), _g(256, 2048, 5), _g(1, 1, 1), _g(40, 70, 33, bias=False)
RD_MODEL, RD_1028, RD_4, RD_1023, RD_257, RD_1, RD_NOBIAS = (_r(8192, 3), _r(1028, 2), _r(4, 1), _r(1023, 2), _r(257, 3), _r(1, 1),
                                                             _r(1028, 2, bias=False))
RB_1, RB_3, RB_NODX, RB_NODW, RB_SKEW = _rb(257, 1), _rb(257, 3), _rb(257, 3, dx=False), _rb(257, 3, dw=False), _rb(257, 3, skew=True)
CA_256, CA_64, CA_320, CA_48, CA_16 = (_ca(256, 100, 17), _ca(64, 6, 1, c_code=False), _ca(320, 1, 17, sat=True), _ca(48, 6, 17),
                                       _ca(16, 1, 1, c_code=False))
CR_40, CR_13, CR_13_1, CR_64_W, CR_64_S = (_ca(40, 130, 2), _ca(13, 5, 2), _ca(13, 1, 1, c_code=False), _ca(64, 6, 2, skew_w=True),
                                           _ca(64, 6, 2, skew_s=True))
TT_17, TT_32, TT_1 = _t(17, 5, 64, 41, 3, 48, 6), _t(2, 32, 32, 9, 1, 64, 3), _t(1, 1, 32, 1, 4, 16, 1)
GLU_BIG = 349527                                   # x 3 rows: 1 048 581 values, past the 4096 x 256 grid cap
BCE_ONE, BCE_BOTH, BCE_NODA, BCE_NODB = (dict(na=1, nb=0, da=True, db=False), dict(na=300, nb=217, da=True, db=True),
                                         dict(na=300, nb=217, da=False, db=True), dict(na=300, nb=217, da=True, db=False))
AFF_SMALL, AFF_WIDE = dict(B=2, C=3, HW=12), dict(B=2, C=2048, HW=516)
MAP_SMALL, MAP_BIG = dict(BC=3, HW=4), dict(BC=33, HW=64000)
AXPY_NUMEL = (4, 12, 12288, 524292)                # the last: 131 073 float4, past the 512 x 256 grid cap
COPY_BYTES = (0, 4, 16, 20, 64, 262192, 64, 8, 12, 32, 48, 4, 0, 1024, 36, 16)     # [4]: src one word off; [6]: dst one word off
U8_BIG = 2097156                                   # 524 289 float4, past the 2048 x 256 grid cap
ADAM_N = (1, 3, 7, 1029, 4194311)                  # the last: 1 048 577 float4, past the 4096 x 256 grid cap, and a tail of 3
ADAM_HYPER = dict(lr=2e-3, b1=0.5, b2=0.999, eps=1e-8)          # tests/test_hip_optim.py's
ADAM_ADVANCE = (1, 1, 1, 0)                        # three steps, then a further range of the third step

TABLE = (
    # entry point, kernel instance / branch, dispatch condition (copied from the launcher), case (None: refused; test_refusals)
    [(CONV1X1, K_NN, "always; M = 40: two row blocks, the last 8 rows (`m0 + r < M`, `m < M`); K = 70: two chunks, the last 6 (`k0 + k "
      "< K`, `kk < K`); N = 130: a second workgroup of 2 columns, three idle waves (`n < N`); B = 2: blockIdx.z strides", NN_TAILS),
     (CONV1X1, K_NN, "M = 32, K = 64, N = 32: the exact tile; bias == NULL", NN_TILE),
     (CONV1X1, K_NN, "M = K = N = 1", NN_ONE),
     (CONV1X1, K_NN, "the model's head: 256 / 768 / 289 at B = 1", NN_MODEL),
     (CONV1X1, K_NN, "x, w, out one word off 16 bytes (dword reads): the aligned call's bits", NN_SKEW),
     (LINEAR, K_NT, "always; N = B = 33: the second wave holds one column (`n0 + r < N`); M = 40, K = 70", NT_33),
     (LINEAR, K_NT, "N = B = 130: a second workgroup", NT_130),
     (LINEAR, K_NT, "the model's: 256 / 2048 at B = 5", NT_MODEL),
     (LINEAR, K_NT, "M = K = N = 1", NT_ONE),
     (LINEAR, K_NT, "bias == NULL", NT_NOBIAS),
     (ROWDOT, K_ROWDOT + " float4", "(K & 3) == 0: the model's K = 8192, B = 3: eight trips", RD_MODEL),
     (ROWDOT, K_ROWDOT + " float4", "(K & 3) == 0: K = 1028: thread 0 alone makes a second trip", RD_1028),
     (ROWDOT, K_ROWDOT + " float4", "(K & 3) == 0: K = 4: one thread", RD_4),
     (ROWDOT, K_ROWDOT + " scalar", "(K & 3) != 0: K = 1023: four trips, the last one short", RD_1023),
     (ROWDOT, K_ROWDOT + " scalar", "(K & 3) != 0: K = 257: thread 0 alone makes a second trip", RD_257),
     (ROWDOT, K_ROWDOT + " scalar", "(K & 3) != 0: K = 1", RD_1),
     (ROWDOT, K_ROWDOT + " float4", "bias == NULL", RD_NOBIAS),
     (ROWDOT, "no instance", "x or w not 16-byte aligned: refused at every K, the scalar branch's included (include/tgsr_hip.h says "
      "aligned)", None),
     (ROWDOT_BWD, K_ROWDOT_BWD, "always; K = 257: the second workgroup holds one k; B = 1", RB_1),
     (ROWDOT_BWD, K_ROWDOT_BWD, "K = 257, B = 3", RB_3),
     (ROWDOT_BWD, K_ROWDOT_BWD, "dx == NULL", RB_NODX),
     (ROWDOT_BWD, K_ROWDOT_BWD, "dw == NULL", RB_NODW),
     (ROWDOT_BWD, K_ROWDOT_BWD, "every operand one word off 16 bytes (dword reads): the aligned call's bits", RB_SKEW),
     (CA_NET, K_CA_MFMA + " float4", "tdim % 16 == 0 and tdim % 64 == 0 and sent_emb, w aligned: tdim = 256, one full trip of four "
      "float4; ncf = 100, B = 17: a second sample block of one", CA_256),
     (CA_NET, K_CA_MFMA + " float4", "... tdim = 64: `in` clips three of four; ncf = 6: a ragged block of 4-channel groups; B = 1; "
      "c_code == eps == NULL", CA_64),
     (CA_NET, K_CA_MFMA + " float4", "... tdim = 320: a second trip; ncf = 1; gate pre-activations of +-30 and beyond", CA_320),
     (CA_NET, K_CA_MFMA + " scalar", "tdim % 16 == 0 and tdim % 64 != 0: tdim = 48, kc = 3", CA_48),
     (CA_NET, K_CA_MFMA + " scalar", "... tdim = 16, kc = 1; ncf = 1, B = 1; c_code == eps == NULL", CA_16),
     (CA_NET, K_CA_ROWS + " float4", "tdim % 16 != 0: tdim = 40, (tdim & 7) == 0 and w aligned; ncf = 130: halves of 65 / 65, 4 ni = 260 "
      "> 256: a second trip", CR_40),
     (CA_NET, K_CA_ROWS + " scalar", "tdim % 16 != 0: tdim = 13; ncf = 5: halves of 3 and 2", CR_13),
     (CA_NET, K_CA_ROWS + " scalar", "... ncf = 1: the second half-block has ni = 0; c_code == eps == NULL", CR_13_1),
     (CA_NET, K_CA_ROWS + " scalar", "tdim % 64 == 0 and w one word off 16 bytes", CR_64_W),
     (CA_NET, K_CA_ROWS + " float4", "tdim % 64 == 0 and only sent_emb one word off 16 bytes: float4 on w", CR_64_S),
     (CA_NET, K_CA_ROWS, "(tdim + 4 ncf) * 4 > 60 KB of LDS: refused (tdim = 13, ncf = 3840)", None),
     (TAIL, K_TAIL, "always; B = 17: a second CA_NET sample block; idf = 64: two channel blocks; cdf = 41: odd; nsets = 3; tdim = 48", TT_17),
     (TAIL, K_TAIL, "T = 32: no padding column; tdim = 64: float4 operands", TT_32),
     (TAIL, K_TAIL, "T = 1, B = 1, nsets = 4, tdim = 16, cdf = 1", TT_1),
     (TAIL, "no instance", "width < T, nsets > 4, T > 32, idf % 32, tdim % 16, tdim % 64 == 0 with sent_emb or ca_w off 16 bytes: "
      "refused", None),
     (GLU, K_GLU + " forward", "dy == NULL; outer = 3, half = 7; gates of +-100 and 0", dict(half=7, bwd=False)),
     (GLU, K_GLU + " backward", "dy != NULL; outer = 3, half = 7", dict(half=7, bwd=True)),
     (GLU, K_GLU + " forward", "n = 3 x 349 527 > 4096 x 256: a second trip of the grid-stride loop", dict(half=GLU_BIG, bwd=False)),
     (GLU, K_GLU + " backward", "... the backward", dict(half=GLU_BIG, bwd=True)),
     (BN_FOLD, K_FOLD, "always; C = 1", dict(C=1)),
     (BN_FOLD, K_FOLD, "C = 257: the second workgroup holds one channel; one running_var of 0", dict(C=257)),
     (TO_U8, K_U8 + " float4", "(n & 3) == 0, x 16-byte and out 4-byte aligned; n = 2 097 156 > 4 x 2048 x 256: a second trip",
      dict(n=U8_BIG, skew=0, lead=0)),
     (TO_U8, K_U8 + " scalar", "(n & 3) != 0: n = 7", dict(n=7, skew=0, lead=0)),
     (TO_U8, K_U8 + " scalar", "x one word off 16 bytes", dict(n=1028, skew=1, lead=0)),
     (TO_U8, K_U8 + " scalar", "out one byte off a word", dict(n=1028, skew=0, lead=1)),
     (MULTI_COPY, K_COPY, "16 segments: 0, 4, 16 and 20 bytes, 16-byte multiples with src / dst one word off (the dword path), 262 192 "
      "bytes > 16 x 64 x 256: a second trip", dict(bytes=COPY_BYTES)),
     (MULTI_COPY, "no launch", "every size 0: TGSR_OK in front of the launch", None),
     (MULTI_COPY, "no instance", "17 segments, a size that is no multiple of 4, a negative size: refused", None),
     (AXPY, K_AXPY, "always; n = 4 images of 4, 12, 12 288 and 524 292 floats: the last past the 512 x 256 grid cap", dict(n=4)),
     (AXPY, K_AXPY, "n = 3", dict(n=3)), (AXPY, K_AXPY, "n = 2", dict(n=2)), (AXPY, K_AXPY, "n = 1: 4 floats", dict(n=1)),
     (AXPY, "no instance", "n > 4, numel % 4, numel > 2^31 - 1, an operand off 16 bytes: refused", None),
     (MAP_FWD, K_MAP, "always; BC = 3, HW = 4: hw4 = 1", MAP_SMALL),
     (MAP_FWD, K_MAP, "BC = 33, HW = 64 000: n4 = 528 000 > 2048 x 256: a second trip", MAP_BIG),
     (MAP_BWD, K_MAP_BWD, "always; BC = 3, HW = 4", dict(MAP_SMALL, ds=True, damap=True)),
     (MAP_BWD, K_MAP_BWD, "BC = 33, HW = 64 000: 63 workgroups, the last 128 float4", dict(MAP_BIG, ds=True, damap=True)),
     (MAP_BWD, K_MAP_BWD, "ds == NULL", dict(MAP_SMALL, ds=False, damap=True)),
     (MAP_BWD, K_MAP_BWD, "damap == NULL, s == NULL", dict(MAP_SMALL, ds=True, damap=False)),
     (AFF_FWD, K_AFF, "always; act 0; C = 3, B = 2, HW = 12", dict(AFF_SMALL, act=0)),
     (AFF_FWD, K_AFF, "act 2", dict(AFF_SMALL, act=2)),
     (AFF_FWD, K_AFF, "C = 2048, B = 2, HW = 516: grid y = 1, two trips, the first across the sample boundary; act 2", dict(AFF_WIDE, act=2)),
     (AFF_BWD, K_AFF_BWD, "always; act 0 with out == NULL", dict(AFF_SMALL, act=0)),
     (AFF_BWD, K_AFF_BWD, "act 2", dict(AFF_SMALL, act=2)),
     (AFF_BWD, K_AFF_BWD, "C = 2048, B = 2, HW = 516; act 2", dict(AFF_WIDE, act=2)),
     (AFF_FWD, "no instance", "HW % 4, act not in {0, 2}, raw / out off 16 bytes: refused, as in " + AFF_BWD, None),
     (BCE_FWD, K_BCE, "always; na = 1, nb = 0, b == NULL", BCE_ONE),
     (BCE_FWD, K_BCE, "na = 300, nb = 217: a second trip, the a / b seam inside a wave", BCE_BOTH),
     (BCE_BWD, K_BCE_BWD, "always; na = 1, nb = 0, b == db == NULL", BCE_ONE),
     (BCE_BWD, K_BCE_BWD, "na = 300, nb = 217: three workgroups, the last 5 logits", BCE_BOTH),
     (BCE_BWD, K_BCE_BWD, "da == NULL", BCE_NODA),
     (BCE_BWD, K_BCE_BWD, "db == NULL", BCE_NODB)]
    + [(ADAM, K_ADV + " + " + K_ADAM, "advance != 0 three times, then " + K_ADAM + " alone; n = %d: n4 = %d, a tail of %d%s; wd = %g"
        % (n, n >> 2, n & 3, "; past the 4096 x 256 grid cap" if (n >> 2) > 4096 * 256 else "", wd), dict(n=n, wd=wd))
       for n in ADAM_N for wd in (0.0, 0.01)]
    + [(ADAM, "no instance", "betas outside [0, 1), eps < 0, lr < 0 or NaN, an operand off 16 bytes: refused", None),
       (SUMPOOL, K_POOL + " float2", "x 8-byte aligned; BC = 3, output 3 x 5", dict(BC=3, H=3, W=5, skew=0)),
       (SUMPOOL, K_POOL + " scalar", "x one word off 8 bytes: single floats, the aligned call's bits", dict(BC=3, H=3, W=5, skew=1))])


def _rows(*entries):
    return [r for r in TABLE if r[0] in entries and r[3] is not None]


def _cases(*entries):
    out = []
    for r in _rows(*entries):
        if r[3] not in out:
            out.append(r[3])
    return out


def case_id(c):
    def one(v):
        return ("y" if v else "n") if isinstance(v, bool) else "x%d" % len(v) if isinstance(v, tuple) else "%d" % v if isinstance(v, int) else "%g" % v
    return "-".join("%s%s" % (k, one(v)) for k, v in c.items())


def row_id(r):
    return r[0][5:] + "-" + case_id(r[3])


# ----------------------------------------------------------------------------------------------------------------------------
# The launchers' arithmetic, restated
# ----------------------------------------------------------------------------------------------------------------------------
def gemm_plan(M, N, K):
    """gemm_launch: grid (ceil(N / 128), ceil(M / 32), batch), four waves of 32 columns, K in chunks of 64."""
    last_cols = (N - 1) % 128 + 1
    return dict(row_blocks=-(-M // 32), last_rows=(M - 1) % 32 + 1, col_blocks=-(-N // 128), last_cols=last_cols,
                idle_waves=4 - -(-last_cols // 32), last_wave_cols=(N - 1) % 32 + 1, k_chunks=-(-K // 64), last_k=(K - 1) % 64 + 1)


def rowdot_plan(K):
    """rowdot_fwd_kernel: 256 threads; float4 when K % 4 == 0 (thread t: k = 4 t, step 1024), single floats otherwise (step 256)."""
    vec = K % 4 == 0
    step = 1024 if vec else 256
    trips = -(-K // step)
    last = K - (trips - 1) * step                    # what the last trip holds
    return dict(branch="float4" if vec else "scalar", trips=trips, last_threads=-(-last // 4) if vec else last)


def rowdot_depth(K):
    """The longest chain of roundings a product of rowdot_fwd_kernel passes through: its thread's running sum (four products per trip
    on the float4 branch, one on the scalar one), the 8 levels of the tree, the bias."""
    p = rowdot_plan(K)
    return (4 if p["branch"] == "float4" else 1) * p["trips"] + 8 + 1


def ca_form(tdim, sent_addr, w_addr):
    """tgsr_ca_net_fwd's dispatch: (kernel, operand reads)."""
    if tdim % 16 == 0 and (tdim % 64 != 0 or (sent_addr | w_addr) % 16 == 0):
        return K_CA_MFMA, "float4" if (tdim >> 4) % 4 == 0 else "scalar"
    return K_CA_ROWS, "float4" if tdim % 8 == 0 and w_addr % 16 == 0 else "scalar"


def ca_rows_plan(tdim, ncf):
    """ca_net_kernel: grid (B, 2), per = (ncf + 1) / 2 outputs per half, 4 ni rows over 256 threads; LDS as the launcher sizes it."""
    per = (ncf + 1) // 2
    ni = [min(per, ncf - h * per) for h in range(2)]
    return dict(per=per, ni=ni, trips=[-(-4 * n // 256) for n in ni], lds_bytes=(tdim + 4 * ncf + 8) * 4,
                refused=(tdim + 4 * ncf) * 4 > 60 * 1024)


def ca_mfma_plan(tdim, ncf, B):
    """ca_net_block: grid (ceil(ncf / 4), ceil(B / 16)); kc = tdim / 16 products per (wave, lane group), float4 trips of 16."""
    kc = tdim >> 4
    return dict(kc=kc, float4=kc % 4 == 0, trips=-(-kc // 16), last_float4=((kc - 1) % 16) // 4 + 1, chan_blocks=-(-ncf // 4),
                last_chans=(ncf - 1) % 4 + 1, sample_blocks=-(-B // 16), last_samples=(B - 1) % 16 + 1)


def stride_plan(work, threads_per_block, cap):
    """A grid-stride launch of min(ceil(work / threads), cap) blocks: (blocks, trips of the busiest thread, threads in the last trip)."""
    blocks = max(1, min(-(-work // threads_per_block), cap))
    per_trip = blocks * threads_per_block
    trips = -(-work // per_trip)
    return dict(blocks=blocks, trips=trips, last=work - (trips - 1) * per_trip)


def affine_plan(B, C, HW):
    """affine_grid_y and the kernels' loop: float4 e = (blockIdx.y * 256 + t) * 4, step gridDim.y * 1024, over B * HW."""
    per = (B * HW + 1023) // 1024
    gy = max(1, min((2048 + C - 1) // C, per))
    return dict(grid_y=gy, trips=-(-(B * HW) // (gy * 1024)), crosses=HW < min(B * HW, gy * 1024) and B > 1)


def adam_plan(n):
    n4 = n >> 2
    p = stride_plan(max(n4, 1), 256, 4096)
    return dict(n4=n4, tail=n - 4 * n4, blocks=p["blocks"], trips=-(-n4 // (p["blocks"] * 256)) if n4 else 0)


# ----------------------------------------------------------------------------------------------------------------------------
# Comparing
# ----------------------------------------------------------------------------------------------------------------------------
def close(got, ref, tol, what=""):
    """|got - ref| <= atol + rtol |ref| everywhere; atol may be a tensor (a cap per element)."""
    atol, rtol = tol
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d of %d values beyond the cap, worst |err| %.3g at |ref| %.3g" % (
        what, int(bad.sum()), bad.numel(), float(err.max()), float(ref.abs().flatten()[int(err.argmax())]))


def moved(ref, other, tol):
    atol, rtol = tol
    return bool(((ref.double() - other.double()).abs() > atol + rtol * ref.double().abs()).any())


def dot_cap(n, absdot):
    """n roundings over a sum whose terms' magnitudes add up to `absdot` (a tensor): n u sum|a b|, and 1 % for u^2 terms."""
    return 1.01 * n * U * absdot.double()


def half_ulp(ref64):
    """Half the spacing of fp32 at the fp64 value: what one correctly rounded operation is within."""
    r = ref64.double().abs().float()
    up = torch.nextafter(r, torch.full_like(r, float("inf"))).double() - r.double()
    return 0.5 * up * (1 + 1e-9) + 1e-45          # (the fp64 reference's own rounding)


def rounded(ref64):
    return ref64.double().float()


def max_dist(xs, refs):
    return max(float((x.double() - r.double()).abs().max()) for x, r in zip(xs, refs))


def ratio_ok(tag, group, got, ref64, ref32):
    """max |kernel - f64| against max |CPU fp32 - f64| over the listed outputs together."""
    own, cpu = max_dist(got, ref64), max_dist(ref32, ref64)
    print("DENSE_RATIO %s %s own %.4g cpu %.4g ratio %s" % (group, tag, own, cpu, "%.3f" % (own / cpu) if cpu else "-"))
    assert cpu > 0.0, "%s: the CPU fp32 run is exact: the case says nothing" % tag
    assert R[group] is not None, "no measured bound for " + group
    assert own <= R[group] * cpu, "%s %s: max |kernel - f64| = %.3g is %.2f x the CPU fp32 run's %.3g (bound %.1f)" % (
        tag, group, own, own / cpu, cpu, R[group])


def same_bits(a, b):
    if a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _key(c):
    return tuple(sorted(c.items()))


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * m for s, m in zip(seed, (1, 1009, 9176, 31337, 77, 5, 3))))


# ----------------------------------------------------------------------------------------------------------------------------
# Calls
# ----------------------------------------------------------------------------------------------------------------------------
def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    from tgsr_amd import ops
    return ops._stream()


def _p(r):
    return r.ptr if r is not None else None


def _twice(a, call, outs):
    """The call, the arena's contract, the call again from the same state: the contract again and the same bits in every output."""
    M, _ = _lib()
    assert call() == M.OK
    a.check()
    got = [o.read() for o in outs]
    a.rearm()
    assert call() == M.OK
    a.check()
    for g, o in zip(got, outs):
        assert same_bits(g, o.read()), "a second call gives other bits"
    return got


def _ptrs(regions):
    return (ctypes.c_void_p * len(regions))(*[r.address for r in regions])


def _i64s(v):
    return (ctypes.c_int64 * len(v))(*v)


# ----------------------------------------------------------------------------------------------------------------------------
# The GEMM: tgsr_conv1x1_fwd (NN), tgsr_linear_fwd (NT)
# ----------------------------------------------------------------------------------------------------------------------------
TOL_GEMM = {False: (5e-5, 1e-4), True: (1e-4, 1e-4)}          # test_cnn_encoder_heads: emb_features, emb_cnn_code


@functools.lru_cache(maxsize=None)
def _gemm_inputs(nt, key):
    c = dict(key)
    g = _gen(c["Cout"], c["K"], c["N"], c["B"], nt)
    x = torch.randn(c["N"], c["K"], generator=g) if nt else torch.randn(c["B"], c["K"], c["N"], generator=g)
    return dict(x=x, w=(torch.rand(c["Cout"], c["K"], generator=g) * 2 - 1) / c["K"] ** 0.5, bias=torch.randn(c["Cout"], generator=g))


def gemm_inputs(nt, c):
    return _gemm_inputs(nt, _key(dict(c, skew=False, bias=True)))


def gemm_reference(nt, c, i, dtype=torch.float64, variant=""):
    """out[b][o][s] = sum_k w[o][k] x[b][k][s] + bias[o] (NN) / out[n][o] = sum_k w[o][k] x[n][k] + bias[o] (NT), by torch on the CPU.
    variant: "k_last" - the last k never enters (a K guard one short); "bias_row" - bias of row m - 1."""
    x, w, bias = i["x"].to(dtype), i["w"].to(dtype).clone(), i["bias"].to(dtype)
    if variant == "k_last":
        w[:, -1] = 0
    if variant == "bias_row":
        bias = torch.roll(bias, 1)
    if nt:
        return F.linear(x, w, bias if c["bias"] else None)
    return F.conv1d(x, w[:, :, None], bias if c["bias"] else None)


@functools.lru_cache(maxsize=None)
def _gemm_refs(nt, key):
    c = dict(key)
    i = gemm_inputs(nt, c)
    return gemm_reference(nt, c, i), gemm_reference(nt, c, i, torch.float32)


def gemm_refs(nt, c):
    return _gemm_refs(nt, _key(c))


def run_gemm(L, nt, c, i, skew):
    s = 1 if skew else 0
    a = Arena(DEV)
    x, w = a.place_input(i["x"], skew=s), a.place_input(i["w"], skew=s)
    bias = a.place_input(i["bias"], skew=s) if c["bias"] else None
    out = a.place_output((c["N"], c["Cout"]) if nt else (c["B"], c["Cout"], c["N"]), skew=s)
    assert x.address % 16 == 4 * s and w.address % 16 == 4 * s and out.address % 16 == 4 * s

    def call():
        if nt:
            return L.tgsr_linear_fwd(x.ptr, c["N"], c["K"], w.ptr, _p(bias), c["Cout"], out.ptr, _stream())
        return L.tgsr_conv1x1_fwd(x.ptr, c["B"], c["K"], c["N"], w.ptr, _p(bias), c["Cout"], out.ptr, _stream())
    return _twice(a, call, [out])[0]


@pytest.mark.parametrize("row", _rows(CONV1X1, LINEAR), ids=row_id)
def test_gemm_entry_points(row):
    entry, instance, _cond, c = row
    nt = entry == LINEAR
    assert instance == (K_NT if nt else K_NN)
    _, L = _lib()
    i = gemm_inputs(nt, c)
    ref64, ref32 = gemm_refs(nt, c)
    out = run_gemm(L, nt, c, i, c["skew"])
    if c["skew"]:
        assert same_bits(out, run_gemm(L, nt, c, i, False)), "one word off 16 bytes changes the bits"
    close(out, ref64, TOL_GEMM[nt], entry)
    ratio_ok(case_id(c), "gemm_nt" if nt else "gemm_nn", [out], [ref64], [ref32])


# ----------------------------------------------------------------------------------------------------------------------------
# The row dot product: tgsr_rowdot_fwd, tgsr_rowdot_bwd
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rowdot_inputs(K, B):
    g = _gen(K, B, 7)
    return dict(x=torch.randn(B, K, generator=g), w=(torch.rand(K, generator=g) * 2 - 1) / K ** 0.5, bias=torch.randn(1, generator=g),
                dy=torch.randn(B, generator=g))


def rowdot_inputs(c):
    return _rowdot_inputs(c["K"], c["B"])


def rowdot_reference(c, i, dtype=torch.float64, variant=""):
    """out[b] = sum_k x[b][k] w[k] + bias[0].  variant "stops_short": the sum stops at (K - 1) & ~3 (K & ~3 where K % 4 != 0: a float4
    loop without its tail; one float4 short where K % 4 == 0)."""
    n = (c["K"] - 1) & ~3 if variant == "stops_short" else c["K"]
    out = i["x"].to(dtype)[:, :n] @ i["w"].to(dtype)[:n]
    return out + i["bias"].to(dtype) if c["bias"] else out


def rowdot_cap(c, i):
    absdot = (i["x"].double().abs() * i["w"].double().abs()).sum(1) + (i["bias"].double().abs() if c["bias"] else 0.0)
    return dot_cap(rowdot_depth(c["K"]), absdot), 0.0


def run_rowdot(L, c, i):
    a = Arena(DEV)
    x, w = a.place_input(i["x"]), a.place_input(i["w"])
    bias = a.place_input(i["bias"]) if c["bias"] else None
    out = a.place_output((c["B"],))
    return _twice(a, lambda: L.tgsr_rowdot_fwd(x.ptr, w.ptr, _p(bias), out.ptr, c["B"], c["K"], _stream()), [out])[0]


@pytest.mark.parametrize("row", _rows(ROWDOT), ids=row_id)
def test_rowdot_forward(row):
    _entry, instance, _cond, c = row
    assert instance == K_ROWDOT + " " + rowdot_plan(c["K"])["branch"]
    _, L = _lib()
    i = rowdot_inputs(c)
    out = run_rowdot(L, c, i)
    ref64 = rowdot_reference(c, i)
    close(out, ref64, rowdot_cap(c, i), ROWDOT)
    ratio_ok(case_id(c), "rowdot_fwd", [out], [ref64], [rowdot_reference(c, i, torch.float32)])


def rowdot_bwd_reference(c, i, dtype=torch.float64):
    """dx[b][k] = dy[b] w[k]; dw[k] = sum_b dy[b] x[b][k]."""
    dy, x, w = i["dy"].to(dtype), i["x"].to(dtype), i["w"].to(dtype)
    return dy[:, None] * w[None, :], dy @ x


def run_rowdot_bwd(L, c, i, skew):
    s = 1 if skew else 0
    B, K = c["B"], c["K"]
    a = Arena(DEV)
    dy, x, w = a.place_input(i["dy"], skew=s), a.place_input(i["x"], skew=s), a.place_input(i["w"], skew=s)
    dx, dw = a.place_output((B, K), skew=s, written=c["dx"]), a.place_output((K,), skew=s, written=c["dw"])
    outs = [r for r, given in ((dx, c["dx"]), (dw, c["dw"])) if given]
    got = _twice(a, lambda: L.tgsr_rowdot_bwd(dy.ptr, x.ptr if c["dw"] else None, w.ptr if c["dx"] else None,
                                              dx.ptr if c["dx"] else None, dw.ptr if c["dw"] else None, B, K, _stream()), outs)
    return dict(zip([k for k in ("dx", "dw") if c[k]], got))


@pytest.mark.parametrize("row", _rows(ROWDOT_BWD), ids=row_id)
def test_rowdot_backward(row):
    """dx is one product: the fp64 product (exact) rounded once, bit for bit.  dw is a chain of B fmas."""
    c = row[3]
    _, L = _lib()
    i = rowdot_inputs(c)
    got = run_rowdot_bwd(L, c, i, c["skew"])
    if c["skew"]:
        al = run_rowdot_bwd(L, c, i, False)
        assert all(same_bits(got[k], al[k]) for k in got), "one word off 16 bytes changes the bits"
    dx64, dw64 = rowdot_bwd_reference(c, i)
    dx32, dw32 = rowdot_bwd_reference(c, i, torch.float32)
    if c["dx"]:
        assert same_bits(got["dx"], rounded(dx64)), "dx is not the correctly rounded product"
    if c["dw"]:
        cap = dot_cap(c["B"], (i["dy"].double().abs()[:, None] * i["x"].double().abs()).sum(0))
        close(got["dw"], dw64, (cap, 0.0), "dw")
    keys = [k for k in ("dx", "dw") if c[k]]
    ref = dict(dx=(dx64, dx32), dw=(dw64, dw32))
    ratio_ok(case_id(c), "rowdot_bwd", [got[k] for k in keys], [ref[k][0] for k in keys], [ref[k][1] for k in keys])


# ----------------------------------------------------------------------------------------------------------------------------
# CA_NET: tgsr_ca_net_fwd
# ----------------------------------------------------------------------------------------------------------------------------
TOL_CA = (1e-5, 1e-5)                                          # test_text_tail_equals_its_parts


@functools.lru_cache(maxsize=None)
def _ca_inputs(tdim, ncf, B, sat):
    g = _gen(tdim, ncf, B, sat)
    sent, w, bias = torch.randn(B, tdim, generator=g), torch.randn(4 * ncf, tdim, generator=g) * 0.1, torch.randn(4 * ncf, generator=g)
    if sat:                                                    # the gates' pre-activations: standard deviation 30
        w[2 * ncf:] *= 30.0 / (0.1 * tdim ** 0.5)
        bias[2 * ncf:] *= 30.0
    return dict(sent=sent, w=w, bias=bias, eps=torch.randn(B, ncf, generator=g))


def ca_inputs(c):
    return _ca_inputs(c["tdim"], c["ncf"], c["B"], c.get("sat", False))


def ca_reference(c, i, dtype=torch.float64, variant=""):
    """util.py:372-400: y = fc(sent); (mu | logvar) = y[:, :2 ncf] * sigmoid(y[:, 2 ncf:]); c_code = eps * exp(logvar / 2) + mu; also the
    gates' pre-activations.  variant "rows_swapped": Linear rows i + 2 ncf (mu's gate) and ncf + i (logvar's value) change places."""
    ncf = c["ncf"]
    y = F.linear(i["sent"].to(dtype), i["w"].to(dtype), i["bias"].to(dtype))
    if variant == "rows_swapped":
        y = torch.cat([y[:, :ncf], y[:, 2 * ncf:3 * ncf], y[:, ncf:2 * ncf], y[:, 3 * ncf:]], 1)
    h = y[:, :2 * ncf] * torch.sigmoid(y[:, 2 * ncf:])
    mu, lv = h[:, :ncf], h[:, ncf:]
    return dict(mu=mu, logvar=lv, c_code=i["eps"].to(dtype) * torch.exp(0.5 * lv) + mu, gates=y[:, 2 * ncf:])


@functools.lru_cache(maxsize=None)
def _ca_refs(key):
    c = dict(key)
    i = ca_inputs(c)
    return ca_reference(c, i), ca_reference(c, i, torch.float32)


def ca_refs(c):
    return _ca_refs(_key(c))


def run_ca_net(L, c, i, form=None):
    """tgsr_ca_net_fwd in an arena of its own: dict of mu, logvar and, where asked for, c_code; `form`: the (kernel, reads) the
    operands' addresses must select."""
    B, ncf = c["B"], c["ncf"]
    a = Arena(DEV)
    sent, w = a.place_input(i["sent"], skew=1 if c.get("skew_s") else 0), a.place_input(i["w"], skew=1 if c.get("skew_w") else 0)
    bias, eps = a.place_input(i["bias"]), a.place_input(i["eps"])
    cc = a.place_output((B, ncf), written=c.get("c_code", False))
    mu, lv = a.place_output((B, ncf)), a.place_output((B, ncf))
    if form is not None:
        assert ca_form(c["tdim"], sent.address, w.address) == form
    given = c.get("c_code", False)
    got = _twice(a, lambda: L.tgsr_ca_net_fwd(sent.ptr, w.ptr, bias.ptr, eps.ptr if given else None, B, c["tdim"], ncf,
                                              cc.ptr if given else None, mu.ptr, lv.ptr, _stream()), [mu, lv] + ([cc] if given else []))
    return dict(zip(("mu", "logvar", "c_code"), got))


@pytest.mark.parametrize("row", _rows(CA_NET), ids=row_id)
def test_ca_net(row):
    _entry, instance, _cond, c = row
    kernel, reads = instance.split(" ")
    _, L = _lib()
    i = ca_inputs(c)
    got = run_ca_net(L, c, i, form=(kernel, reads))
    ref64, ref32 = ca_refs(c)
    for k in got:
        close(got[k], ref64[k], TOL_CA, k)
    ratio_ok(case_id(c), "ca_mfma" if kernel == K_CA_MFMA else "ca_rows", [got[k] for k in got], [ref64[k] for k in got],
             [ref32[k] for k in got])


# ----------------------------------------------------------------------------------------------------------------------------
# The text tail: tgsr_text_tail_fwd = tgsr_word_project_fwd + CA_NET's mu / logvar + the caption mask
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_inputs(key):
    c = dict(key)
    g = _gen(c["B"], c["T"], c["tdim"], c["nsets"])
    i = dict(ca_inputs(dict(tdim=c["tdim"], ncf=c["ncf"], B=c["B"])))
    i["words"] = torch.randn(c["B"], c["cdf"], c["T"], generator=g)
    i["w_ctx"] = tuple(torch.randn(c["idf"], c["cdf"], generator=g) for _ in range(c["nsets"]))
    cap = torch.randint(0, 4, (c["B"], c["width"]), generator=g)
    cap[0, 0], cap[-1, c["T"] - 1] = 3, 0                      # both values inside the captions, whatever the draw
    if c["B"] * c["T"] == 1:
        cap[0, 0] = 0
    i["captions"] = cap
    return i


def tail_inputs(c):
    return _tail_inputs(_key(c))


def project_reference(c, i, dtype=torch.float64):
    """src[set][b][i][t] = sum_c w[set][i][c] words[b][c][t], zero in the columns t >= T of the 32; and sum_c |w| |words|."""
    src = torch.zeros(c["nsets"], c["B"], c["idf"], 32, dtype=dtype)
    mag = torch.zeros(c["nsets"], c["B"], c["idf"], 32, dtype=torch.float64)
    for k, w in enumerate(i["w_ctx"]):
        src[k, :, :, :c["T"]] = torch.einsum("ic,bct->bit", w.to(dtype), i["words"].to(dtype))
        mag[k, :, :, :c["T"]] = torch.einsum("ic,bct->bit", w.double().abs(), i["words"].double().abs())
    return src, mag


def run_word_project(L, c, i):
    a = Arena(DEV)
    words, ws = a.place_input(i["words"]), [a.place_input(w) for w in i["w_ctx"]]
    out = a.place_output((c["nsets"], c["B"], c["idf"], 32))
    return _twice(a, lambda: L.tgsr_word_project_fwd(words.ptr, _ptrs(ws), c["nsets"], c["B"], c["idf"], c["cdf"], c["T"], out.ptr,
                                                     _stream()), [out])[0]


def run_text_tail(L, c, i):
    B, T, ncf = c["B"], c["T"], c["ncf"]
    a = Arena(DEV)
    words, ws = a.place_input(i["words"]), [a.place_input(w) for w in i["w_ctx"]]
    sent, w, bias = a.place_input(i["sent"]), a.place_input(i["w"]), a.place_input(i["bias"])
    cap = a.place_input(i["captions"])
    src, mu, lv = a.place_output((c["nsets"], B, c["idf"], 32)), a.place_output((B, ncf)), a.place_output((B, ncf))
    mask = a.place_output_u8((B, T))
    return _twice(a, lambda: L.tgsr_text_tail_fwd(words.ptr, _ptrs(ws), c["nsets"], B, c["idf"], c["cdf"], T, src.ptr, sent.ptr, w.ptr,
                                                  bias.ptr, c["tdim"], ncf, mu.ptr, lv.ptr, cap.ptr, c["width"], mask.ptr, _stream()),
                  [src, mu, lv, mask])


@pytest.mark.parametrize("row", _rows(TAIL), ids=row_id)
def test_text_tail(row):
    c = row[3]
    _, L = _lib()
    i = tail_inputs(c)
    src, mu, lv, mask = run_text_tail(L, c, i)
    assert same_bits(src, run_word_project(L, c, i)), "src_out differs from tgsr_word_project_fwd"
    ca = run_ca_net(L, c, i, form=(K_CA_MFMA, "float4" if c["tdim"] % 64 == 0 else "scalar"))
    assert same_bits(mu, ca["mu"]) and same_bits(lv, ca["logvar"]), "mu / logvar differ from tgsr_ca_net_fwd"
    assert torch.equal(mask, (i["captions"][:, :c["T"]] == 0).to(torch.uint8)), "the mask bytes"
    src64, mag = project_reference(c, i)
    assert float(src[..., c["T"]:].abs().sum()) == 0.0, "the padding columns are exactly zero"
    close(src, src64, (dot_cap(c["cdf"], mag) + 1e-45, 0.0), "src_out")
    ref64 = ca_reference(c, i)
    close(mu, ref64["mu"], TOL_CA, "mu")
    close(lv, ref64["logvar"], TOL_CA, "logvar")


# ----------------------------------------------------------------------------------------------------------------------------
# GLU: tgsr_glu
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def glu_inputs(half):
    g = _gen(half, 11)
    x, dy = torch.randn(3, 2, half, generator=g), torch.randn(3, half, generator=g)
    x[:, 1] *= 4.0
    x[0, 1, :3] = torch.tensor([100.0, -100.0, 0.0])           # saturated both ways, and the middle
    return dict(x=x, dy=dy)


def glu_reference(i, bwd, dtype=torch.float64):
    """util.py:45-53: out = v sigmoid(g); the backward dv = dy s, dg = dy v s (1 - s).  Returns (result, cap).
    Cap: s = 1 / (1 + expf(-g)) is a library exponential (2 ulp), an add and a correctly rounded division: 4 u relative, 8 u with
    the product that follows; dg = ((dy v) s) (1 - s) is three products on s and (1 - s), whose absolute error of 4 u s + u is
    nothing relative to 1 but everything relative to itself as s -> 1: 10 u relative and 4 u |dy v s| on top.  A gate of -100
    overflows expf to inf: s = 0 where fp64 has 4e-44 - below fp32's normal range, hence the 1e-37."""
    x, dy = i["x"].to(dtype), i["dy"].to(dtype)
    v, s = x[:, 0], torch.sigmoid(x[:, 1])
    if not bwd:
        ref = v * s
        return ref, 8 * U * ref.double().abs() + 1e-37
    ref = torch.stack([dy * s, dy * v * s * (1 - s)], 1)
    cap = 8 * U * ref.double().abs() + 1e-37
    cap[:, 1] = 10 * U * ref[:, 1].double().abs() + 4 * U * (dy * v * s).double().abs() + 1e-37
    return ref, cap


@pytest.mark.parametrize("row", _rows(GLU), ids=row_id)
def test_glu(row):
    c = row[3]
    _, L = _lib()
    i = glu_inputs(c["half"])
    a = Arena(DEV)
    x = a.place_input(i["x"])
    dy = a.place_input(i["dy"]) if c["bwd"] else None
    out = a.place_output((3, 2, c["half"]) if c["bwd"] else (3, c["half"]))
    got = _twice(a, lambda: L.tgsr_glu(x.ptr, _p(dy), out.ptr, 3, c["half"], _stream()), [out])[0]
    ref, cap = glu_reference(i, c["bwd"])
    close(got, ref, (cap, 0.0), GLU)


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_bn_fold, tgsr_sumpool2x2
# ----------------------------------------------------------------------------------------------------------------------------
BN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def fold_inputs(C):
    g = _gen(C, 13)
    i = dict(weight=torch.randn(C, generator=g), bias=torch.randn(C, generator=g), mean=torch.randn(C, generator=g),
             var=torch.rand(C, generator=g) + 0.1)
    i["var"][C // 2] = 0.0
    return i


def fold_reference(i, dtype=torch.float64):
    """scale = weight / sqrt(var + eps), shift = bias - mean scale, and their caps: add, square root and division are correctly
    rounded (1.5 u together, 3 u allowed); shift adds one product and one difference (or one fma) on the rounded scale."""
    eps = torch.tensor(BN_EPS, dtype=torch.float32).to(dtype)
    scale = i["weight"].to(dtype) / torch.sqrt(i["var"].to(dtype) + eps)
    shift = i["bias"].to(dtype) - i["mean"].to(dtype) * scale
    ms = (i["mean"].double() * scale.double()).abs()
    cap_scale, cap_shift = 3 * U * scale.double().abs(), 2 * U * (i["bias"].double().abs() + ms) + 3 * U * ms
    return scale, shift, cap_scale, cap_shift


@pytest.mark.parametrize("row", _rows(BN_FOLD), ids=row_id)
def test_bn_fold(row):
    C = row[3]["C"]
    _, L = _lib()
    i = fold_inputs(C)
    a = Arena(DEV)
    w, b, m, v = (a.place_input(i[k]) for k in ("weight", "bias", "mean", "var"))
    scale, shift = a.place_output((C,)), a.place_output((C,))
    got = _twice(a, lambda: L.tgsr_bn_fold(w.ptr, b.ptr, m.ptr, v.ptr, BN_EPS, scale.ptr, shift.ptr, C, _stream()), [scale, shift])
    s64, t64, cap_s, cap_t = fold_reference(i)
    close(got[0], s64, (cap_s, 0.0), "scale")
    close(got[1], t64, (cap_t, 0.0), "shift")


@functools.lru_cache(maxsize=None)
def pool_input(BC, H, W):
    return torch.randn(BC, 2 * H, 2 * W, generator=_gen(BC, H, W, 17))


def pool_reference(x):
    """(x00 + x01) + (x10 + x11) in fp32 - three additions in the kernel's order, so bit for bit - and in fp64."""
    return (x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])


def run_sumpool(L, c, x, skew):
    a = Arena(DEV)
    xin = a.place_input(x, skew=skew)
    out = a.place_output((c["BC"], c["H"], c["W"]))
    assert xin.address % 8 == 4 * skew
    return _twice(a, lambda: L.tgsr_sumpool2x2(xin.ptr, c["BC"], c["H"], c["W"], out.ptr, _stream()), [out])[0]


@pytest.mark.parametrize("row", _rows(SUMPOOL), ids=row_id)
def test_sumpool2x2(row):
    """include/tgsr_hip.h: x needs a float's alignment; 8-byte loads where it has 8, single floats where not, the same bits."""
    c = row[3]
    _, L = _lib()
    x = pool_input(c["BC"], c["H"], c["W"])
    got = run_sumpool(L, c, x, c["skew"])
    assert same_bits(got, pool_reference(x)), "not (x00 + x01) + (x10 + x11)"
    close(got, pool_reference(x.double()), (dot_cap(2, pool_reference(x.double().abs())), 0.0), SUMPOOL)


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_to_uint8
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def u8_input(n):
    """Both clips, +-inf, every k / 127.5 - 1, every half-way point (k + 0.5) / 127.5 - 1, then random values 1.2 wide; no NaN."""
    k = torch.arange(0, 256, dtype=torch.float32)
    special = torch.cat([torch.tensor([float("-inf"), float("inf"), -3.0, 3.0]), (k[:255] + 0.5) / 127.5 - 1.0, k / 127.5 - 1.0])
    if n < special.numel():
        return torch.cat([special[:4], special[4 + 100:4 + 101], special[4 + 255 + 7:4 + 255 + 8], torch.tensor([0.3])])[:n].clone()
    x = torch.randn(n, generator=_gen(n, 19)) * 1.2
    x[:special.numel()] = special
    return x


def u8_reference(x):
    """trainer_objective.py:153-155 in numpy's float32 arithmetic, as in test_to_uint8_bytes_match_numpy."""
    a = x.numpy()
    return torch.from_numpy(np.round(np.maximum(0, np.minimum(255, (a + np.float32(1.0)) * np.float32(127.5)))).astype(np.uint8))


def u8_branch(n, x_addr, out_addr):
    return "float4" if n % 4 == 0 and x_addr % 16 == 0 and out_addr % 4 == 0 else "scalar"


@pytest.mark.parametrize("row", _rows(TO_U8), ids=row_id)
def test_to_uint8(row):
    _entry, instance, _cond, c = row
    _, L = _lib()
    x = u8_input(c["n"])
    ref = u8_reference(x)
    a = Arena(DEV)
    xin = a.place_input(x, skew=c["skew"])
    out = a.place_output_u8((c["n"],), lead=c["lead"], expect=ref)
    assert instance == K_U8 + " " + u8_branch(c["n"], xin.address, out.address)
    got = _twice(a, lambda: L.tgsr_to_uint8(xin.ptr, out.ptr, c["n"], _stream()), [out])[0]
    assert torch.equal(got, ref), "%d bytes differ from numpy's" % int((got != ref).sum())


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_multi_copy, tgsr_axpy_images
# ----------------------------------------------------------------------------------------------------------------------------
COPY_SRC_SKEW, COPY_DST_SKEW = 4, 6


def copy_branch(nbytes, dst_addr, src_addr):
    return "uint4" if (nbytes | dst_addr | src_addr) % 16 == 0 else "dword"


def test_multi_copy():
    _, L = _lib()
    g = _gen(23)
    n = len(COPY_BYTES)
    data = [torch.randint(0, 2 ** 31 - 1, (max(b // 4, 1),), generator=g, dtype=torch.int64).to(torch.int32) for b in COPY_BYTES]
    a = Arena(DEV)
    srcs = [a.place_input(d, skew=1 if k == COPY_SRC_SKEW else 0) for k, d in enumerate(data)]
    dsts = [a.place_output((d.numel(),), dtype=torch.int32, written=b > 0, skew=1 if k == COPY_DST_SKEW else 0)
            for k, (d, b) in enumerate(zip(data, COPY_BYTES))]
    branches = [copy_branch(b, d.address, s.address) for b, d, s in zip(COPY_BYTES, dsts, srcs)]
    assert branches[COPY_SRC_SKEW] == branches[COPY_DST_SKEW] == "dword" and branches[2] == branches[5] == "uint4" and branches[3] == "dword"
    live = [k for k in range(n) if COPY_BYTES[k] > 0]
    got = _twice(a, lambda: L.tgsr_multi_copy(n, _ptrs(dsts), _ptrs(srcs), _i64s(COPY_BYTES), _stream()), [dsts[k] for k in live])
    for k, out in zip(live, got):
        assert torch.equal(out, data[k]), "segment %d" % k


@functools.lru_cache(maxsize=None)
def axpy_inputs():
    g = _gen(29)
    return dict(t=tuple(torch.randn(m, generator=g) for m in AXPY_NUMEL), s=tuple(torch.randn(m, generator=g) for m in AXPY_NUMEL))


AXPY_ALPHA = 0.3


@pytest.mark.parametrize("row", _rows(AXPY), ids=row_id)
def test_axpy_images(row):
    """out = fma(alpha, s, t): within 0.5 ulp of t + alpha s in fp64 (alpha as the float the kernel is handed)."""
    n = row[3]["n"]
    _, L = _lib()
    i = axpy_inputs()
    pick = list(range(4))[-n:] if n > 1 else [0]               # n = 1: the 4 floats alone; otherwise the n largest
    a = Arena(DEV)
    ts, ss = [a.place_input(i["t"][k]) for k in pick], [a.place_input(i["s"][k]) for k in pick]
    outs = [a.place_output((AXPY_NUMEL[k],)) for k in pick]
    got = _twice(a, lambda: L.tgsr_axpy_images(n, _ptrs(outs), _ptrs(ts), _ptrs(ss), _i64s([AXPY_NUMEL[k] for k in pick]), AXPY_ALPHA,
                                               _stream()), outs)
    al = float(np.float32(AXPY_ALPHA))
    for k, out in zip(pick, got):
        ref = i["t"][k].double() + al * i["s"][k].double()
        close(out, ref, (half_ulp(ref), 0.0), "image %d" % k)


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_axpy_map_fwd / _bwd
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def map_inputs(BC, HW):
    g = _gen(BC, HW, 31)
    return dict(t=torch.randn(BC, HW, generator=g), s=torch.randn(BC, HW, generator=g), amap=torch.randn(HW, generator=g) + 1.0,
                dy=torch.randn(BC, HW, generator=g))


def map_reference(i, variant=""):
    """out[bc][p] = t + amap[p] s in fp64.  variant "flat_index": the map read at the flat float4 index instead of i % hw4 - what lies
    behind the map taken as zeros."""
    amap = i["amap"].double()[None, :]
    if variant == "flat_index":
        amap = torch.zeros_like(i["s"], dtype=torch.float64)
        amap[0] = i["amap"].double()
    return i["t"].double() + amap * i["s"].double()


@pytest.mark.parametrize("row", _rows(MAP_FWD), ids=row_id)
def test_axpy_map_forward(row):
    c = row[3]
    _, L = _lib()
    i = map_inputs(c["BC"], c["HW"])
    a = Arena(DEV)
    t, s, amap = a.place_input(i["t"]), a.place_input(i["s"]), a.place_input(i["amap"])
    out = a.place_output((c["BC"], c["HW"]))
    got = _twice(a, lambda: L.tgsr_axpy_map_fwd(t.ptr, s.ptr, amap.ptr, out.ptr, c["BC"], c["HW"], _stream()), [out])[0]
    ref = map_reference(i)
    close(got, ref, (half_ulp(ref), 0.0), MAP_FWD)


@pytest.mark.parametrize("row", _rows(MAP_BWD), ids=row_id)
def test_axpy_map_backward(row):
    """ds = amap dy: one product, the exact fp64 product rounded once, bit for bit.  damap: a chain of BC fmas in plane order."""
    c = row[3]
    BC, HW = c["BC"], c["HW"]
    _, L = _lib()
    i = map_inputs(BC, HW)
    a = Arena(DEV)
    dy, s, amap = a.place_input(i["dy"]), a.place_input(i["s"]), a.place_input(i["amap"])
    ds, damap = a.place_output((BC, HW), written=c["ds"]), a.place_output((HW,), written=c["damap"])
    outs = [r for r, given in ((ds, c["ds"]), (damap, c["damap"])) if given]
    got = _twice(a, lambda: L.tgsr_axpy_map_bwd(dy.ptr, s.ptr if c["damap"] else None, amap.ptr, ds.ptr if c["ds"] else None,
                                                damap.ptr if c["damap"] else None, BC, HW, _stream()), outs)
    got = dict(zip([k for k in ("ds", "damap") if c[k]], got))
    if c["ds"]:
        assert same_bits(got["ds"], rounded(i["amap"].double()[None, :] * i["dy"].double())), "ds is not the correctly rounded product"
    if c["damap"]:
        prod = i["dy"].double() * i["s"].double()
        close(got["damap"], prod.sum(0), (dot_cap(BC, prod.abs().sum(0)), 0.0), "damap")


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_affine_act_fwd / _bwd
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def affine_inputs(B, C, HW):
    g = _gen(B, C, HW, 37)
    return dict(raw=torch.randn(B, C, HW, generator=g), scale=torch.randn(C, generator=g), shift=torch.randn(C, generator=g) * 0.5,
                dy=torch.randn(B, C, HW, generator=g))


def _per_channel(v, like, variant):
    """v[c] spread over [B][C][HW]; variant "b_c_swapped": the channel taken as if the tensor were [C][B][HW]."""
    B, C, HW = like.shape
    if variant == "b_c_swapped":
        return v.double()[(torch.arange(B * C) // B)].reshape(B, C, 1)
    return v.double()[None, :, None]


def affine_reference(i, act, variant=""):
    """out = act(raw scale[c] + shift[c]); the fma in fp64, LeakyReLU(0.2) on its value rounded to fp32 (the module's second op)."""
    y = i["raw"].double() * _per_channel(i["scale"], i["raw"], variant) + _per_channel(i["shift"], i["raw"], variant)
    if act == 2:
        y = torch.where(y > 0, y, float(np.float32(0.2)) * rounded(y).double())
    return y


def affine_bwd_reference(i, act, out, variant=""):
    """draw = dy scale[c], x 0.2f on its rounded value where the forward output is not positive."""
    r = i["dy"].double() * _per_channel(i["scale"], i["dy"], variant)
    if act == 2:
        r = torch.where(out > 0, r, float(np.float32(0.2)) * rounded(r).double())
    return r


def run_affine_fwd(L, c, i):
    B, C, HW = c["B"], c["C"], c["HW"]
    a = Arena(DEV)
    raw, scale, shift = a.place_input(i["raw"]), a.place_input(i["scale"]), a.place_input(i["shift"])
    out = a.place_output((B, C, HW))
    return _twice(a, lambda: L.tgsr_affine_act_fwd(raw.ptr, scale.ptr, shift.ptr, out.ptr, B, C, HW, c["act"], _stream()), [out])[0]


@pytest.mark.parametrize("row", _rows(AFF_FWD), ids=row_id)
def test_affine_act_forward(row):
    c = row[3]
    _, L = _lib()
    i = affine_inputs(c["B"], c["C"], c["HW"])
    got = run_affine_fwd(L, c, i)
    ref = affine_reference(i, c["act"])
    close(got, ref, (half_ulp(ref), 0.0), AFF_FWD)
    assert bool((got > 0).any()) and bool((got < 0).any())


@pytest.mark.parametrize("row", _rows(AFF_BWD), ids=row_id)
def test_affine_act_backward(row):
    """The forward output it reads is the fp64 reference rounded once; act 0 is handed out == NULL."""
    c = row[3]
    B, C, HW = c["B"], c["C"], c["HW"]
    _, L = _lib()
    i = affine_inputs(B, C, HW)
    fwd = rounded(affine_reference(i, c["act"]))
    a = Arena(DEV)
    dy, scale = a.place_input(i["dy"]), a.place_input(i["scale"])
    out = a.place_input(fwd) if c["act"] == 2 else None
    draw = a.place_output((B, C, HW))
    got = _twice(a, lambda: L.tgsr_affine_act_bwd(dy.ptr, _p(out), scale.ptr, draw.ptr, B, C, HW, c["act"], _stream()), [draw])[0]
    ref = affine_bwd_reference(i, c["act"], fwd)
    close(got, ref, (half_ulp(ref), 0.0), AFF_BWD)


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_weighted_bce_fwd / _bwd
# ----------------------------------------------------------------------------------------------------------------------------
TOL_BCE_GRAD = (1e-7, 1e-5)                                    # tests/test_hip_gan.py


def bce_value_cap(ref):
    return 2e-6 * max(1.0, abs(float(ref)))                    # tests/test_hip_gan.py


@functools.lru_cache(maxsize=None)
def bce_inputs(na, nb):
    """Logits of +-100, +-20, 0 and random ones, targets of 0, 1 and 0.3 against each of them, every weight another value."""
    n = na + nb
    g = _gen(na, nb, 41)
    l = torch.randn(n, generator=g) * 3
    t = torch.tensor([0.0, 1.0, 0.3])[torch.arange(n) % 3]
    if n >= 15:
        l[:15] = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0]).repeat_interleave(3)
        l[na - 3:na + 3] = torch.tensor([100.0, -20.0, 0.0, -100.0, 20.0, 0.0])[:min(6, n - na + 3)]      # ... on both sides of the seam
    w = (1.0 + torch.arange(n) / 1000.0) / n
    return dict(a=l[:na].clone(), b=l[na:].clone(), t=t, w=w, dy=torch.tensor([1.7]))


def bce_reference(i, dtype=torch.float64, variant=""):
    """sum_i w[i] BCEWithLogits(l[i], t[i]) over l = [a; b], and d/dl = dy w (sigmoid(l) - t).  variant "b_weights": the b part takes
    w[i - na]; "no_target": t = 0 (for the case without a b part)."""
    na = i["a"].numel()
    l, t, w, dy = torch.cat([i["a"], i["b"]]).to(dtype), i["t"].to(dtype).clone(), i["w"].to(dtype).clone(), i["dy"].to(dtype)
    if variant == "b_weights":
        w[na:] = w[:l.numel() - na]
    if variant == "no_target":
        t[:] = 0
    value = (w * F.binary_cross_entropy_with_logits(l, t, reduction="none")).sum()
    grad = dy * w * (torch.sigmoid(l) - t)
    return value, grad[:na], grad[na:]


@pytest.mark.parametrize("row", _rows(BCE_FWD), ids=row_id)
def test_weighted_bce_forward(row):
    c = row[3]
    na, nb = c["na"], c["nb"]
    _, L = _lib()
    i = bce_inputs(na, nb)
    a = Arena(DEV)
    la, lb = a.place_input(i["a"]), a.place_input(i["b"]) if nb else None
    t, w = a.place_input(i["t"]), a.place_input(i["w"])
    out = a.place_output((1,))
    got = _twice(a, lambda: L.tgsr_weighted_bce_fwd(la.ptr, na, _p(lb), nb, t.ptr, w.ptr, out.ptr, _stream()), [out])[0]
    ref = bce_reference(i)[0]
    print("DENSE_BCE na %d nb %d |out - f64| %.3g cap %.3g" % (na, nb, abs(float(got) - float(ref)), bce_value_cap(ref)))
    assert abs(float(got) - float(ref)) <= bce_value_cap(ref)


@pytest.mark.parametrize("row", _rows(BCE_BWD), ids=row_id)
def test_weighted_bce_backward(row):
    c = row[3]
    na, nb = c["na"], c["nb"]
    _, L = _lib()
    i = bce_inputs(na, nb)
    a = Arena(DEV)
    dy, la, lb = a.place_input(i["dy"]), a.place_input(i["a"]), a.place_input(i["b"]) if nb else None
    t, w = a.place_input(i["t"]), a.place_input(i["w"])
    da, db = a.place_output((na,), written=c["da"]), a.place_output((max(nb, 1),), written=c["db"])
    outs = [r for r, given in ((da, c["da"]), (db, c["db"])) if given]
    got = _twice(a, lambda: L.tgsr_weighted_bce_bwd(dy.ptr, la.ptr, na, _p(lb), nb, t.ptr, w.ptr, da.ptr if c["da"] else None,
                                                    db.ptr if c["db"] else None, _stream()), outs)
    _, ga, gb = bce_reference(i)
    for k, out in zip([k for k in ("da", "db") if c[k]], got):
        close(out, ga if k == "da" else gb, TOL_BCE_GRAD, k)


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_adam_flat
# ----------------------------------------------------------------------------------------------------------------------------
TOL_ADAM = dict(p=(2e-7, 2e-6), m=(1e-8, 1e-5), v=(1e-10, 1e-5))          # tests/test_hip_optim.py
ADAM_STATE0 = (0.0, 0.25, 0.75)                    # step 0; the corrections hold anything before the first advance


@functools.lru_cache(maxsize=None)
def adam_inputs(n):
    g = _gen(n, 43)
    grad = torch.randn(n, generator=g)
    grad[0] = 0.0
    if n > 1:
        grad[n - 1] = 1e18                         # in the tail loop where n % 4 != 0
    if n > 4:
        grad[1], grad[4] = 1e18, 0.0               # ... and in the float4 loop
    return dict(p=torch.randn(n, generator=g), g=grad, m=torch.randn(n, generator=g) * 0.1, v=torch.rand(n, generator=g) * 0.01)


def adam_reference(i, wd, dtype=torch.float64, variant=""):
    """torch.optim.Adam's formula (no amsgrad, L2 weight decay folded into the gradient) over ADAM_ADVANCE, the step counted as the
    kernel's state does.  variant "no_bias_correction": both corrections 1; "decoupled_decay": the moments of the bare gradient,
    then p -= lr wd p."""
    h = ADAM_HYPER
    p, g0, m, v = (i[k].to(dtype).clone() for k in ("p", "g", "m", "v"))
    step, state = 0, None
    for advance in ADAM_ADVANCE:
        step += 1 if advance else 0
        bc1, bc2 = 1.0 - h["b1"] ** step, 1.0 - h["b2"] ** step
        state = (float(step), bc1, math.sqrt(bc2))
        if variant == "no_bias_correction":
            bc1 = bc2 = 1.0
        g = g0 + wd * p if wd and variant != "decoupled_decay" else g0
        m = m + (g - m) * (1.0 - h["b1"])
        v = v * h["b2"] + (1.0 - h["b2"]) * g * g
        p = p - (h["lr"] / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + h["eps"]))
        if wd and variant == "decoupled_decay":
            p = p - h["lr"] * wd * p
    return dict(p=p, m=m, v=v, state=state)


@functools.lru_cache(maxsize=None)
def _adam_ref(n, wd):
    return adam_reference(adam_inputs(n), wd)


@pytest.mark.parametrize("row", _rows(ADAM), ids=row_id)
def test_adam_flat(row):
    c = row[3]
    n, wd, h = c["n"], c["wd"], ADAM_HYPER
    _, L = _lib()
    i = adam_inputs(n)
    a = Arena(DEV)
    p, m, v = a.place_inout(i["p"]), a.place_inout(i["m"]), a.place_inout(i["v"])
    g, state = a.place_input(i["g"]), a.place_inout(torch.tensor(ADAM_STATE0))

    def call():
        for advance in ADAM_ADVANCE:
            rc = L.tgsr_adam_flat(p.ptr, g.ptr, m.ptr, v.ptr, state.ptr, n, h["lr"], h["b1"], h["b2"], h["eps"], wd, advance, _stream())
            if rc != 0:
                return rc
        return 0
    got = dict(zip(("p", "m", "v", "state"), _twice(a, call, [p, m, v, state])))
    ref = _adam_ref(n, wd)
    assert float(got["state"][0]) == 3.0, "the step count"
    assert same_bits(got["state"][1:], torch.tensor(ref["state"][1:], dtype=torch.float64).float()), "the corrections are not fp64's, rounded"
    for k in ("m", "v", "p"):
        close(got[k], ref[k], TOL_ADAM[k], k)


# ----------------------------------------------------------------------------------------------------------------------------
# Refusals: every one a host-side return in front of the first launch - the code, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------
def _I(name, dtype=torch.float32):
    return ("in", name, dtype)


def _O(name):
    return ("out", name, None)


def _N(name, default):
    return ("num", name, default)


# the arguments of every entry point, in order (the stream follows): operands as arena regions of 64 words, numbers with the value
# a valid small call takes
SPEC = {
    CONV1X1: [_I("x"), _N("B", 1), _N("Cin", 2), _N("S", 3), _I("w"), _I("bias"), _N("Cout", 2), _O("out")],
    LINEAR: [_I("x"), _N("B", 1), _N("K", 2), _I("w"), _I("bias"), _N("Cout", 2), _O("out")],
    ROWDOT: [_I("x"), _I("w"), _I("bias"), _O("out"), _N("B", 1), _N("K", 5)],
    ROWDOT_BWD: [_I("dy"), _I("x"), _I("w"), _O("dx"), _O("dw"), _N("B", 1), _N("K", 5)],
    CA_NET: [_I("sent_emb"), _I("w"), _I("bias"), _I("eps"), _N("B", 1), _N("tdim", 13), _N("ncf", 1), _O("c_code"), _O("mu"), _O("logvar")],
    GLU: [_I("x"), _I("dy"), _O("out"), _N("outer", 1), _N("half", 2)],
    BN_FOLD: [_I("weight"), _I("bias"), _I("running_mean"), _I("running_var"), _N("eps", 1e-5), _O("scale"), _O("shift"), _N("C", 2)],
    TO_U8: [_I("x"), _O("out"), _N("n", 4)],
    MAP_FWD: [_I("t"), _I("s"), _I("amap"), _O("out"), _N("BC", 1), _N("HW", 4)],
    MAP_BWD: [_I("dy"), _I("s"), _I("amap"), _O("ds"), _O("damap"), _N("BC", 1), _N("HW", 4)],
    AFF_FWD: [_I("raw"), _I("scale"), _I("shift"), _O("out"), _N("B", 1), _N("C", 1), _N("HW", 4), _N("act", 2)],
    AFF_BWD: [_I("dy"), _I("out"), _I("scale"), _O("draw"), _N("B", 1), _N("C", 1), _N("HW", 4), _N("act", 2)],
    BCE_FWD: [_I("a"), _N("na", 2), _I("b"), _N("nb", 2), _I("target"), _I("weight"), _O("out")],
    BCE_BWD: [_I("dy"), _I("a"), _N("na", 2), _I("b"), _N("nb", 2), _I("target"), _I("weight"), _O("da"), _O("db")],
    ADAM: [_O("param"), _I("grad"), _O("exp_avg"), _O("exp_avg_sq"), _O("state"), _N("n", 4), _N("lr", 1e-3), _N("beta1", 0.5),
           _N("beta2", 0.999), _N("eps", 1e-8), _N("weight_decay", 0.0), _N("advance", 1)],
    SUMPOOL: [_I("x"), _N("BC", 1), _N("H", 1), _N("W", 1), _O("out")],
    TAIL: [_I("words"), ("ptrs", "w_ctx", 4), _N("nsets", 1), _N("B", 1), _N("idf", 32), _N("cdf", 1), _N("T", 1), _O("src_out"),
           _I("sent_emb"), _I("ca_w"), _I("ca_b"), _N("tdim", 16), _N("ncf", 1), _O("mu"), _O("logvar"), _I("captions", torch.int64),
           _N("width", 1), ("out8", "mask", None)],
    MULTI_COPY: [_N("n", 2), ("ptrs", "dst", 17), ("ptrs", "src", 17), ("nums", "nbytes", (4, 8) + (4,) * 15)],
    AXPY: [_N("n", 2), ("ptrs", "out", 5), ("ptrs", "t", 5), ("ptrs", "s", 5), ("nums", "numel", (4, 8, 4, 4, 4)), _N("alpha", 0.5)],
}


def _refusal_call(L, a, entry, null=None, skew=(), entry_null=None, nums=None, **kw):
    """A call of `entry` on zero operands with every output placed written=False.  null: the operand handed over as NULL; skew: the
    operands one word off 16 bytes; entry_null = (array, index): that entry of a host array of pointers is NULL; nums = (array,
    index, value): that entry of a host array of numbers, every entry where index is None; every other keyword replaces the number of that name."""
    spec = SPEC[entry]
    assert null is None or null in [s[1] for s in spec]
    assert all(k in [s[1] for s in spec if s[0] == "num"] for k in kw), kw
    held = []
    for kind, name, arg in spec:
        s = 1 if name in skew else 0
        if kind == "in":
            held.append(a.place_input(torch.zeros(64 // (2 if arg == torch.int64 else 1), dtype=arg), skew=s))
        elif kind == "out":
            held.append(a.place_output((64,), written=False, skew=s))
        elif kind == "out8":
            held.append(a.place_output_u8((256,), written=False))
        elif kind == "ptrs":
            held.append([a.place_output((8,), written=False, skew=1 if (name, k) in skew else 0) for k in range(arg)])
        else:
            held.append(None)
    args = []
    for (kind, name, arg), r in zip(spec, held):
        if name == null:
            args.append(None)
        elif kind in ("in", "out", "out8"):
            args.append(r.ptr)
        elif kind == "ptrs":
            arr = _ptrs(r)
            if entry_null is not None and entry_null[0] == name:
                arr[entry_null[1]] = None
            args.append(arr)
        elif kind == "nums":
            v = list(arg)
            if nums is not None and nums[0] == name:
                v = [nums[2]] * len(v) if nums[1] is None else v[:nums[1]] + [nums[2]] + v[nums[1] + 1:]
            args.append(_i64s(v))
        else:
            args.append(kw.get(name, arg))
    fn = getattr(L, entry)
    return lambda: fn(*args, _stream())


# the operands each entry point refuses as NULL with TGSR_EINVAL (those that may be NULL are not here)
NULLS = {
    CONV1X1: ("x", "w", "out"), LINEAR: ("x", "w", "out"), ROWDOT: ("x", "w", "out"), ROWDOT_BWD: ("dy",),
    CA_NET: ("sent_emb", "w", "bias", "mu", "logvar", "eps"), GLU: ("x", "out"),
    BN_FOLD: ("weight", "bias", "running_mean", "running_var", "scale", "shift"), TO_U8: ("x", "out"),
    MAP_FWD: ("t", "s", "amap", "out"), MAP_BWD: ("dy", "amap", "s"), AFF_FWD: ("raw", "scale", "shift", "out"),
    AFF_BWD: ("dy", "scale", "draw", "out"), BCE_FWD: ("a", "b", "target", "weight", "out"), BCE_BWD: ("dy", "a", "b", "target", "weight"),
    ADAM: ("param", "grad", "exp_avg", "exp_avg_sq", "state"), SUMPOOL: ("x", "out"),
    TAIL: ("words", "w_ctx", "src_out", "sent_emb", "ca_w", "ca_b", "mu", "logvar", "captions", "mask"),
    MULTI_COPY: ("dst", "src", "nbytes"), AXPY: ("out", "t", "s", "numel"),
}
# the sizes each takes and refuses below 1 with TGSR_EINVAL
SIZES = {
    CONV1X1: ("B", "Cin", "S", "Cout"), LINEAR: ("B", "K", "Cout"), ROWDOT: ("B", "K"), ROWDOT_BWD: ("B", "K"), CA_NET: ("B", "tdim", "ncf"),
    GLU: ("outer", "half"), BN_FOLD: ("C",), TO_U8: ("n",), MAP_FWD: ("BC", "HW"), MAP_BWD: ("BC", "HW"), AFF_FWD: ("B", "C", "HW"),
    AFF_BWD: ("B", "C", "HW"), BCE_FWD: ("na",), BCE_BWD: ("na",), ADAM: ("n",), SUMPOOL: ("BC", "H", "W"),
    TAIL: ("nsets", "B", "cdf", "T", "tdim", "ncf"), MULTI_COPY: ("n",), AXPY: ("n",),
}
# the operands each refuses one word off 16 bytes with TGSR_EUNSUPPORTED
UNALIGNED = {
    ROWDOT: ("x", "w"), MAP_FWD: ("t", "s", "amap", "out"), MAP_BWD: ("dy", "s", "amap", "ds", "damap"), AFF_FWD: ("raw", "out"),
    AFF_BWD: ("dy", "out", "draw"), ADAM: ("param", "grad", "exp_avg", "exp_avg_sq"), AXPY: (("out", 1), ("t", 0), ("s", 1)),
}


def refusals():
    """(name, entry point, arguments of _refusal_call, code)."""
    out = []
    for e, names in NULLS.items():
        out += [("%s-%s-null" % (e[5:], n), e, dict(null=n), "EINVAL") for n in names]
    for e, names in SIZES.items():
        out += [("%s-%s-0" % (e[5:], n), e, {n: 0}, "EINVAL") for n in names]
    for e, names in UNALIGNED.items():
        out += [("%s-%s-unaligned" % (e[5:], n if isinstance(n, str) else "%s[%d]" % n), e, dict(skew=(n,)), "EUNSUPPORTED") for n in names]
    inv, uns = "EINVAL", "EUNSUPPORTED"
    out += [
        ("rowdot_fwd-unaligned-scalar-K", ROWDOT, dict(skew=("x",), K=7), uns),             # the scalar branch would run: refused all the same
        ("rowdot_bwd-dx-without-w", ROWDOT_BWD, dict(null="w"), inv), ("rowdot_bwd-dw-without-x", ROWDOT_BWD, dict(null="x"), inv),
        ("ca_net_fwd-lds-limit", CA_NET, dict(tdim=13, ncf=3840), uns), ("ca_net_fwd-lds-limit-tdim", CA_NET, dict(tdim=15361, ncf=1), uns),
        ("text_tail_fwd-width-below-T", TAIL, dict(T=5, width=4), inv), ("text_tail_fwd-nsets-5", TAIL, dict(nsets=5), uns),
        ("text_tail_fwd-T-33", TAIL, dict(T=33, width=33), uns), ("text_tail_fwd-idf-48", TAIL, dict(idf=48), uns),
        ("text_tail_fwd-idf-0", TAIL, dict(idf=0), uns), ("text_tail_fwd-tdim-40", TAIL, dict(tdim=40), uns),
        ("text_tail_fwd-tdim-64-sent-unaligned", TAIL, dict(tdim=64, skew=("sent_emb",)), uns),
        ("text_tail_fwd-tdim-64-w-unaligned", TAIL, dict(tdim=64, skew=("ca_w",)), uns),
        ("text_tail_fwd-w_ctx-entry-null", TAIL, dict(entry_null=("w_ctx", 0)), inv),
        ("multi_copy-17", MULTI_COPY, dict(n=17), uns), ("multi_copy-odd-size", MULTI_COPY, dict(nums=("nbytes", 1, 6)), uns),
        ("multi_copy-negative-size", MULTI_COPY, dict(nums=("nbytes", 0, -4)), inv),
        ("multi_copy-size-2^31", MULTI_COPY, dict(nums=("nbytes", 1, 2 ** 31)), uns),
        ("multi_copy-dst-entry-null", MULTI_COPY, dict(entry_null=("dst", 1)), inv),
        ("multi_copy-src-entry-null", MULTI_COPY, dict(entry_null=("src", 0)), inv),
        ("multi_copy-all-zero", MULTI_COPY, dict(n=16, nums=("nbytes", None, 0)), "OK"),
        ("axpy_images-5", AXPY, dict(n=5), uns), ("axpy_images-numel-6", AXPY, dict(nums=("numel", 1, 6)), uns),
        ("axpy_images-numel-0", AXPY, dict(nums=("numel", 0, 0)), inv), ("axpy_images-numel-2^31", AXPY, dict(nums=("numel", 1, 2 ** 31)), uns),
        ("axpy_images-t-entry-null", AXPY, dict(entry_null=("t", 1)), inv),
        ("axpy_map_fwd-HW-6", MAP_FWD, dict(HW=6), uns), ("axpy_map_bwd-HW-6", MAP_BWD, dict(HW=6), uns),
        ("affine_act_fwd-HW-6", AFF_FWD, dict(HW=6), uns), ("affine_act_bwd-HW-6", AFF_BWD, dict(HW=6), uns),
        ("affine_act_fwd-act-1", AFF_FWD, dict(act=1), inv), ("affine_act_bwd-act-3", AFF_BWD, dict(act=3), inv),
        ("weighted_bce_fwd-nb-negative", BCE_FWD, dict(nb=-1), inv), ("weighted_bce_bwd-nb-negative", BCE_BWD, dict(nb=-1), inv),
        ("adam_flat-beta1-1", ADAM, dict(beta1=1.0), inv), ("adam_flat-beta1-negative", ADAM, dict(beta1=-0.1), inv),
        ("adam_flat-beta2-1", ADAM, dict(beta2=1.0), inv), ("adam_flat-beta2-negative", ADAM, dict(beta2=-0.1), inv),
        ("adam_flat-beta1-nan", ADAM, dict(beta1=float("nan")), inv), ("adam_flat-lr-nan", ADAM, dict(lr=float("nan")), inv),
        ("adam_flat-lr-negative", ADAM, dict(lr=-1e-3), inv), ("adam_flat-eps-negative", ADAM, dict(eps=-1e-8), inv),
        ("adam_flat-eps-nan", ADAM, dict(eps=float("nan")), inv),
    ]
    return out


def test_refusals():
    """Bad operands and sizes, shapes without an instance, operands the vector loads cannot read: the code, and no word written.
    Two NULLs that are refusals only together (rowdot_bwd's dx and dw, weighted_bce_bwd's da and db, axpy_map_bwd's ds and damap)
    follow the list."""
    M, L = _lib()
    for name, entry, kw, code in refusals():
        a = Arena(DEV, guard=64)
        call = _refusal_call(L, a, entry, **kw)
        assert call() == getattr(M, code), name
        v = a.violations()
        assert not v, name + ": " + "; ".join(v)
    for entry, pair in ((ROWDOT_BWD, ("dx", "dw")), (BCE_BWD, ("da", "db")), (MAP_BWD, ("ds", "damap"))):
        a = Arena(DEV, guard=64)
        spec = SPEC[entry]
        held = [a.place_input(torch.zeros(64)) if s[0] == "in" else a.place_output((64,), written=False) if s[0] == "out" else None
                for s in spec]
        args = [None if s[1] in pair else r.ptr if r is not None else s[2] for s, r in zip(spec, held)]
        assert getattr(L, entry)(*args, _stream()) == M.EINVAL, entry + " without either output"
        assert not a.violations()
