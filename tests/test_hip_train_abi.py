"""GPU: the seven entry points of the generator's training path held to their C ABI contract, called directly through ctypes.

    tgsr_conv3x3_wgrad   tgsr_wino_wgrad   tgsr_upwino_wgrad   tgsr_conv_to3_bwd
    tgsr_bn_train_fwd    tgsr_bn_train_fwd_from_stats          tgsr_bn_train_bwd

tests/test_hip_train.py reaches them through tgsr_amd.autograd and the wrappers of tgsr_amd/ops.py only: the routing sends every
Cin % 32 == 0 layer to the Winograd-domain kernels (ten of the direct kernel's twelve instances never ran), every stride is passed
dense, every workspace comes rounded up and recycled from the caching allocator.  Here every operand of a call is placed in a
guarded arena (tests/arena.py): workspaces of exactly *_ws_elems floats prefilled with NaN, outputs prefilled with a pattern no
arithmetic produces, strided operands with NaN between their samples, guard bands around everything.  After the call the guard
bands and gaps must be untouched, every output word written and finite, the result within the project's caps of an fp64 CPU
reference (F.conv2d / F.batch_norm in double under autograd, repeat_interleave for the upBlock) - and a second call with the
workspace holding a finite constant instead of NaN must give the same bits.

TABLE below has one row per (entry point, kernel instance), the dispatch condition copied from the extern "C" launcher; a test
re-evaluates that condition (plan_of / the public planners *_ws_elems, tgsr_conv3x3_wgrad_plan, tgsr_bn_train_nsplit) and asserts the row's instance is the
one its case reaches.  Shapes are the smallest at which the kernel can still go wrong: B = 1, odd H, W no multiple of the tile, Cin
= 20, several tiles per workgroup with a short last one (asserted from the planner: 1 < nslots < units).

Weight gradients additionally carry the project's ratio bound (tests/test_hip_parity_margin.py): the kernel's mean distance from
fp64 against the distance of torch's CPU fp32 gradient from the same fp64, R_DIRECT / R_WINO below.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, MOMENTUM = 1e-5, 0.1

# mean |kernel - f64| / mean |torch CPU fp32 - f64| over a case's weight gradient: 1.5 x the largest measured ratio of the group,
# rounded up to one decimal (the reduction order differs from torch's, so the ratio moves a little with the shape)
R_DIRECT = 1.2          # tgsr_conv3x3_wgrad: measured 0.29 .. 0.79 over the 15 cases on the MI355X (the fp32 MFMA is an fma chain per
                        # workgroup, the slabs summed in a fixed tree: as good as torch's blocked CPU sum at 3 x 19, better as the pixel count grows)
R_WINO = 1.4            # tgsr_wino_wgrad, tgsr_upwino_wgrad: measured 0.22 .. 0.91 over the 13 cases (largest: 64 -> 64 upBlock at 3 x 19)


# ----------------------------------------------------------------------------------------------------------------------------
# The instance table.  Case fields - conv3x3 weight gradients: B, Cin, Cout, H, W (pre-upsample sizes), up; xextra = channels of the
# wider buffer x is a slice of (x_bstride = (Cin + xextra) H W), xpad = further floats on x_bstride; multi = the case whose
# workgroups walk several tiles / chunks with a short last one.  conv_to3: + K, act (1 = TGSR_ACT_TANH_AXPY), dx / dw = outputs asked for.
# BatchNorm: B, C, H, W, act (the `glu` selector), res, run (running statistics given), nbt, oextra / rextra = channels of the wider
# buffers out is written into / the residual is read from.
# ----------------------------------------------------------------------------------------------------------------------------
def _c(B, Cin, Cout, H, W, up=0, xextra=0, xpad=0, multi=False):
    return dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, up=up, xextra=xextra, xpad=xpad, multi=multi)


def _t(B, Cin, H, W, K, act, xextra=0, dx=True, dw=True, addend=True):
    return dict(B=B, Cin=Cin, H=H, W=W, K=K, act=act, xextra=xextra, dx=dx, dw=dw, addend=addend)


def _b(B, C, H, W, act, res=False, run=True, nbt=True, oextra=0, rextra=0):
    return dict(B=B, C=C, H=H, W=W, act=act, res=res, run=run, nbt=nbt, oextra=oextra, rextra=rextra)


DIRECT, WINO, UPWINO, TO3, BNF = ("tgsr_conv3x3_wgrad", "tgsr_wino_wgrad", "tgsr_upwino_wgrad", "tgsr_conv_to3_bwd",
                                  "tgsr_bn_train_fwd / tgsr_bn_train_bwd")
_D = "conv3x3_wgrad_kernel<%s>"          # <NCOB, NCIB, UP>: cb = Cout / 32, ib = ceil(Cin / 32) (wgrad_plan_direct)
_M = "conv_to3_wgrad_mfma_kernel<%s>"    # <K, TANH, NCG = Cin / 16>: W % 16 == 0 and Cin in {16, 32, 48, 64} (wgrad_plan_to3)
_F = "conv_to3_wgrad_kernel<%s>"         # <K, TANH>: otherwise
TABLE = [
    # entry point, kernel instance, dispatch condition, case (None: not covered, the condition names the knob)
    (DIRECT, _D % "4,2,false", "cb % 4 == 0, ib % 2 == 0, upsample = 0", _c(2, 64, 128, 5, 37, xextra=8)),
    (DIRECT, _D % "4,2,false", "... 128 -> 256: 36 workgroups of two tiles over 72", _c(3, 128, 256, 16, 70, xextra=8, multi=True)),
    (DIRECT, _D % "4,2,true", "cb % 4 == 0, ib % 2 == 0, upsample = 1", _c(1, 64, 128, 3, 19, up=1)),
    (DIRECT, _D % "4,1,false", "cb % 4 == 0, ib odd, upsample = 0", _c(1, 32, 128, 5, 37)),
    (DIRECT, _D % "4,1,true", "cb % 4 == 0, ib odd, upsample = 1", _c(2, 32, 128, 3, 19, up=1, xextra=8)),
    (DIRECT, _D % "2,2,false", "cb % 4 == 2, ib % 2 == 0, upsample = 0", _c(2, 64, 64, 5, 37, xextra=8)),
    (DIRECT, _D % "2,2,true", "cb % 4 == 2, ib % 2 == 0, upsample = 1", _c(2, 64, 64, 3, 19, up=1)),
    (DIRECT, _D % "2,1,false", "cb % 4 == 2, ib odd, upsample = 0", _c(2, 32, 64, 5, 37)),
    (DIRECT, _D % "2,1,true", "cb % 4 == 2, ib odd, upsample = 1", _c(1, 32, 64, 3, 19, up=1, xextra=8)),
    (DIRECT, _D % "1,2,false", "cb odd, ib % 2 == 0, upsample = 0", _c(1, 64, 32, 5, 37, xextra=8)),
    (DIRECT, _D % "1,2,true", "cb odd, ib % 2 == 0, upsample = 1", _c(2, 64, 32, 3, 19, up=1)),
    (DIRECT, _D % "1,1,false", "cb odd, ib odd, upsample = 0", _c(2, 32, 32, 5, 37)),
    (DIRECT, _D % "1,1,true", "cb odd, ib odd, upsample = 1", _c(2, 32, 32, 3, 19, up=1, xextra=8)),
    (DIRECT, _D % "1,1,false", "... Cin = 20 (CinPad = 32), Cout = 96 (cb = 3), odd x_bstride", _c(2, 20, 96, 5, 37, xextra=3)),
    (DIRECT, _D % "1,1,true", "... Cin = 20, Cout = 96, upsample = 1", _c(1, 20, 96, 3, 19, up=1)),
    (DIRECT, "every instance at another split", "TGSR_WGRAD_SPLIT_PCT (read once per process): not covered", None),
    # wino_wgrad_kernel<NCI, NCOB>; nci = 2 where Cin % 64 == 0 and the plan did not choose the 64 x 32 tile (wgrad_plan_wino)
    (WINO, "wino_wgrad_kernel<1,1>", "Cin % 64 != 0, Cout % 64 != 0", _c(2, 32, 32, 5, 37, xextra=8)),
    (WINO, "wino_wgrad_kernel<1,1>", "... 68 workgroups of two chunks over 135", _c(3, 32, 32, 9, 138, multi=True)),
    (WINO, "wino_wgrad_kernel<1,2>", "Cin % 64 != 0, Cout % 64 == 0", _c(1, 32, 64, 5, 37)),
    (WINO, "wino_wgrad_kernel<2,1>", "Cin % 64 == 0, Cout % 64 != 0", _c(2, 64, 32, 5, 37, xextra=8)),
    (WINO, "wino_wgrad_kernel<2,2>", "Cin % 64 == 0, Cout % 64 == 0, W % 4 != 0", _c(2, 64, 64, 6, 13)),
    (WINO, "wino_wgrad_kernel<2,2>", "... W % 4 == 0 but x_bstride % 4 != 0 (more than 2048 chunks: else the plan's 64 x 32 tile "
     "makes it <1,2>)", _c(1, 64, 64, 4098, 4, xextra=8, xpad=2)),
    (WINO, "wino_wgrad_kernel<1,2>", "Cin % 64 == 0, Cout % 64 == 0, W % 4 == 0, <= 2048 chunks, x_bstride % 4 != 0: the 64 x 32 "
     "plan without the DMA staging", _c(2, 64, 64, 6, 40, xextra=8, xpad=2)),
    (WINO, "wino_wgrad_dma_kernel<1>", "Cin % 64 == 0, Cout % 64 == 0, W % 4 == 0, 16-byte aligned, x_bstride % 4 == 0, "
     "<= 2048 chunks", _c(3, 64, 64, 10, 144, xextra=8, multi=True)),
    (WINO, "wino_wgrad_dma_kernel<2>", "... more than 2048 chunks (the cheapest: one sample of 2049 tile rows x 1 chunk)",
     _c(1, 64, 64, 4098, 4, xextra=8, multi=True)),
    (WINO, "wino_wgrad_dma_kernel<1> / <2> at the other chunk counts", "TGSR_WGRAD_TILE = 32 | 64: not covered", None),
    (WINO, "wino_wgrad_kernel<2,2> / <1,2> on aligned operands", "TGSR_WGRAD_DMA = 0: not covered", None),
    (WINO, "every instance at another split", "TGSR_WGRAD_SPLIT_PCT: not covered", None),
    # upwino_wgrad_kernel<NCI>
    (UPWINO, "upwino_wgrad_kernel<1>", "Cin % 64 != 0", _c(2, 32, 64, 3, 19, up=1, xextra=8)),
    (UPWINO, "upwino_wgrad_kernel<1>", "... 137 workgroups of two chunks over 273", _c(3, 32, 64, 13, 100, up=1, multi=True)),
    (UPWINO, "upwino_wgrad_kernel<2>", "Cin % 64 == 0", _c(1, 64, 64, 3, 19, up=1)),
    (UPWINO, "upwino_wgrad_kernel<2>", "Cin % 64 == 0, two co groups", _c(2, 64, 128, 5, 37, up=1, xextra=8)),
    (UPWINO, "every instance at another split", "TGSR_WGRAD_SPLIT_PCT: not covered", None),
    # conv_to3: dgrad<K, TANH> whenever dx is asked for; the weight gradient on the matrix cores where wgrad_plan_to3 says mfma
    (TO3, "conv_to3_dgrad_kernel<3,false> + " + _M % "3,false,1", "K = 3, act = 0, Cin = 16, W % 16 == 0", _t(2, 16, 7, 48, 3, 0)),
    (TO3, "conv_to3_dgrad_kernel<3,false> + " + _M % "3,false,2", "... Cin = 32", _t(1, 32, 7, 48, 3, 0, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<3,false> + " + _M % "3,false,3", "... Cin = 48, two column tiles", _t(1, 48, 5, 80, 3, 0)),
    (TO3, "conv_to3_dgrad_kernel<3,false> + " + _M % "3,false,4", "... Cin = 64", _t(2, 64, 7, 48, 3, 0, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<3,true> + " + _M % "3,true,1", "K = 3, act = TANH_AXPY, Cin = 16", _t(1, 16, 7, 48, 3, 1, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<3,true> + " + _M % "3,true,2", "... Cin = 32", _t(2, 32, 7, 48, 3, 1)),
    (TO3, "conv_to3_dgrad_kernel<3,true> + " + _M % "3,true,3", "... Cin = 48", _t(2, 48, 7, 48, 3, 1, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<3,true> + " + _M % "3,true,4", "... Cin = 64, no addend", _t(1, 64, 5, 80, 3, 1, addend=False)),
    (TO3, "conv_to3_dgrad_kernel<5,false> + " + _M % "5,false,1", "K = 5, act = 0, Cin = 16", _t(1, 16, 5, 80, 5, 0, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<5,false> + " + _M % "5,false,2", "... Cin = 32", _t(2, 32, 7, 48, 5, 0)),
    (TO3, "conv_to3_dgrad_kernel<5,false> + " + _M % "5,false,3", "... Cin = 48", _t(2, 48, 7, 48, 5, 0, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<5,false> + " + _M % "5,false,4", "... Cin = 64", _t(1, 64, 7, 48, 5, 0)),
    (TO3, "conv_to3_dgrad_kernel<5,true> + " + _M % "5,true,1", "K = 5, act = TANH_AXPY, Cin = 16", _t(2, 16, 7, 48, 5, 1)),
    (TO3, "conv_to3_dgrad_kernel<5,true> + " + _M % "5,true,2", "... Cin = 32", _t(1, 32, 5, 80, 5, 1, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<5,true> + " + _M % "5,true,3", "... Cin = 48", _t(1, 48, 7, 48, 5, 1)),
    (TO3, "conv_to3_dgrad_kernel<5,true> + " + _M % "5,true,4", "... Cin = 64", _t(2, 64, 7, 48, 5, 1, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<3,false> + " + _F % "3,false", "K = 3, act = 0, Cin = 20", _t(2, 20, 5, 37, 3, 0, xextra=3)),
    (TO3, "conv_to3_dgrad_kernel<3,true> + " + _F % "3,true", "K = 3, TANH_AXPY, W % 16 != 0", _t(1, 32, 5, 37, 3, 1)),
    (TO3, "conv_to3_dgrad_kernel<5,false> + " + _F % "5,false", "K = 5, act = 0, W % 16 != 0, 2 x 2 tiles",
     _t(2, 32, 19, 70, 5, 0, xextra=8)),
    (TO3, "conv_to3_dgrad_kernel<5,true> + " + _F % "5,true", "K = 5, TANH_AXPY, Cin = 20", _t(2, 20, 5, 37, 5, 1)),
    (TO3, "conv_to3_dgrad_kernel<5,true>", "dw == NULL, ws == NULL", _t(2, 32, 7, 48, 5, 1, dw=False)),
    (TO3, "conv_to3_dgrad_kernel<3,false>", "dw == NULL, ws == NULL (ragged W)", _t(1, 20, 5, 37, 3, 0, dw=False)),
    (TO3, _M % "5,true,2", "dx == NULL", _t(2, 32, 7, 48, 5, 1, dx=False, xextra=8)),
    (TO3, _F % "3,false", "dx == NULL", _t(1, 20, 5, 37, 3, 0, dx=False)),
    (TO3, "the MFMA kernel's taller wave tiles (rpw 2, 4, 8)", ">= 1024 workgroups: tests/test_hip_train.py's large cases", None),
    # BatchNorm: forward and backward of one case run in one test
    (BNF, "bn_fin_act_fwd_kernel<false,FUSED> / bn_fin_act_bwd_apply_kernel<false,FUSED>", "nsplit == 1, act = 0",
     _b(1, 8, 6, 6, 0, oextra=4)),
    (BNF, "... the same", "nsplit == 1, act = 0 + residual (read from a channel slice)", _b(2, 6, 5, 8, 0, res=True, run=False,
                                                                                           nbt=False, rextra=2)),
    (BNF, "... the same", "nsplit == 1, act = 2", _b(3, 5, 7, 4, 2, nbt=False)),
    (BNF, "bn_stats_kernel + bn_fin_act_fwd_kernel<true> / bn_act_bwd_reduce_kernel<true> + bn_fin_act_bwd_apply_kernel<true>",
     "act = 1 (GLU), nsplit == 1, out written into a channel slice", _b(2, 8, 5, 4, 1, oextra=4)),
    (BNF, "... the same", "act = 1, B HW >= 8192: nsplit == 2", _b(2, 8, 64, 64, 1, run=False, oextra=4)),
    (BNF, "bn_stats_kernel + bn_fin_act_fwd_kernel<false> / bn_act_bwd_reduce_kernel<false> + bn_fin_act_bwd_apply_kernel<false>",
     "act = 0, B HW >= 8192: nsplit == 2", _b(2, 8, 64, 64, 0, nbt=False, oextra=4)),
    (BNF, "... the same", "act = 0 + residual, nsplit == 2", _b(2, 8, 64, 64, 0, res=True, run=False, rextra=4, oextra=8)),
    (BNF, "... the same", "act = 2, nsplit == 2, slices across a sample boundary", _b(3, 6, 50, 56, 2)),
    (BNF, "the two-pass form on small layers", "TGSR_BN_FUSE_SMALL = 0 (the same instances as above): not covered", None),
]
FROM_STATS = [   # tgsr_bn_train_fwd_from_stats: (nslots, case); 96 takes the nsplit > 64 branch of bn_channel_affine
    (1, _b(2, 6, 10, 12, 0, res=True, rextra=2, nbt=False)),
    (3, _b(2, 6, 10, 12, 1, oextra=3, run=False)),
    (96, _b(2, 6, 10, 12, 2)),
]


def _rows(*entries):
    return [r for r in TABLE if r[0] in entries and r[3] is not None]


def row_id(r):
    c = r[3]
    if r[0] == TO3:
        tag = "K%d-act%d-%dto3-B%d-%dx%d%s%s%s" % (c["K"], c["act"], c["Cin"], c["B"], c["H"], c["W"], "-slice" if c["xextra"] else "",
                                                 "" if c["dx"] else "-nodx", "" if c["dw"] else "-nodw")
    elif r[0] == BNF:
        tag = "act%d%s-B%d-C%d-%dx%d%s%s" % (c["act"], "res" if c["res"] else "", c["B"], c["C"], c["H"], c["W"],
                                            "" if c["run"] else "-norun", "" if c["nbt"] else "-nonbt")
    else:
        inst = r[1].replace("_kernel", "").replace("<", "").replace(">", "").replace(",", "_")
        tag = "%s-%dto%d-B%d-%dx%d%s%s" % (inst, c["Cin"], c["Cout"], c["B"], c["H"], c["W"], "-slice" if c["xextra"] else "",
                                          "-pad%d" % c["xpad"] if c["xpad"] else "")
    return r[0][5:].split(" ")[0] + "-" + tag


# ----------------------------------------------------------------------------------------------------------------------------
# The launchers' dispatch conditions, restated (the planners' arithmetic with the default split; `units` = tiles / chunks)
# ----------------------------------------------------------------------------------------------------------------------------
def _split(units, want):
    want = max(1, min(want, units))
    per = -(-units // want)
    return per, -(-units // per)


def plan_of(entry, c, g_addr=0, x_addr=0, xbs=0):
    B, Cin, Cout, H, W = c["B"], c["Cin"], c["Cout"], c["H"], c["W"]
    if entry == DIRECT:
        Ho, Wo = (2 * H, 2 * W) if c["up"] else (H, W)
        cb, ib = (Cout + 31) // 32, (Cin + 31) // 32
        ncob, ncib = (4 if cb % 4 == 0 else 2 if cb % 2 == 0 else 1), (2 if ib % 2 == 0 else 1)
        groups = (cb // ncob) * (ib // ncib)
        units = B * ((Ho + 1) // 2) * ((Wo + 31) // 32)
        per, nslots = _split(units, 2048 // (ncob * ncib) // groups)
        inst = "conv3x3_wgrad_kernel<%d,%d,%s>" % (ncob, ncib, "true" if c["up"] else "false")
        return dict(instance=inst, slab=9 * Cout * ib * 32, units=units, per=per, nslots=nslots)
    if entry == WINO:
        units = B * ((H + 1) // 2) * (((W + 1) // 2 + 7) // 8)
        use32 = Cin % 64 == 0 and Cout % 64 == 0 and W % 4 == 0 and units <= 2048
        nci = 2 if Cin % 64 == 0 and not use32 else 1
        co64 = Cout % 64 == 0
        groups = (Cout // (64 if co64 else 32)) * (Cin // (32 * nci))
        want = (512 if use32 else 256) // groups
        if units <= 512 and want >= 64:
            want //= 2
        per, nslots = _split(units, want)
        dma_ok = W % 4 == 0 and (g_addr | x_addr) % 16 == 0 and xbs % 4 == 0
        if nci == 2 and co64 and dma_ok:
            inst = "wino_wgrad_dma_kernel<2>"
        elif nci == 1 and co64 and dma_ok and Cin % 64 == 0:
            inst = "wino_wgrad_dma_kernel<1>"
        else:
            inst = "wino_wgrad_kernel<%d,%d>" % (nci, 2 if co64 else 1)
        return dict(instance=inst, slab=16 * Cout * Cin, units=units, per=per, nslots=nslots)
    assert entry == UPWINO
    nci = 2 if Cin % 64 == 0 else 1
    groups = (Cout // 64) * (Cin // (32 * nci))
    units = B * H * ((W + 15) // 16)
    want = 512 // groups
    if units <= 1024 and want >= 64:
        want //= 2
    per, nslots = _split(units, want)
    return dict(instance="upwino_wgrad_kernel<%d>" % nci, slab=9 * Cout * Cin, units=units, per=per, nslots=nslots)


def ws_elems(L, entry, c):
    if entry == DIRECT:
        return L.tgsr_conv3x3_wgrad_ws_elems(c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["up"])
    fn = L.tgsr_wino_wgrad_ws_elems if entry == WINO else L.tgsr_upwino_wgrad_ws_elems
    return fn(c["B"], c["Cin"], c["Cout"], c["H"], c["W"])


def to3_plan(c):
    """(instances, slabs) of a conv_to3_bwd case; the MFMA tile is 4 rows (rpw = 1) below 1024 workgroups."""
    B, Cin, H, W, K = c["B"], c["Cin"], c["H"], c["W"], c["K"]
    kt = "%d,%s" % (K, "true" if c["act"] else "false")
    tx = (W + 63) // 64
    inst, slabs = [], B * tx * ((H + 15) // 16)
    if c["dx"]:
        inst.append("conv_to3_dgrad_kernel<%s>" % kt)
    mfma = W % 16 == 0 and Cin in (16, 32, 48, 64)
    if mfma:
        rpw = next((r for r in (8, 4, 2) if B * tx * ((H + 4 * r - 1) // (4 * r)) >= 1024), 1)
        assert rpw == 1, "the taller wave tiles are tests/test_hip_train.py's"
        slabs = B * tx * ((H + 3) // 4)
    if c["dw"]:
        inst.append(("conv_to3_wgrad_mfma_kernel<%s,%d>" % (kt, Cin // 16)) if mfma else "conv_to3_wgrad_kernel<%s>" % kt)
    return " + ".join(inst), slabs


# The same two answers from the library: tgsr_conv3x3_wgrad_plan / tgsr_conv_to3_bwd_plan are the functions the launchers plan with
WGRAD_KIND = {DIRECT: 0, WINO: 1, UPWINO: 2}          # TGSR_WGRAD_DIRECT, _WINO, _UPWINO


def exported_plan(entry, c, g_addr=0, x_addr=0, xbs=0):
    """plan_of's fields as tgsr_conv3x3_wgrad_plan states them for operands at these addresses"""
    M, L = _lib()
    out = (ctypes.c_int64 * M.WGRAD_PLAN_FIELDS)()
    rc = L.tgsr_conv3x3_wgrad_plan(WGRAD_KIND[entry], ctypes.c_void_p(g_addr), ctypes.c_void_p(x_addr), xbs, c["B"], c["Cin"],
                                   c["H"], c["W"], c["Cout"], c["up"], out)
    assert rc == M.OK, rc
    fam, t0, t1, t2, units, per, nslots, _groups, slab, ws = out
    fmt = M.WGRAD_FAMILIES[fam]
    inst = fmt % ((t0, t1, "true" if t2 else "false") if "%s" in fmt else (t0, t1)[:fmt.count("%d")])
    assert ws == nslots * slab
    return dict(instance=inst, slab=slab, units=units, per=per, nslots=nslots)


def exported_to3_plan(c):
    """to3_plan's answers as tgsr_conv_to3_bwd_plan states them (rows per wave: 1 at every case of the table)"""
    M, L = _lib()
    out = (ctypes.c_int64 * M.TO3_BWD_PLAN_FIELDS)()
    assert L.tgsr_conv_to3_bwd_plan(c["B"], c["Cin"], c["H"], c["W"], c["K"], out) == M.OK
    mfma, rpw, slabs, ws = out
    assert ws == slabs * 3 * c["Cin"] * c["K"] ** 2 and rpw == 1
    kt = "%d,%s" % (c["K"], "true" if c["act"] else "false")
    inst = ["conv_to3_dgrad_kernel<%s>" % kt] if c["dx"] else []
    if c["dw"]:
        inst.append(("conv_to3_wgrad_mfma_kernel<%s,%d>" % (kt, c["Cin"] // 16)) if mfma else "conv_to3_wgrad_kernel<%s>" % kt)
    return " + ".join(inst), slabs


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs and references (CPU; computed once per shape and shared)
# ----------------------------------------------------------------------------------------------------------------------------
def _wkey(c):
    return (c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["up"])


@functools.lru_cache(maxsize=None)
def wgrad_inputs(key):
    B, Cin, Cout, H, W, up = key
    g = torch.Generator().manual_seed(B + 3 * Cin + 5 * Cout + 7 * H + 11 * W + up)
    s = 2 if up else 1
    return torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cout, s * H, s * W, generator=g)


def wgrad_reference(x, dy, up, dtype):
    """dw of conv3x3(up ? nearest_x2(x) : x) by torch autograd on the CPU in `dtype`."""
    x = x.to(dtype)
    xi = x.repeat_interleave(2, 2).repeat_interleave(2, 3) if up else x
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=dtype, requires_grad=True)
    F.conv2d(xi, w, None, 1, 1).backward(dy.to(dtype))
    return w.grad


@functools.lru_cache(maxsize=None)
def wgrad_refs(key):
    x, dy = wgrad_inputs(key)
    return wgrad_reference(x, dy, key[5], torch.float64), wgrad_reference(x, dy, key[5], torch.float32)


def wgrad_tol(dy):
    """The caps of test_conv_bn_act_train_fwd_bwd: (atol, rtol)."""
    return 2e-5 * float(dy.numel()) ** 0.5, 2e-3


def _tkey(c):
    return (c["B"], c["Cin"], c["H"], c["W"], c["K"], c["act"], c["addend"])


ALPHA = 0.5


@functools.lru_cache(maxsize=None)
def to3_inputs(key):
    B, Cin, H, W, K, act, addend = key
    g = torch.Generator().manual_seed(K * 10 + H + 3 * Cin + W + act)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(3, Cin, K, K, generator=g) / (K * Cin ** 0.5)
    add = torch.randn(B, 3, H, W, generator=g) if act and addend else None
    dy = torch.randn(B, 3, H, W, generator=g)
    return x, w, add, dy


def to3_reference(x, w, add, dy, act, dtype=torch.float64):
    """(out, dx, dw) of conv_to3 [+ tanh + ALPHA addend] by torch autograd on the CPU."""
    xr, wr = x.to(dtype).requires_grad_(), w.to(dtype).requires_grad_()
    y = F.conv2d(xr, wr, None, 1, w.shape[2] // 2)
    if act:
        y = torch.tanh(y)
        y = y + ALPHA * add.to(dtype) if add is not None else y
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, wr.grad


@functools.lru_cache(maxsize=None)
def to3_refs(key):
    x, w, add, dy = to3_inputs(key)
    return to3_reference(x, w, add, dy, key[5])


def to3_tol(c):
    """The caps of test_conv_to3_backward on dw: (atol, rtol)."""
    return 3e-5 * float(c["B"] * c["H"] * c["W"]) ** 0.5, 2e-3


def _bkey(c):
    return (c["B"], c["C"], c["H"], c["W"], c["act"], c["res"])


@functools.lru_cache(maxsize=None)
def bn_inputs(key):
    B, C, H, W, act, res = key
    g = torch.Generator().manual_seed(B + 3 * C + 5 * H + 7 * W + act)
    co = C // 2 if act == 1 else C
    raw = torch.randn(B, C, H, W, generator=g) * (0.5 + torch.rand(1, C, 1, 1, generator=g)) + 0.5 * torch.randn(1, C, 1, 1, generator=g)
    return dict(raw=raw, gamma=1 + 0.2 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
                rm=0.1 * torch.randn(C, generator=g), rv=0.5 + torch.rand(C, generator=g),
                res=torch.randn(B, co, H, W, generator=g) if res else None, dout=torch.randn(B, co, H, W, generator=g))


def bn_reference(i, act, dout=None, dtype=torch.float64):
    """Everything tgsr_bn_train_fwd / _bwd return, by F.batch_norm(training) under torch autograd on the CPU."""
    raw, gamma, beta = (i[k].to(dtype).requires_grad_() for k in ("raw", "gamma", "beta"))
    rm, rv = i["rm"].to(dtype).clone(), i["rv"].to(dtype).clone()
    y = F.batch_norm(raw, rm, rv, gamma, beta, True, MOMENTUM, EPS)
    if act == 1:
        y = F.glu(y, 1)
    elif act == 2:
        y = F.leaky_relu(y, 0.2)
    if i["res"] is not None:
        y = y + i["res"].to(dtype)
    y.backward((i["dout"] if dout is None else dout).to(dtype))
    r = raw.detach()
    mean, var = r.mean((0, 2, 3)), r.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.detach() * invstd
    return dict(out=y.detach(), mean=mean, invstd=invstd, scale=scale, shift=beta.detach() - mean * scale, rm=rm, rv=rv,
                draw=raw.grad, dgamma=gamma.grad, dbeta=beta.grad)


@functools.lru_cache(maxsize=None)
def bn_refs(key):
    return bn_reference(bn_inputs(key), key[4])


def bn_affine_tol(dout):
    """The caps of test_conv_bn_act_train_fwd_bwd on dgamma / dbeta: (atol, rtol)."""
    return 2e-5 * float(dout.numel()) ** 0.5, 2e-3


# Outputs 5e-5, running statistics 1e-5 (the caps of test_conv_bn_act_train_fwd_bwd, rtol 1e-4 as its close()); draw is an
# elementwise expression of the same form as `out` and takes the same cap.  mean / invstd / scale / shift: O(1) values from fp32
# partial sums of at most 8 values per thread combined in double - a few ulp (6e-8 relative); 1e-6 + 1e-5 |ref| leaves room for
# the cancellation in E[x^2] - mean^2 at |mean| <= 2 sigma and nothing more.
OUT_ATOL, RUN_ATOL, STAT_ATOL, STAT_RTOL = 5e-5, 1e-5, 1e-6, 1e-5


def close(got, ref, atol, rtol=1e-4, what=""):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d of %d values beyond atol %.3g rtol %.3g, worst |err| %.3g at |ref| %.3g" % (
        what, int(bad.sum()), bad.numel(), atol, rtol, float(err.max()), float(ref.abs().flatten()[int(err.argmax())]))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    from tgsr_amd import ops
    return ops._stream()


# ----------------------------------------------------------------------------------------------------------------------------
# 1-3: the three conv3x3 weight gradients
# ----------------------------------------------------------------------------------------------------------------------------
def _place_wgrad(a, entry, c, g_skew=0):
    x, dy = wgrad_inputs(_wkey(c))
    xbs = (c["Cin"] + c["xextra"]) * c["H"] * c["W"] + c["xpad"]
    return a.place_input(dy, skew=g_skew), a.place_input(x, bstride=xbs), xbs


def _call_wgrad(L, entry, c, gr, xr, xbs, ws, dw):
    if entry == DIRECT:
        return L.tgsr_conv3x3_wgrad(gr.ptr, xr.ptr, xbs, c["B"], c["Cin"], c["H"], c["W"], c["Cout"], c["up"], ws.ptr, dw.ptr, _stream())
    fn = L.tgsr_wino_wgrad if entry == WINO else L.tgsr_upwino_wgrad
    return fn(gr.ptr, xr.ptr, xbs, c["B"], c["Cin"], c["H"], c["W"], c["Cout"], ws.ptr, dw.ptr, _stream())


@pytest.mark.parametrize("row", _rows(DIRECT, WINO, UPWINO), ids=row_id)
def test_weight_gradient_entry_points(row):
    entry, instance, _cond, c = row
    M, L = _lib()
    x, dy = wgrad_inputs(_wkey(c))
    a = Arena(DEV)
    gr, xr, xbs = _place_wgrad(a, entry, c)
    n = ws_elems(L, entry, c)
    ws, dw = a.place_ws(n), a.place_output((c["Cout"], c["Cin"], 3, 3))
    plan = plan_of(entry, c, gr.address, xr.address, xbs)
    assert plan["instance"] == instance, "the case reaches %s" % plan["instance"]
    assert n == plan["nslots"] * plan["slab"], "the planner's split is not the restated one"
    if c["multi"]:        # several tiles / chunks per workgroup ...
        assert 1 < n // plan["slab"] < plan["units"], plan
        assert entry == DIRECT or plan["units"] % plan["per"] != 0, plan      # ... and the last workgroup short
    assert xbs > c["Cin"] * c["H"] * c["W"] or not (c["xextra"] or c["xpad"])
    assert _call_wgrad(L, entry, c, gr, xr, xbs, ws, dw) == M.OK
    a.check()
    got = dw.read()
    a.rearm(ws_fill=0.75)
    assert _call_wgrad(L, entry, c, gr, xr, xbs, ws, dw) == M.OK
    a.check()
    assert same_bits(got, dw.read()), "the result depends on what the workspace held"
    ref64, ref32 = wgrad_refs(_wkey(c))
    own = float((got.double() - ref64).abs().mean())
    cpu = float((ref32.double() - ref64).abs().mean())
    print("WGRAD_RATIO %s %s own %.4g cpu %.4g ratio %.3f max|err| %.4g" % (
        entry, row_id(row), own, cpu, own / cpu, float((got.double() - ref64).abs().max())))
    atol, rtol = wgrad_tol(dy)
    close(got, ref64, atol, rtol, "dw")
    R = R_DIRECT if entry == DIRECT else R_WINO
    assert own <= R * cpu, "mean |kernel - f64| = %.3g is %.2f x the CPU fp32 gradient's %.3g (bound %.1f)" % (own, own / cpu, cpu, R)


def test_upwino_wgrad_refuses_a_grad_out_that_is_not_8_byte_aligned():
    M, L = _lib()
    c = _c(2, 32, 64, 3, 19, up=1)
    a = Arena(DEV)
    gr, xr, xbs = _place_wgrad(a, UPWINO, c, g_skew=1)
    ws = a.place_output((ws_elems(L, UPWINO, c),), written=False)
    dw = a.place_output((c["Cout"], c["Cin"], 3, 3), written=False)
    assert gr.address % 8 == 4
    assert _call_wgrad(L, UPWINO, c, gr, xr, xbs, ws, dw) == M.EUNSUPPORTED
    a.check()          # neither the workspace nor dw was touched


def test_ops_raise_on_a_shape_the_launchers_refuse():
    """An empty batch on each of the three routes, and a 4x4 image head: TgsrError from check(), the process lives."""
    from tgsr_amd import ops
    M, _L = _lib()
    for Cin, Cout, up in ((20, 32, False), (32, 32, False), (32, 64, True)):
        s = 2 if up else 1
        with pytest.raises(M.TgsrError):
            ops.conv3x3_wgrad(torch.empty(0, Cout, 8 * s, 8 * s, device=DEV), torch.empty(0, Cin, 8, 8, device=DEV), up)
    x, w, dy = torch.randn(2, 32, 8, 8, device=DEV), torch.randn(3, 32, 4, 4, device=DEV), torch.randn(2, 3, 8, 8, device=DEV)
    with pytest.raises(M.TgsrError):
        ops.conv_to3_bwd(dy, None, None, 0.0, x, w, False)


# ----------------------------------------------------------------------------------------------------------------------------
# 4: the image heads' backward
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", _rows(TO3), ids=row_id)
def test_conv_to3_bwd_entry_point(row):
    _entry, instance, _cond, c = row
    M, L = _lib()
    B, Cin, H, W, K, act = (c[k] for k in ("B", "Cin", "H", "W", "K", "act"))
    x, w, add, dy = to3_inputs(_tkey(c))
    out64, dx64, dw64 = to3_refs(_tkey(c))
    inst, slabs = to3_plan(c)
    assert inst == instance, "the case reaches %s" % inst
    n = L.tgsr_conv_to3_bwd_ws_elems(B, Cin, H, W, K)
    assert n == slabs * 3 * Cin * K * K
    a = Arena(DEV)
    xbs = (Cin + c["xextra"]) * H * W
    dyr, xr, wr = a.place_input(dy), a.place_input(x, bstride=xbs), a.place_input(w)
    outr = a.place_input(out64.float()) if act else None       # the forward output, as the forward stores it
    addr = a.place_input(add) if add is not None else None
    dx = a.place_output((B, Cin, H, W), written=c["dx"])
    ws = a.place_ws(n) if c["dw"] else a.place_output((n,), written=False)
    dw = a.place_output((3, Cin, K, K), written=c["dw"])

    def call():
        return L.tgsr_conv_to3_bwd(dyr.ptr, outr.ptr if outr else None, addr.ptr if addr else None, ALPHA, xr.ptr, xbs, wr.ptr,
                                   B, Cin, H, W, K, M.ACT_TANH_AXPY if act else M.ACT_NONE, dx.ptr if c["dx"] else None,
                                   ws.ptr if c["dw"] else None, dw.ptr if c["dw"] else None, _stream())
    assert call() == M.OK
    a.check()                                                  # an absent output's region is untouched
    got_dx, got_dw = dx.read(), dw.read()
    a.rearm(ws_fill=0.75)
    assert call() == M.OK
    a.check()
    if c["dx"]:
        assert same_bits(got_dx, dx.read())
        close(got_dx, dx64, 2e-5, 1e-3, "dx")
    if c["dw"]:
        assert same_bits(got_dw, dw.read()), "the result depends on what the workspace held"
        atol, rtol = to3_tol(c)
        close(got_dw, dw64, atol, rtol, "dw")


# ----------------------------------------------------------------------------------------------------------------------------
# 5-6: BatchNorm in training mode
# ----------------------------------------------------------------------------------------------------------------------------
def _bn_forward(M, L, c, stat_partial=None):
    """One forward call in an arena of its own; returns the outputs read back (two calls: NaN and constant workspace)."""
    B, C, H, W, act = (c[k] for k in ("B", "C", "H", "W", "act"))
    HW, co = H * W, (C // 2 if act == 1 else C)
    i = bn_inputs(_bkey(c))
    a = Arena(DEV)
    raw, gamma, beta = a.place_input(i["raw"]), a.place_input(i["gamma"]), a.place_input(i["beta"])
    rm = a.place_inout(i["rm"]) if c["run"] else None
    rv = a.place_inout(i["rv"]) if c["run"] else None
    nbt = a.place_inout(torch.tensor([41], dtype=torch.int64)) if c["nbt"] else None
    rbs, obs = (co + c["rextra"]) * HW, (co + c["oextra"]) * HW
    res = a.place_input(i["res"], bstride=rbs) if c["res"] else None
    nsplit = L.tgsr_bn_train_nsplit(B, C, HW)
    if stat_partial is None:
        ws = a.place_ws(C * nsplit * 4)
    else:
        ws = a.place_input(stat_partial)
    st = [a.place_output((C,)) for _ in range(4)]               # mean, invstd, scale, shift
    out = a.place_output((B, co, H, W), bstride=obs)
    assert obs % 4 == 0 and rbs % 4 == 0
    _p = lambda r: r.ptr if r is not None else None             # noqa: E731

    def call():
        if stat_partial is None:
            return L.tgsr_bn_train_fwd(raw.ptr, B, C, HW, gamma.ptr, beta.ptr, EPS, MOMENTUM, _p(rm), _p(rv), act, _p(res),
                                       rbs if c["res"] else 0, ws.ptr, st[0].ptr, st[1].ptr, st[2].ptr, st[3].ptr, out.ptr, obs,
                                       _p(nbt), _stream())
        return L.tgsr_bn_train_fwd_from_stats(raw.ptr, B, C, HW, gamma.ptr, beta.ptr, EPS, MOMENTUM, _p(rm), _p(rv), act, _p(res),
                                              rbs if c["res"] else 0, ws.ptr, stat_partial.shape[1], st[0].ptr, st[1].ptr,
                                              st[2].ptr, st[3].ptr, out.ptr, obs, _p(nbt), _stream())

    def read():
        g = dict(out=out.read(), mean=st[0].read(), invstd=st[1].read(), scale=st[2].read(), shift=st[3].read())
        if c["run"]:
            g["rm"], g["rv"] = rm.read(), rv.read()
        if c["nbt"]:
            g["nbt"] = int(nbt.read())
        return g
    assert call() == M.OK
    a.check()
    got = read()
    a.rearm(ws_fill=None if stat_partial is not None else 0.75)
    assert call() == M.OK
    a.check()
    again = read()
    for k, v in got.items():
        assert v == again[k] if k == "nbt" else same_bits(v, again[k]), "%s depends on what the workspace held" % k
    if c["nbt"]:
        assert got["nbt"] == 42
    return got, nsplit


def _check_bn_forward(got, ref, c):
    close(got["out"], ref["out"], OUT_ATOL, what="out")
    for k in ("mean", "invstd", "scale", "shift"):
        close(got[k], ref[k], STAT_ATOL, STAT_RTOL, k)
    if c["run"]:
        close(got["rm"], ref["rm"], RUN_ATOL, what="running_mean")
        close(got["rv"], ref["rv"], RUN_ATOL, what="running_var")


@pytest.mark.parametrize("row", _rows(BNF), ids=row_id)
def test_bn_train_fwd_and_bwd_entry_points(row):
    _entry, _instance, cond, c = row
    M, L = _lib()
    B, C, H, W, act = (c[k] for k in ("B", "C", "H", "W", "act"))
    HW, co = H * W, (C // 2 if act == 1 else C)
    i, ref = bn_inputs(_bkey(c)), bn_refs(_bkey(c))
    got, nsplit = _bn_forward(M, L, c)
    assert ("nsplit == 1" in cond) == (nsplit == 1) and ("nsplit == 2" in cond) == (nsplit == 2), nsplit
    assert (nsplit == 1) == (B * HW < 8192)                     # the one-launch form where act != 1, the two-pass form otherwise
    _check_bn_forward(got, ref, c)
    # backward on the statistics the forward saved
    a = Arena(DEV)
    dout, raw = a.place_input(i["dout"]), a.place_input(i["raw"])
    st = {k: a.place_input(got[k]) for k in ("scale", "shift", "mean", "invstd")}
    ws = a.place_ws(C * nsplit * 4)
    assert co * L.tgsr_bn_train_nsplit(B, co, HW) <= C * nsplit     # the backward's slabs fit the workspace the header asks for
    draw, dgamma, dbeta = a.place_output((B, C, H, W)), a.place_output((C,)), a.place_output((C,))

    def call():
        return L.tgsr_bn_train_bwd(dout.ptr, raw.ptr, B, C, HW, st["scale"].ptr, st["shift"].ptr, st["mean"].ptr, st["invstd"].ptr,
                                   act, ws.ptr, ws.ptr, draw.ptr, dgamma.ptr, dbeta.ptr, _stream())
    assert call() == M.OK
    a.check()
    g = [draw.read(), dgamma.read(), dbeta.read()]
    a.rearm(ws_fill=0.75)
    assert call() == M.OK
    a.check()
    for u, v in zip(g, (draw.read(), dgamma.read(), dbeta.read())):
        assert same_bits(u, v), "the backward depends on what the workspace held"
    close(g[0], ref["draw"], OUT_ATOL, what="draw")
    atol, rtol = bn_affine_tol(i["dout"])
    close(g[1], ref["dgamma"], atol, rtol, "dgamma")
    close(g[2], ref["dbeta"], atol, rtol, "dbeta")


def stat_partial_of(raw, nslots):
    """[C][nslots][2] (sum, sum of squares) pairs of nslots contiguous pieces of every channel's B x HW values: fp64, rounded to fp32."""
    B, C = raw.shape[:2]
    flat = raw.double().permute(1, 0, 2, 3).reshape(C, -1).numpy()
    out = np.zeros((C, nslots, 2))
    for s, piece in enumerate(np.array_split(np.arange(flat.shape[1]), nslots)):
        out[:, s, 0] = flat[:, piece].sum(1)
        out[:, s, 1] = (flat[:, piece] ** 2).sum(1)
    return torch.from_numpy(out.astype(np.float32))


@pytest.mark.parametrize("nslots,c", FROM_STATS, ids=lambda v: str(v) if isinstance(v, int) else "act%d" % v["act"])
def test_bn_train_fwd_from_stats_entry_point(nslots, c):
    M, L = _lib()
    i, ref = bn_inputs(_bkey(c)), bn_refs(_bkey(c))
    sp = stat_partial_of(i["raw"], nslots)
    assert tuple(sp.shape) == (c["C"], nslots, 2)
    got, _ = _bn_forward(M, L, c, stat_partial=sp)
    _check_bn_forward(got, ref, c)
    own, _ = _bn_forward(M, L, c)                                # tgsr_bn_train_fwd on the same raw
    close(got["out"], own["out"], OUT_ATOL, what="out against tgsr_bn_train_fwd")
    for k in ("mean", "invstd", "scale", "shift"):
        close(got[k], own[k], STAT_ATOL, STAT_RTOL, k + " against tgsr_bn_train_fwd")
    if c["run"]:
        close(got["rm"], own["rm"], RUN_ATOL, what="running_mean against tgsr_bn_train_fwd")
        close(got["rv"], own["rv"], RUN_ATOL, what="running_var against tgsr_bn_train_fwd")
