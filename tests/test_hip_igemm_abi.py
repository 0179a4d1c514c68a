"""GPU: the implicit-GEMM family (csrc/tgsr_down.hip, csrc/tgsr_igemm.hip) held to its C ABI contract, called directly through ctypes.

    tgsr_conv4x4s2_{fwd, dgrad, wgrad}      tgsr_conv3x3_gemm_{fwd, dgrad, wgrad}      (the discriminators)
    tgsr_gconv(dgrad = 0 | 1)   tgsr_gconv_stats   tgsr_gconv_pack   tgsr_bn_train_relu_slice_from_stats      (the Inception trunk)
    and the trunk's strided companions: the pools, tgsr_relu_mask, tgsr_interleave2x2, tgsr_sum_stack, tgsr_plane_mean(_bwd),
    tgsr_bilinear_{fwd, bwd}, tgsr_leaky_relu

tests/test_hip_gan.py and tests/test_hip_inception*.py reach these kernels through tgsr_amd.ops / custom_ops / autograd only: dense
512-byte aligned operands from the caching allocator, workspaces rounded up and recycled with finite contents, the channels beside a
slice prefilled with a finite value.  Here every operand of a call lives in a guarded arena (tests/arena.py): S a channel slice of a
wider buffer with an odd pad on its batch stride, out a slice of a wider buffer, the mask laid out like out with the NaN pattern in
its gaps, the workspace exactly *_ws_elems floats (NULL where tgsr_gconv's plan has one slab), stat_partial exactly M x nslots x 2,
the packed weights produced by tgsr_gconv_pack into exactly their element count.  After the call the guard bands, gaps and inputs
hold their bits, every output word is written and finite, a second call - the workspace now holding a finite constant - gives the
same bits, and the values hold against the same operation in fp64 on the CPU.

DTABLE / GTABLE have one row per (entry point, kernel instance, launch path) with the dispatch condition copied from the launcher
(ig_plan / gc_plan); a test asserts from the exported planners that the row's case reaches the instance the row names.  Every GEMM
instance appears with one slab and with a K split whose last slab is shorter than the others.

Alignment (include/tgsr_hip.h states it per operand): the three-piece form loads A - w, the workspace's head, dy of a weight
gradient - 16 bytes at a time and its launchers fall back to the fp32 MFMA, all dword accesses, for an A that is not 16-byte aligned;
every other operand is read and written by dwords.  The rows named "skew" move an operand one word off and take that fallback;
their bits equal the aligned call's with the three-piece form switched off.

Besides the caps every convolution carries the ratio bound of tests/test_hip_parity_margin.py: its mean distance from fp64 against
the distance of torch's CPU fp32 evaluation of the same operation from the same fp64 (R below).
"""
import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from arena import GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, U = -1, -2         # TGSR_EINVAL, TGSR_EUNSUPPORTED

# mean |kernel - f64| / mean |torch CPU fp32 of the same operation - f64| over a case's output, per group: 1.5 x the largest ratio
# measured on the MI355X, rounded up to one decimal (the reduction order differs from torch's, so the ratio moves with the shape).
# Measured ranges (D = the discriminators' rows, G = the trunk's; the largest ratios are the weight gradients', whose K runs over
# pixels: 1.26 .. 1.45 on one slab).  Where a row exists in both forms at the same shape (13 discriminator pairs, 3 trunk pairs)
# the three-piece form's ratio is below the fp32 MFMA's in every pair, 0.53 .. 1.11 against 0.64 .. 1.31 (include/tgsr_hip.h:
# "measured error against fp64: below the fp32 MFMA's").  The image kernels have no K split, so that group does not exist.
R = {
    "fp32": 2.2,              # 27 cases: D 0.94 .. 1.44 (16), G 0.97 .. 1.06 (11)
    "fp32+ksplit": 2.0,       # 18 cases: D 0.67 .. 1.28 (12), G 0.56 .. 1.18 (6)
    "split": 2.2,             # 21 cases: D 0.80 .. 1.45 (14; 1.45 = the 3x3 weight gradient on 128 pixels), G 0.80 .. 0.89 (7)
    "split+ksplit": 1.7,      # 22 cases: D 0.59 .. 1.04 (13), G 0.53 .. 1.08 (9)
    "image": 2.0,             # 9 cases: dconv_dgrad4_image_kernel 1.03 .. 1.28 (5), gconv_image_dgrad_kernel 1.000 (4: one fmaf chain, as torch's)
}


# ----------------------------------------------------------------------------------------------------------------------------
# The discriminators' table.  A case: kind (4 = 4x4 stride 2 pad 1, 3 = 3x3 stride 1 pad 1), op (0 forward, 1 data gradient,
# 2 weight gradient), B, Cin, Cout, H, W (the INPUT's size), sw = tgsr_dconv_set_split's argument, act (forward of the 4x4 form),
# skew = {operand: words off its 16-byte alignment}.
# ----------------------------------------------------------------------------------------------------------------------------
def _d(kind, op, B, Cin, Cout, H, W, sw=1, act=0, skew=None):
    return dict(kind=kind, op=op, B=B, Cin=Cin, Cout=Cout, H=H, W=W, sw=sw, act=act, skew=skew or {})


D_MODE = {(4, 0): "kFwd4", (4, 1): "kDgrad4", (4, 2): "kWgrad4", (3, 0): "kFwd3", (3, 1): "kDgrad3", (3, 2): "kWgrad3"}
D_FN = {(4, 0): "tgsr_conv4x4s2_fwd", (4, 1): "tgsr_conv4x4s2_dgrad", (4, 2): "tgsr_conv4x4s2_wgrad",
        (3, 0): "tgsr_conv3x3_gemm_fwd", (3, 1): "tgsr_conv3x3_gemm_dgrad", (3, 2): "tgsr_conv3x3_gemm_wgrad"}
D_ALIGN = {(4, 0): ("w", "ws"), (4, 1): ("w", "ws"), (4, 2): ("dy",), (3, 0): ("w", "ws"), (3, 1): (), (3, 2): ("dy",)}   # ig_plan's `align`
_F32 = "dconv_igemm_kernel<%s,%s>"             # <MODE, WIDE>
_S6 = "dconv_igemm6_kernel<%s,%s,%s>"          # <MODE, WIDE, APRE>
_C1 = "switch != 0, K % 16 == 0 (weight gradient: pixels per image % 16 == 0), A 16-byte aligned"
_ONE = "; one slab (K <= 128, or >= 512 tiles)"
_KS = "; K split, last slab short"
DTABLE = [
    # ---- fp32 MFMA (switch 0), one slab | K split
    ("tgsr_conv4x4s2_fwd", _F32 % ("kFwd4", "true"), "switch 0; M = Cout <= 64: WIDE" + _ONE + "; act in the GEMM epilogue", _d(4, 0, 2, 3, 8, 16, 16, sw=0, act=1)),
    ("tgsr_conv4x4s2_fwd", _F32 % ("kFwd4", "true"), "switch 0; WIDE" + _KS + "; act in slab_sum_kernel", _d(4, 0, 2, 20, 24, 8, 12, sw=0, act=1)),
    ("tgsr_conv4x4s2_fwd", _F32 % ("kFwd4", "false"), "switch 0; Cout > 64" + _ONE, _d(4, 0, 2, 8, 72, 8, 12, sw=0)),
    ("tgsr_conv4x4s2_fwd", _F32 % ("kFwd4", "false"), "switch 0; Cout > 64" + _KS, _d(4, 0, 2, 20, 136, 8, 8, sw=0)),
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "true"), "switch 0; 4 < M = Cin <= 64: WIDE" + _ONE, _d(4, 1, 2, 8, 16, 8, 12, sw=0)),
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "true"), "switch 0; WIDE" + _KS, _d(4, 1, 2, 24, 80, 8, 8, sw=0)),
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "false"), "switch 0; Cin > 64" + _ONE, _d(4, 1, 2, 72, 16, 8, 12, sw=0)),
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "false"), "switch 0; Cin > 64" + _KS, _d(4, 1, 2, 136, 80, 8, 8, sw=0)),
    ("tgsr_conv3x3_gemm_fwd", _F32 % ("kFwd3", "false"), "switch 0" + _ONE, _d(3, 0, 2, 8, 24, 5, 7, sw=0)),
    ("tgsr_conv3x3_gemm_fwd", _F32 % ("kFwd3", "false"), "switch 0" + _KS, _d(3, 0, 1, 48, 80, 4, 8, sw=0)),
    ("tgsr_conv3x3_gemm_dgrad", _F32 % ("kDgrad3", "false"), "switch 0" + _ONE, _d(3, 1, 2, 24, 8, 5, 7, sw=0)),
    ("tgsr_conv3x3_gemm_dgrad", _F32 % ("kDgrad3", "false"), "switch 0" + _KS, _d(3, 1, 1, 48, 80, 4, 8, sw=0)),
    ("tgsr_conv4x4s2_wgrad", _F32 % ("kWgrad4", "false"), "switch 0" + _ONE, _d(4, 2, 2, 5, 24, 16, 16, sw=0)),
    ("tgsr_conv4x4s2_wgrad", _F32 % ("kWgrad4", "false"), "switch 0" + _KS, _d(4, 2, 5, 5, 24, 16, 16, sw=0)),
    ("tgsr_conv3x3_gemm_wgrad", _F32 % ("kWgrad3", "false"), "switch 0" + _ONE, _d(3, 2, 2, 8, 24, 4, 8, sw=0)),
    ("tgsr_conv3x3_gemm_wgrad", _F32 % ("kWgrad3", "false"), "switch 0" + _KS, _d(3, 2, 5, 8, 24, 4, 16, sw=0)),
    # ---- three-piece form (switch 1), one slab | K split
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "true", "false"), _C1 + "; WIDE" + _ONE + "; act in the GEMM epilogue", _d(4, 0, 2, 3, 8, 16, 16, act=1)),
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "true", "false"), _C1 + "; WIDE" + _KS + "; act in slab_sum_kernel", _d(4, 0, 2, 20, 24, 8, 12, act=1)),
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "false", "false"), _C1 + _ONE, _d(4, 0, 2, 8, 72, 8, 12)),
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "false", "false"), _C1 + _KS, _d(4, 0, 2, 20, 136, 8, 8)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "true", "false"), _C1 + " (4 Cout % 16 == 0); WIDE" + _ONE, _d(4, 1, 2, 8, 16, 8, 12)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "true", "false"), _C1 + "; WIDE" + _KS, _d(4, 1, 2, 24, 80, 8, 8)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "false", "false"), _C1 + _ONE, _d(4, 1, 2, 72, 16, 8, 12)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "false", "false"), _C1 + _KS, _d(4, 1, 2, 136, 80, 8, 8)),
    # ---- ... with the A operand pre-split into LDS images (switch 3)
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "true", "true"), "switch & 2; " + _C1 + "; WIDE" + _ONE, _d(4, 0, 2, 3, 8, 16, 16, sw=3, act=1)),
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "true", "true"), "switch & 2; WIDE" + _KS, _d(4, 0, 2, 20, 24, 8, 12, sw=3, act=1)),
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "false", "true"), "switch & 2" + _ONE, _d(4, 0, 2, 8, 72, 8, 12, sw=3)),
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "false", "true"), "switch & 2" + _KS, _d(4, 0, 2, 20, 136, 8, 8, sw=3)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "true", "true"), "switch & 2; WIDE" + _ONE, _d(4, 1, 2, 8, 16, 8, 12, sw=3)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "true", "true"), "switch & 2; WIDE" + _KS, _d(4, 1, 2, 24, 80, 8, 8, sw=3)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "false", "true"), "switch & 2" + _ONE, _d(4, 1, 2, 72, 16, 8, 12, sw=3)),
    ("tgsr_conv4x4s2_dgrad", _S6 % ("kDgrad4", "false", "true"), "switch & 2" + _KS, _d(4, 1, 2, 136, 80, 8, 8, sw=3)),
    # ---- the 3x3 form and the weight gradients: no WIDE tile, no pre-split A (the static_assert of dconv_igemm6_kernel)
    ("tgsr_conv3x3_gemm_fwd", _S6 % ("kFwd3", "false", "false"), _C1 + " (9 Cin % 16 == 0: K >= 144, so one slab needs >= 512 tiles)" + _ONE,
     _d(3, 0, 16, 16, 24, 63, 65)),
    ("tgsr_conv3x3_gemm_fwd", _S6 % ("kFwd3", "false", "false"), _C1 + _KS, _d(3, 0, 1, 48, 80, 4, 8, sw=3)),
    ("tgsr_conv3x3_gemm_dgrad", _S6 % ("kDgrad3", "false", "false"), _C1 + " (9 Cout % 16 == 0; w read by dwords)" + _ONE,
     _d(3, 1, 16, 24, 16, 63, 65)),
    ("tgsr_conv3x3_gemm_dgrad", _S6 % ("kDgrad3", "false", "false"), _C1 + _KS, _d(3, 1, 1, 48, 80, 4, 8)),
    ("tgsr_conv4x4s2_wgrad", _S6 % ("kWgrad4", "false", "false"), _C1 + _ONE, _d(4, 2, 2, 5, 24, 16, 16)),
    ("tgsr_conv4x4s2_wgrad", _S6 % ("kWgrad4", "false", "false"), _C1 + _KS, _d(4, 2, 5, 5, 24, 16, 16, sw=3)),
    ("tgsr_conv3x3_gemm_wgrad", _S6 % ("kWgrad3", "false", "false"), _C1 + _ONE, _d(3, 2, 4, 8, 24, 4, 8)),
    ("tgsr_conv3x3_gemm_wgrad", _S6 % ("kWgrad3", "false", "false"), _C1 + _KS, _d(3, 2, 5, 8, 24, 4, 16)),
    ("tgsr_conv3x3_gemm_*", "dconv_igemm6_kernel<kFwd3 | kDgrad3 | kWgrad3 | kWgrad4, WIDE = true or APRE = true>",
     "not instantiated: the wide tile and the pre-split A serve the 4x4 form's pixel-column modes (its static_assert)", None),
    # ---- the image layer's data gradient
    ("tgsr_conv4x4s2_dgrad", "dconv_dgrad4_image_kernel<1>", "Cin <= 4 and Cout Cin 64 <= 64 KiB, any switch", _d(4, 1, 2, 1, 8, 8, 8)),
    ("tgsr_conv4x4s2_dgrad", "dconv_dgrad4_image_kernel<2>", "...", _d(4, 1, 2, 2, 12, 6, 10, sw=0)),
    ("tgsr_conv4x4s2_dgrad", "dconv_dgrad4_image_kernel<3>", "... more than one tile of 4 x 64 low-resolution positions", _d(4, 1, 3, 3, 16, 10, 132, sw=3)),
    ("tgsr_conv4x4s2_dgrad", "dconv_dgrad4_image_kernel<4>", "...", _d(4, 1, 1, 4, 16, 12, 20)),
    ("tgsr_conv4x4s2_dgrad", "dconv_dgrad4_image_kernel<3>", "... dx one word off 8 bytes: dword stores, the same bits", _d(4, 1, 2, 3, 16, 10, 12, skew={"out": 1})),
    # ---- the fallbacks into the fp32 MFMA under switch 1
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "false"), "switch 1, 4 Cout % 16 != 0: a partial last chunk", _d(4, 1, 2, 72, 10, 8, 8)),
    ("tgsr_conv4x4s2_wgrad", _F32 % ("kWgrad4", "false"), "switch 1, pixels per image % 16 != 0", _d(4, 2, 3, 5, 16, 8, 12)),
    ("tgsr_conv3x3_gemm_fwd", _F32 % ("kFwd3", "false"), "switch 1, K = 9 Cin % 16 != 0", _d(3, 0, 1, 8, 16, 12, 9)),
    ("tgsr_conv3x3_gemm_wgrad", _F32 % ("kWgrad3", "false"), "switch 1, pixels % 16 != 0", _d(3, 2, 2, 8, 16, 5, 7)),
    ("tgsr_conv4x4s2_fwd", _F32 % ("kFwd4", "true"), "skew: w one word off 16 bytes", _d(4, 0, 2, 3, 8, 16, 16, act=1, skew={"w": 1})),
    ("tgsr_conv4x4s2_fwd", _F32 % ("kFwd4", "false"), "skew: ws one word off 16 bytes, K split", _d(4, 0, 2, 20, 136, 8, 8, skew={"ws": 1})),
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "true"), "skew: w one word off: the scalar class pack", _d(4, 1, 2, 8, 16, 8, 12, skew={"w": 1})),
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "false"), "skew: ws one word off: the scalar class pack, K split", _d(4, 1, 2, 136, 80, 8, 8, skew={"ws": 1})),
    ("tgsr_conv4x4s2_dgrad", _F32 % ("kDgrad4", "true"), "skew: w and ws off under switch 3 (the workspace still holds room for the images)",
     _d(4, 1, 2, 8, 16, 8, 12, sw=3, skew={"w": 3, "ws": 2})),
    ("tgsr_conv4x4s2_wgrad", _F32 % ("kWgrad4", "false"), "skew: dy one word off", _d(4, 2, 2, 5, 24, 16, 16, skew={"dy": 1})),
    ("tgsr_conv3x3_gemm_fwd", _F32 % ("kFwd3", "false"), "skew: w one word off, K split", _d(3, 0, 1, 48, 80, 4, 8, skew={"w": 1})),
    ("tgsr_conv3x3_gemm_wgrad", _F32 % ("kWgrad3", "false"), "skew: dy two words off, K split", _d(3, 2, 5, 8, 24, 4, 16, skew={"dy": 2})),
    # ---- operands the three-piece form reads and writes by dwords stay on it off their alignment
    ("tgsr_conv4x4s2_fwd", _S6 % ("kFwd4", "true", "false"), "x and out one word off: S and the output are dword accesses", _d(4, 0, 2, 3, 8, 16, 16, skew={"x": 1, "out": 1})),
    ("tgsr_conv3x3_gemm_dgrad", _S6 % ("kDgrad3", "false", "false"), "w, dy and dx off: this mode reads w by dwords", _d(3, 1, 1, 48, 80, 4, 8, skew={"w": 1, "dy": 3, "out": 1})),
    ("tgsr_conv4x4s2_wgrad", _S6 % ("kWgrad4", "false", "false"), "x and dw off, dy aligned", _d(4, 2, 2, 5, 24, 16, 16, skew={"x": 1, "out": 3})),
]


def _drows():
    return [r for r in DTABLE if r[3] is not None]


def drow_id(r):
    c = r[3]
    inst = r[1].replace("_kernel", "").replace("<", "_").replace(">", "").replace(",", "_")
    return "%s-%dto%d-B%d-%dx%d-sw%d%s" % (inst, c["Cin"], c["Cout"], c["B"], c["H"], c["W"], c["sw"],
                                          "".join("-%s+%d" % kv for kv in sorted(c["skew"].items())))


@contextlib.contextmanager
def switches(L, sw=None, gform=None):
    """tgsr_dconv_set_split / tgsr_gconv_set_form for the body; both process-wide switches are put back."""
    was_sw = L.tgsr_dconv_set_split(sw) if sw is not None else None
    was_gf = L.tgsr_gconv_set_form(gform) if gform is not None else None
    try:
        yield
    finally:
        if sw is not None:
            L.tgsr_dconv_set_split(was_sw)
        if gform is not None:
            L.tgsr_gconv_set_form(was_gf)


def _ceil(a, b):
    return -(-a // b)


def d_gemm(c):
    """(M, N, K, elements of the output = a slab) of a discriminator case: ig_plan's first lines."""
    kind, op, B, Cin, Cout, H, W = (c[k] for k in ("kind", "op", "B", "Cin", "Cout", "H", "W"))
    T = 16 if kind == 4 else 9
    px = (H // 2) * (W // 2) if kind == 4 else H * W
    if op == 0:
        return Cout, B * px, Cin * T, B * Cout * px
    if op == 1:
        return Cin, B * px, (4 if kind == 4 else 9) * Cout, B * Cin * H * W
    return Cout, Cin * T, B * px, Cout * Cin * T


def d_plan(L, c):
    """What a discriminator case reaches, from the exported planners under the case's switch and the launcher's conditions."""
    kind, op, B, Cin, Cout, H, W, sw = (c[k] for k in ("kind", "op", "B", "Cin", "Cout", "H", "W", "sw"))
    form, wsf = (L.tgsr_conv4x4s2_split_form, L.tgsr_conv4x4s2_ws_elems) if kind == 4 else \
        (L.tgsr_conv3x3_gemm_split_form, L.tgsr_conv3x3_gemm_ws_elems)
    with switches(L, sw=sw):
        split, ws = int(form(op, B, Cin, H, W, Cout)), int(wsf(op, B, Cin, H, W, Cout))
    M, N, K, slab = d_gemm(c)
    wide = kind == 4 and op != 2 and M <= 64
    MB, NB = (64, 256) if wide else (128, 128)
    canpre = bool(sw & 2) and kind == 4 and op != 2
    # the head of the workspace: the data gradient's fp32 class pack, or (switch & 2) the split images of A, whichever is larger
    img = (4 if op == 1 else 1) * _ceil(M, MB) * MB * K * 3 // 2 if canpre and K % 16 == 0 else 0
    head = max(img, 16 * Cin * Cout if (kind == 4 and op == 1) else 0)
    asked = max(1, (ws - head) // slab)                                   # (a planner that needs no workspace answers 1 float)
    assert ws == max(1, head + (asked * slab if asked > 1 else 0)), "the workspace is [head | asked slabs]"
    chunks = _ceil(K, 16)
    cps = _ceil(chunks, asked)
    nsplit = _ceil(chunks, cps)
    if kind == 4 and op == 1 and Cin <= 4 and Cout * Cin * 64 <= 64 * 1024:
        assert split == 0
        inst = "dconv_dgrad4_image_kernel<%d>" % Cin
    elif split and not any(c["skew"].get(n, 0) % 4 for n in D_ALIGN[(kind, op)]):
        inst = _S6 % (D_MODE[(kind, op)], "true" if wide else "false", "true" if canpre else "false")
    else:
        inst = _F32 % (D_MODE[(kind, op)], "true" if wide else "false")
    return dict(instance=inst, split=split, ws=ws, head=head, slab=slab, M=M, N=N, K=K, MB=MB, NB=NB, chunks=chunks, cps=cps,
                nsplit=nsplit, last=chunks - (nsplit - 1) * cps, image=inst.startswith("dconv_dgrad4"))


def check_plan_claims(cond, p):
    """What a row's dispatch condition claims about its K split and its statistics slots, asserted on the plan."""
    if "one slab" in cond:
        assert p["nsplit"] == 1
    if "last slab short" in cond:
        assert p["nsplit"] > 1 and p["last"] < p["cps"], "no K split with a short last slab: cps %d, last %d" % (p["cps"], p["last"])
    if "2048-pixel slot short" in cond:
        assert p["nsplit"] > 1 and p["slot_px"] == 2048 and p["nslots"] > 1 and p["N"] % 2048 != 0
    if "two N tiles" in cond:
        assert p["nslots"] == 2 and p["N"] % p["NB"] != 0


def d_group(p):
    g = "image" if p["image"] else "split" if "igemm6" in p["instance"] else "fp32"
    return g + ("+ksplit" if p["nsplit"] > 1 and not p["image"] else "")


# ---- inputs and references (CPU; computed once per shape and shared)
def _dkey(c):
    return (c["kind"], c["B"], c["Cin"], c["Cout"], c["H"], c["W"])


@functools.lru_cache(maxsize=None)
def d_inputs(key):
    kind, B, Cin, Cout, H, W = key
    g = torch.Generator().manual_seed(kind * 100000 + B * 1000 + Cin + 7 * Cout + 13 * H + W)
    Ho, Wo = (H // 2, W // 2) if kind == 4 else (H, W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, kind, kind, generator=g) / (kind * Cin ** 0.5)
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    return x, w, dy


def d_reference(kind, op, act, x, w, dy, dtype):
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    st = 2 if kind == 4 else 1
    if op == 0:
        y = F.conv2d(x, w, None, st, 1)
        return F.leaky_relu(y, 0.2) if act else y
    if op == 1:
        return torch.nn.grad.conv2d_input(x.shape, w, dy, st, 1)
    return torch.nn.grad.conv2d_weight(x, w.shape, dy, st, 1)


@functools.lru_cache(maxsize=None)
def d_refs(key, op, act):
    x, w, dy = d_inputs(key)
    return d_reference(key[0], op, act, x, w, dy, torch.float64), d_reference(key[0], op, act, x, w, dy, torch.float32)


def d_tol(c, ref):
    """(atol, rtol): tests/test_hip_gan.py's - 1e-4 / 1e-4 for the 4x4 form's forward and data gradient, 2e-5 / 1e-4 for the 3x3
    form's, 2e-4 max |ref| / 2e-4 for the weight gradients."""
    if c["op"] == 2:
        return 2e-4 * float(ref.abs().max()), 2e-4
    return (1e-4 if c["kind"] == 4 else 2e-5), 1e-4


def d_gathered(c):
    """Index of the operand the kernel gathers (the one a ragged-tile bug would drop a border pixel of): x, or dy for the data gradient."""
    return 2 if c["op"] == 1 else 0


def close(got, ref, atol, rtol, what=""):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d of %d values beyond atol %.3g rtol %.3g, worst |err| %.3g at |ref| %.3g" % (
        what, int(bad.sum()), bad.numel(), atol, rtol, float(err.max()), float(ref.abs().flatten()[int(err.argmax())]))


def rel(got, ref):
    """tests/test_hip_inception.py's measure: max |got - ref| over max |ref|"""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ratio(tag, group, rid, got, ref64, ref32):
    own = float((got.double() - ref64).abs().mean())
    cpu = float((ref32.double() - ref64).abs().mean())
    print("IGEMM_RATIO %s %s %s own %.4g cpu %.4g ratio %.3f max|err| %.4g" % (
        tag, group, rid, own, cpu, own / cpu, float((got.double() - ref64).abs().max())))
    cap = R[group]
    assert own <= cap * cpu, "mean |kernel - f64| = %.3g is %.2f x the CPU fp32 result's %.3g (bound %.1f, group %s)" % (
        own, own / cpu, cpu, cap, group)


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(r):
    return r.ptr if r is not None else None


def place_d(c, plan, written=True, ws_elems=None):
    """Every operand of a discriminator call in one arena; returns (arena, regions, the call's arguments)."""
    kind, op, B, Cin, Cout, H, W = (c[k] for k in ("kind", "op", "B", "Cin", "Cout", "H", "W"))
    x, w, dy = d_inputs(_dkey(c))
    sk = c["skew"]
    a = Arena(DEV, guard=max(GUARD, 4 * W + 4096))
    r = {}
    if op != 1:
        r["x"] = a.place_input(x, skew=sk.get("x", 0))
    if op != 2:
        r["w"] = a.place_input(w, skew=sk.get("w", 0))
    if op != 0:
        r["dy"] = a.place_input(dy, skew=sk.get("dy", 0))
    r["ws"] = a.place_ws(plan["ws"] if ws_elems is None else ws_elems, skew=sk.get("ws", 0))
    r["out"] = a.place_output((dy.shape, x.shape, w.shape)[op], skew=sk.get("out", 0), written=written)
    if op == 0:
        args = [r["x"].ptr, B, Cin, H, W, r["w"].ptr, Cout] + ([c["act"]] if kind == 4 else []) + [r["ws"].ptr, r["out"].ptr]
    elif op == 1:
        args = [r["dy"].ptr, B, Cin, H, W, r["w"].ptr, Cout, r["ws"].ptr, r["out"].ptr]
    else:
        args = [r["dy"].ptr, r["x"].ptr, B, Cin, H, W, Cout, r["ws"].ptr, r["out"].ptr]
    for name, mis in sk.items():
        assert r[name].address % 16 == 4 * mis
    return a, r, args


def run_d(L, c, plan):
    """The call twice (the second with a finite workspace) under the case's switch: (first output, arena, regions)."""
    M, _ = _lib()
    a, r, args = place_d(c, plan)
    fn = getattr(L, D_FN[(c["kind"], c["op"])])
    with switches(L, sw=c["sw"]):
        assert fn(*args, _stream()) == M.OK
        a.check()
        got = r["out"].read()
        a.rearm(ws_fill=0.5)
        assert fn(*args, _stream()) == M.OK
        a.check()
    assert same_bits(got, r["out"].read()), "two calls on the same operands differ"
    return got


# ----------------------------------------------------------------------------------------------------------------------------
# 1: the discriminators' entry points, every instance and launch path
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", _drows(), ids=drow_id)
def test_discriminator_entry_points(row):
    _entry, instance, cond, c = row
    _M, L = _lib()
    p = d_plan(L, c)
    assert p["instance"] == instance, "the case reaches %s" % p["instance"]
    check_plan_claims(cond, p)
    got = run_d(L, c, p)
    ref64, ref32 = d_refs(_dkey(c), c["op"], c["act"])
    ratio("D", d_group(p), drow_id(row), got, ref64, ref32)
    atol, rtol = d_tol(c, ref64)
    close(got, ref64, atol, rtol, "out")


@pytest.mark.parametrize("row", [r for r in _drows() if r[3]["skew"] and ("skew" in r[2] or "dword stores" in r[2])], ids=drow_id)
def test_skewed_discriminator_call_equals_the_aligned_fp32_call_bit_for_bit(row):
    """An operand the three-piece form would load 16 bytes at a time, one word off: the launcher takes the fp32 MFMA (and, for the 4x4
    data gradient, the scalar class pack), whose bits are those of the aligned call with the three-piece form switched off."""
    _entry, instance, _cond, c = row
    _M, L = _lib()
    p = d_plan(L, c)
    assert p["instance"] == instance and "igemm6" not in instance
    got = run_d(L, c, p)
    flat = dict(c, skew={}, sw=0 if not p["image"] else c["sw"])
    pf = d_plan(L, flat)
    assert pf["instance"] == instance and (pf["nsplit"], pf["cps"]) == (p["nsplit"], p["cps"])
    # (switch 0 needs no room for the images: the aligned call gets its own planner's workspace)
    assert same_bits(got, run_d(L, flat, pf))


# ----------------------------------------------------------------------------------------------------------------------------
# The trunk's table.  A case: mode ("f" forward, "d" data gradient, "s" the statistics form), geom = (B, Cin, H, W, Cout, kh, kw,
# stride, padh, padw) of the FORWARD layer, gform / sw = the two switches, bias / relu / acc / mask, scale (tgsr_gconv_pack's, or
# NULL), skewA = words A lies off 16 bytes, sextra / oextra = channels of the wider buffers S is a slice of / out is written into,
# spad / opad = further floats on the batch strides, raw = A is the caller's own matrix (ops.linear, ops.conv1x1_wgrad: no pack),
# bn = (running statistics given, num_batches_tracked given) of the slice form that follows a statistics call.
# ----------------------------------------------------------------------------------------------------------------------------
def _g(mode, geom, gform=1, sw=1, bias=0, relu=0, acc=0, mask=0, scale=1, skewA=0, sextra=3, spad=1, oextra=5, opad=3, raw=0, bn=None):
    return dict(mode=mode, geom=geom, gform=gform, sw=sw, bias=bias, relu=relu, acc=acc, mask=mask, scale=scale, skewA=skewA,
                sextra=sextra, spad=spad, oextra=oextra, opad=opad, raw=raw, bn=bn)


_GF = "gconv_igemm_kernel<%s,%s,%s>"               # <DG, WIDE, STATS>
_G6 = "dconv_igemm6_kernel<%s,%s,false,%s>"        # <kFwdG | kDgradG, WIDE, APRE = false, STATS>
_IM = "gconv_image_dgrad_kernel<%d>"
_FIN, _FST = " + gconv_finish_kernel", " + gconv_finish_stats_kernel"
_C6 = "both switches on, KH KW <= 25, K % 16 == 0, A 16-byte aligned"
GCONV, GSTATS = "tgsr_gconv", "tgsr_gconv_stats"
GTABLE = [
    # ---- fp32 MFMA (tgsr_gconv_set_form(0))
    (GCONV, _GF % ("false", "false", "false"), "form 0; M > 64; one slab; 3x3 s1, bias + relu", _g("f", (2, 8, 9, 9, 72, 3, 3, 1, 1, 1), gform=0, bias=1, relu=1)),
    (GCONV, _GF % ("false", "false", "false") + _FIN, "form 0; M > 64; K split, last slab short; bias + relu in the finish", _g("f", (2, 40, 9, 9, 72, 3, 3, 1, 1, 1), gform=0, bias=1, relu=1)),
    (GCONV, _GF % ("false", "true", "false"), "form 0; M <= 64: WIDE; one slab; 1x7", _g("f", (2, 16, 8, 8, 32, 1, 7, 1, 0, 3), gform=0, scale=0)),
    (GCONV, _GF % ("false", "true", "false") + _FIN, "form 0; WIDE; K split, last slab short; 3x3 s2", _g("f", (2, 40, 9, 9, 24, 3, 3, 2, 0, 0), gform=0, bias=1)),
    (GCONV, _GF % ("true", "false", "false"), "form 0; data gradient, M = Cin > 64; one slab; accumulate + mask in the GEMM epilogue", _g("d", (2, 72, 9, 9, 8, 3, 3, 1, 1, 1), gform=0, acc=1, mask=1)),
    (GCONV, _GF % ("true", "false", "false") + _FIN, "form 0; data gradient; K split, last slab short; accumulate + mask in the finish", _g("d", (2, 72, 9, 9, 40, 3, 3, 1, 1, 1), gform=0, acc=1, mask=1)),
    (GCONV, _GF % ("true", "true", "false"), "form 0; data gradient, WIDE; one slab; 7x1", _g("d", (2, 16, 8, 8, 8, 7, 1, 1, 3, 0), gform=0, mask=1)),
    (GCONV, _GF % ("true", "true", "false") + _FIN, "form 0; data gradient, WIDE; K split, last slab short", _g("d", (2, 16, 8, 8, 40, 3, 3, 1, 1, 1), gform=0, acc=1)),
    (GSTATS, _GF % ("false", "false", "true"), "form 0; statistics in the GEMM epilogue (one slab); M > 64", _g("s", (2, 8, 9, 9, 72, 3, 3, 1, 1, 1), gform=0, bn=(1, 1))),
    (GSTATS, _GF % ("false", "true", "true"), "form 0; statistics in the GEMM epilogue; WIDE; two N tiles, the last short", _g("s", (3, 16, 10, 10, 24, 3, 3, 1, 1, 1), gform=0, bn=(0, 0))),
    (GSTATS, _GF % ("false", "true", "false") + _FST, "form 0; K split: the slab finish takes the statistics; the last 2048-pixel slot short",
     _g("s", (2, 16, 34, 34, 24, 5, 5, 1, 2, 2), gform=0, bn=(1, 0))),
    # ---- three-piece form (both switches on)
    (GCONV, _G6 % ("kFwdG", "false", "false"), _C6 + "; M > 64; one slab; 3x3 s1, bias + relu", _g("f", (2, 16, 9, 9, 72, 3, 3, 1, 1, 1), bias=1, relu=1)),
    (GCONV, _G6 % ("kFwdG", "false", "false") + _FIN, _C6 + "; M > 64; K split, last slab short; 5x5", _g("f", (2, 16, 9, 9, 72, 5, 5, 1, 2, 2), bias=1, relu=1)),
    (GCONV, _G6 % ("kFwdG", "true", "false"), _C6 + "; WIDE; one slab; 3x3 s2", _g("f", (2, 16, 9, 9, 24, 3, 3, 2, 0, 0), scale=0)),
    (GCONV, _G6 % ("kFwdG", "true", "false") + _FIN, _C6 + "; WIDE; K split, last slab short; 1x7", _g("f", (2, 48, 8, 8, 32, 1, 7, 1, 0, 3), bias=1)),
    (GCONV, _G6 % ("kDgradG", "false", "false"), _C6 + ", stride 1; M = Cin > 64; one slab; accumulate + mask in the GEMM epilogue", _g("d", (2, 72, 9, 9, 16, 3, 3, 1, 1, 1), acc=1, mask=1)),
    (GCONV, _G6 % ("kDgradG", "false", "false") + _FIN, _C6 + "; data gradient; K split, last slab short; 7x1; accumulate + mask in the finish", _g("d", (2, 72, 9, 9, 48, 7, 1, 1, 3, 0), acc=1, mask=1)),
    (GCONV, _G6 % ("kDgradG", "true", "false"), _C6 + "; data gradient, WIDE; one slab; 3x3", _g("d", (2, 24, 9, 9, 16, 3, 3, 1, 1, 1), mask=1)),
    (GCONV, _G6 % ("kDgradG", "true", "false") + _FIN, _C6 + "; data gradient, WIDE; K split, last slab short; 5x5; mask in the finish", _g("d", (2, 24, 9, 9, 16, 5, 5, 1, 2, 2), mask=1)),
    (GCONV, _G6 % ("kDgradG", "true", "false") + _FIN, _C6 + "; data gradient, WIDE; K split, last slab short; 1x1", _g("d", (2, 24, 9, 9, 272, 1, 1, 1, 0, 0), acc=1)),
    (GCONV, _G6 % ("kDgradG", "true", "false"), "mask given with M <= 4: not the image kernel", _g("d", (2, 3, 9, 9, 16, 3, 3, 1, 1, 1), mask=1, acc=1)),
    (GSTATS, _G6 % ("kFwdG", "false", "true"), _C6 + "; statistics in the GEMM epilogue; M > 64", _g("s", (2, 16, 9, 9, 72, 3, 3, 1, 1, 1), bn=(1, 1))),
    (GSTATS, _G6 % ("kFwdG", "true", "true"), _C6 + "; statistics in the GEMM epilogue; WIDE; two N tiles, the last short", _g("s", (3, 16, 10, 10, 24, 3, 3, 1, 1, 1), bn=(1, 0))),
    (GSTATS, _G6 % ("kFwdG", "true", "false") + _FST, _C6 + "; K split: the slab finish takes the statistics; the last 2048-pixel slot short",
     _g("s", (2, 16, 34, 34, 24, 5, 5, 1, 2, 2), bn=(0, 1))),
    (GSTATS, _G6 % ("kFwdG", "false", "false") + _FST, _C6 + "; K split, M > 64; the last 2048-pixel slot short", _g("s", (2, 48, 34, 34, 72, 1, 7, 1, 0, 3), bn=(1, 1))),
    (GCONV, "dconv_igemm6_kernel<kFwdG | kDgradG, *, true, *> and <kDgradG, *, false, true>",
     "not instantiated: the generic taps take no pre-split A, and the statistics epilogue serves the forward", None),
    # ---- the image kernels: M = Cin <= 4, no mask, M K 4 <= 48 KiB, either form
    (GCONV, _IM % 1, "data gradient, M = 1", _g("d", (2, 1, 9, 9, 8, 3, 3, 1, 1, 1))),
    (GCONV, _IM % 2, "data gradient, M = 2; 1x7; accumulate", _g("d", (2, 2, 8, 8, 8, 1, 7, 1, 0, 3), acc=1, gform=0)),
    (GCONV, _IM % 3, "data gradient, M = 3; 3x3 s2 (Conv2d_1a_3x3); more than one workgroup", _g("d", (2, 3, 17, 17, 32, 3, 3, 2, 0, 0), acc=1)),
    (GCONV, _IM % 4, "data gradient, M = 4; 5x5", _g("d", (1, 4, 10, 10, 8, 5, 5, 1, 2, 2))),
    # ---- the predicates of gc_plan that send a call to the fp32 MFMA with both switches on
    (GCONV, _GF % ("false", "true", "false"), "form 1; KH KW = 36 > 25", _g("f", (2, 4, 10, 10, 16, 6, 6, 1, 0, 0))),
    (GCONV, _GF % ("false", "true", "false"), "form 1; K = 27: K % 16 != 0", _g("f", (2, 3, 17, 17, 32, 3, 3, 2, 0, 0), bias=1, relu=1)),
    (GCONV, _GF % ("true", "true", "false") + _FIN, "form 1; data gradient at stride 2", _g("d", (2, 32, 9, 9, 96, 3, 3, 2, 0, 0), acc=1, mask=1)),
    (GCONV, _GF % ("false", "true", "false"), "form 1; A one word off 16 bytes", _g("f", (2, 16, 8, 8, 32, 3, 3, 1, 1, 1), skewA=1)),
    (GCONV, _GF % ("false", "false", "false"), "form 1, tgsr_dconv_set_split(0): the same kernel's other switch", _g("f", (2, 16, 9, 9, 72, 3, 3, 1, 1, 1), sw=0)),
    (GSTATS, _GF % ("false", "true", "true"), "form 1; K = 27: statistics on the fp32 MFMA", _g("s", (2, 3, 17, 17, 32, 3, 3, 2, 0, 0), bn=(0, 0))),
    # ---- the caller forms of tgsr_amd/ops.py: A is the caller's own matrix, the "image" a transposed matrix
    (GCONV, _G6 % ("kFwdG", "true", "false") + _FIN, "ops.linear: x^T as a [1, K, B, 1] image at B = 1 - PH = PW = 1; bias in the finish", _g("f", (1, 336, 1, 1, 40, 1, 1, 1, 0, 0), bias=1, raw=1, scale=0, sextra=0, spad=0, oextra=0, opad=0)),
    (GCONV, _G6 % ("kFwdG", "true", "false") + _FIN, "ops.conv1x1_wgrad: K = B H W pixels as the channels, Cin as the pixels", _g("f", (1, 336, 72, 1, 24, 1, 1, 1, 0, 0), raw=1, scale=0, sextra=0, spad=0, oextra=0, opad=0)),
]


def _grows(*entries):
    return [r for r in GTABLE if r[3] is not None and (not entries or r[0] in entries)]


def grow_id(r):
    c = r[3]
    inst = r[1].replace("_kernel", "").replace("<", "_").replace(">", "").replace(",", "_").replace(" + ", "+")
    flags = "".join(k[0] for k in ("bias", "relu", "acc", "mask") if c[k]) + ("A+%d" % c["skewA"] if c["skewA"] else "")
    return "%s-%s-%s-gf%dsw%d%s" % (inst, c["mode"], "x".join(map(str, c["geom"])), c["gform"], c["sw"], "-" + flags if flags else "")


def g_dims(c):
    """GEMM and gather sizes of a trunk case: dict(M, N, K, KK, sch = channels of S, Hs, Ws, PH, PW, slab)."""
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = c["geom"]
    OH, OW = (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1
    KK = kh * kw
    if c["mode"] == "d":
        d = dict(M=Cin, K=Cout * KK, sch=Cout, Hs=OH, Ws=OW, PH=H, PW=W)
    else:
        d = dict(M=Cout, K=Cin * KK, sch=Cin, Hs=H, Ws=W, PH=OH, PW=OW)
    d.update(B=B, KK=KK, N=B * d["PH"] * d["PW"], slab=B * d["M"] * d["PH"] * d["PW"], OH=OH, OW=OW)
    return d


def g_plan(L, c):
    """What a trunk case reaches: split, workspace and slots from the exported planners, the form from gc_plan's conditions."""
    d = g_dims(c)
    M, N, K, KK, B = d["M"], d["N"], d["K"], d["KK"], d["B"]
    st = c["geom"][7]
    asked = int(L.tgsr_gconv_nsplit(M, N, K))
    ws = int(L.tgsr_gconv_ws_elems(B, M, d["PH"], d["PW"], K))
    assert ws == (asked * d["slab"] if asked > 1 else 0), "the workspace is `asked` slabs, none for one"
    chunks = _ceil(K, 16)
    cps = _ceil(chunks, asked)
    nsplit = _ceil(chunks, cps)
    wide = M <= 64
    NB = 256 if wide else 128
    nslots, slot_px = int(L.tgsr_gconv_stats_nslots(B, M, d["PH"], d["PW"], K)), int(L.tgsr_gconv_stats_slot_pixels(B, M, d["PH"], d["PW"], K))
    assert slot_px == (2048 if nsplit > 1 else NB) and nslots == _ceil(N, slot_px)
    mode = c["mode"]
    w, f = ("true" if wide else "false"), "false"
    stats = mode == "s" and nsplit == 1
    if mode == "d" and M <= 4 and not c["mask"] and M * K * 4 <= 48 * 1024:
        inst, form = _IM % M, "image"
    elif c["gform"] and c["sw"] and KK <= 25 and K % 16 == 0 and not (mode == "d" and st != 1) and not c["skewA"] % 4:
        inst, form = _G6 % ("kDgradG" if mode == "d" else "kFwdG", w, "true" if stats else f), "split"
    else:
        inst, form = _GF % ("true" if mode == "d" else f, w, "true" if stats else f), "fp32"
    if form != "image" and nsplit > 1:
        inst += _FST if mode == "s" else _FIN
    return dict(d, instance=inst, form=form, asked=asked, ws=ws, chunks=chunks, cps=cps, nsplit=1 if form == "image" else nsplit,
                last=chunks - (nsplit - 1) * cps, nslots=nslots, slot_px=slot_px, wide=wide, NB=NB)


def g_group(p):
    return p["form"] + ("+ksplit" if p["nsplit"] > 1 else "")


def _gkey(c):
    return ("d" if c["mode"] == "d" else "f", c["geom"], c["bias"], c["relu"], c["acc"], c["mask"], c["scale"])     # (the statistics form: the forward's inputs)


@functools.lru_cache(maxsize=None)
def g_inputs(key):
    """x, w, scale, bias, dy, base (what an accumulating call adds to), mask (about half zeros), the BatchNorm affine and running statistics"""
    mode, geom, _bias, _relu, _acc, _mask, scale = key
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = geom
    g = torch.Generator().manual_seed(sum((i + 3) * v for i, v in enumerate(geom)) + ord(mode))
    OH, OW = (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1
    t = dict(x=torch.randn(B, Cin, H, W, generator=g), w=torch.randn(Cout, Cin, kh, kw, generator=g) / (Cin * kh * kw) ** 0.5,
             scale=0.5 + torch.rand(Cout, generator=g), bias=0.2 * torch.randn(Cout, generator=g),
             dy=torch.randn(B, Cout, OH, OW, generator=g), base=torch.randn(B, Cin, H, W, generator=g),
             mask=(torch.randn(B, Cin, H, W, generator=g) > 0).float(), gamma=0.5 + torch.rand(Cout, generator=g),
             beta=0.2 * torch.randn(Cout, generator=g), rm=0.1 * torch.randn(Cout, generator=g), rv=0.5 + torch.rand(Cout, generator=g))
    # the filter the kernels multiply with: tgsr_gconv_pack's fp32 product w * scale[co] (one rounding, the same on the host)
    t["wp"] = t["w"] * t["scale"][:, None, None, None] if scale else t["w"]
    return t


def g_reference(key, dtype, cut=False):
    """The operation of a trunk case on the CPU in `dtype`; cut: one border pixel (last row, last column of the last sample) of the
    gathered operand zeroed."""
    mode, geom, bias, relu, acc, mask, _scale = key
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = geom
    t = g_inputs(key)
    wp = t["wp"].to(dtype)
    s = (t["dy"] if mode == "d" else t["x"]).to(dtype).clone()
    if cut:
        s[-1, :, -1, -1] = 0
    if mode == "d":
        y = torch.nn.grad.conv2d_input((B, Cin, H, W), wp, s, st, (ph, pw))
        if mask:
            y = torch.where(t["mask"] > 0, y, torch.zeros_like(y))
        return t["base"].to(dtype) + y if acc else y
    y = F.conv2d(s, wp, t["bias"].to(dtype) if bias else None, st, (ph, pw))
    return F.relu(y) if relu else y


@functools.lru_cache(maxsize=None)
def g_refs(key):
    return g_reference(key, torch.float64), g_reference(key, torch.float32)


G_CAP = {"f": 2e-5, "s": 2e-5, "d": 5e-5}       # max |err| / max |ref|: tests/test_hip_inception.py, tests/test_hip_inception_train.py


def g_contribution(c, t, full):
    """What the call itself computed: an accumulating call's output less what it was added to."""
    return full.double() - t["base"].double() if c["acc"] else full.double()


def run_gpack(L, w, scale, dgrad):
    """tgsr_gconv_pack on the device into an arena output of exactly Cout Cin KK floats."""
    M, _ = _lib()
    Cout, Cin, kh, kw = w.shape
    a = Arena(DEV)
    wr = a.place_input(w)
    sr = a.place_input(scale) if scale is not None else None
    pk = a.place_output((Cin, Cout * kh * kw) if dgrad else (Cout, Cin * kh * kw))
    assert L.tgsr_gconv_pack(wr.ptr, _p(sr), pk.ptr, Cout, Cin, kh * kw, 1 if dgrad else 0, _stream()) == M.OK
    a.check()
    return pk.read()


def place_g(L, c, p, A, written=True, stat_rows=None):
    """Every operand of a trunk call in one arena; returns (arena, regions, named arguments)."""
    t = g_inputs(_gkey(c))
    B, M, K, Hs, Ws, PH, PW, sch = (p[k] for k in ("B", "M", "K", "Hs", "Ws", "PH", "PW", "sch"))
    _B, _Cin, _H, _W, _Cout, kh, kw, st, ph, pw = c["geom"]
    sbs = (sch + c["sextra"]) * Hs * Ws + c["spad"]
    obs = (M + c["oextra"]) * PH * PW + c["opad"]
    a = Arena(DEV, guard=max(GUARD, 8 * max(Ws, PW) + 4096))
    r = dict(A=a.place_input(A, skew=c["skewA"]), S=a.place_input(t["dy"] if c["mode"] == "d" else t["x"], bstride=sbs),
             bias=a.place_input(t["bias"]) if c["bias"] else None,
             mask=a.place_input(t["mask"], bstride=obs) if c["mask"] else None,
             ws=a.place_ws(p["ws"]) if p["ws"] else None)
    if c["acc"] and written:
        r["out"] = a.place_inout(t["base"], bstride=obs)
    else:
        r["out"] = a.place_output((B, M, PH, PW), bstride=obs, written=written)
    r["stat"] = a.place_output((M, stat_rows or p["nslots"], 2), written=written) if c["mode"] == "s" else None
    if c["bn"] is not None:
        r.update(gamma=a.place_input(t["gamma"]), beta=a.place_input(t["beta"]),
                 rm=a.place_inout(t["rm"]) if c["bn"][0] else None, rv=a.place_inout(t["rv"]) if c["bn"][0] else None,
                 nbt=a.place_inout(torch.tensor([41], dtype=torch.int64), align=8) if c["bn"][1] else None,
                 stats=a.place_output((4, M), written=written))
    kw_ = dict(dgrad=1 if c["mode"] == "d" else 0, A=r["A"].ptr, S=r["S"].ptr, sbs=sbs, B=B, Hs=Hs, Ws=Ws, M=M, K=K, PH=PH, PW=PW, KH=kh,
               KW=kw, stride=st, padh=ph, padw=pw, bias=_p(r["bias"]), relu=c["relu"], acc=c["acc"], mask=_p(r["mask"]), out=r["out"].ptr,
               obs=obs, ws=_p(r["ws"]), stat=_p(r["stat"]))
    return a, r, kw_


G_ORDER = {GCONV: "dgrad A S sbs B Hs Ws M K PH PW KH KW stride padh padw bias relu acc mask out obs ws",
           GSTATS: "A S sbs B Hs Ws M K PH PW KH KW stride padh padw out obs ws stat"}
BN_EPS, BN_MOM = 1e-3, 0.37


def call_g(L, fn, kw_):
    return getattr(L, fn)(*[kw_[k] for k in G_ORDER[fn].split()], _stream())


def call_bn(L, r, kw_, p, **over):
    """tgsr_bn_train_relu_slice_from_stats in place on the slice the statistics call wrote."""
    a = dict(y=kw_["out"], bstride=kw_["obs"], B=p["B"], C=p["M"], HW=p["PH"] * p["PW"], gamma=r["gamma"].ptr, beta=r["beta"].ptr,
             rm=_p(r["rm"]), rv=_p(r["rv"]), stat=kw_["stat"], nslots=p["nslots"], slot_px=p["slot_px"], stats=r["stats"].ptr, nbt=_p(r["nbt"]))
    a.update(over)
    return L.tgsr_bn_train_relu_slice_from_stats(a["y"], a["bstride"], a["B"], a["C"], a["HW"], a["gamma"], a["beta"], BN_EPS, BN_MOM,
                                                 a["rm"], a["rv"], a["stat"], a["nslots"], a["slot_px"], a["stats"], a["nbt"], _stream())


def g_operand_A(L, c):
    """A as the call gets it: the caller's own matrix (raw), or tgsr_gconv_pack's output read back from its arena."""
    t = g_inputs(_gkey(c))
    Cout, Cin, kh, kw = t["w"].shape
    if c["raw"]:
        assert kh * kw == 1 and c["mode"] == "f" and not c["scale"]
        return t["w"].reshape(Cout, Cin)
    return run_gpack(L, t["w"], t["scale"] if c["scale"] else None, c["mode"] == "d")


# ----------------------------------------------------------------------------------------------------------------------------
# 2: the trunk's convolutions, every instance and launch path
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", _grows(GCONV), ids=grow_id)
def test_gconv_entry_point(row):
    _entry, instance, cond, c = row
    M, L = _lib()
    p = g_plan(L, c)
    assert p["instance"] == instance, "the case reaches %s" % p["instance"]
    check_plan_claims(cond, p)
    A = g_operand_A(L, c)
    a, r, kw_ = place_g(L, c, p, A)
    with switches(L, sw=c["sw"], gform=c["gform"]):
        assert call_g(L, GCONV, kw_) == M.OK
        a.check()
        got = r["out"].read()
        a.rearm(ws_fill=0.5)
        assert call_g(L, GCONV, kw_) == M.OK
        a.check()
    assert same_bits(got, r["out"].read()), "two calls on the same operands differ"
    ref64, ref32 = g_refs(_gkey(c))
    ratio("G", g_group(p), grow_id(row), got, ref64, ref32)
    t = g_inputs(_gkey(c))
    err = rel(g_contribution(c, t, got), g_contribution(c, t, ref64))
    assert err < G_CAP[c["mode"]], "max |err| / max |ref| = %.3g" % err


def chan_combine(stat, N, slot_px):
    """(sum, M2) per channel from the slots' (sum, sum of squared deviations from the slot's mean) by Chan's formula in fp64."""
    pc = stat.double()
    ns = pc.shape[1]
    nt = torch.tensor([min(slot_px, N - t * slot_px) for t in range(ns)], dtype=torch.float64)
    s = pc[:, :, 0].sum(1)
    mean = s / N
    return s, (pc[:, :, 1] + nt * (pc[:, :, 0] / nt - mean[:, None]) ** 2).sum(1)


@pytest.mark.parametrize("row", _grows(GSTATS), ids=grow_id)
def test_gconv_stats_and_the_slice_form(row):
    """tgsr_gconv_stats into a slice and exactly M x nslots x 2 partials, then tgsr_bn_train_relu_slice_from_stats in place on that
    slice; the raw output equals tgsr_gconv(dgrad = 0, bias = NULL, relu = 0, accumulate = 0, mask = NULL) in the same form bit for bit."""
    _entry, instance, cond, c = row
    M, L = _lib()
    p = g_plan(L, c)
    assert p["instance"] == instance, "the case reaches %s" % p["instance"]
    check_plan_claims(cond, p)
    A = g_operand_A(L, c)
    t = g_inputs(_gkey(c))
    a, r, kw_ = place_g(L, c, p, A)
    outs = []
    with switches(L, sw=c["sw"], gform=c["gform"]):
        for fill in (None, 0.5):
            a.rearm(ws_fill=fill)
            assert call_g(L, GSTATS, kw_) == M.OK
            torch.cuda.synchronize()
            raw, stat = r["out"].read(), r["stat"].read()
            assert call_bn(L, r, kw_, p) == M.OK
            a.check()
            outs.append((raw, stat, r["out"].read(), r["stats"].read(), r["rm"].read() if r["rm"] else None,
                         r["rv"].read() if r["rv"] else None, int(r["nbt"].read()) if r["nbt"] else None))
        plain = dict(c, mode="f", bn=None)
        b, rb, kwb = place_g(L, plain, p, A)
        assert kwb["bias"] is None and kwb["mask"] is None and not kwb["relu"] and not kwb["acc"]
        assert call_g(L, GCONV, kwb) == M.OK
        b.check()
    raw, stat, y, stats, rm, rv, nbt = outs[0]
    for first, second in zip(outs[0][:6], outs[1][:6]):
        assert first is None or same_bits(first, second), "two calls on the same operands differ"
    assert same_bits(raw, rb["out"].read()), "the raw output differs from tgsr_gconv's in the same form"
    ref64, ref32 = g_refs(_gkey(c))
    ratio("G", g_group(p), grow_id(row), raw, ref64, ref32)
    assert rel(raw, ref64) < G_CAP["s"]
    # the caps of tests/test_hip_inception_train.py: the partials against the kernel's own raw output, the slice form against
    # relu(batch_norm(training = True)) of it in fp64
    r64 = raw.double()
    s, m2 = chan_combine(stat, p["N"], p["slot_px"])
    assert rel(s, r64.sum((0, 2, 3))) < 1e-6
    assert rel(m2, (r64 - r64.mean((0, 2, 3), keepdim=True)).square().sum((0, 2, 3))) < 1e-6
    rm_ref, rv_ref = t["rm"].double().clone(), t["rv"].double().clone()
    ref = F.relu(F.batch_norm(r64, rm_ref, rv_ref, t["gamma"].double(), t["beta"].double(), True, BN_MOM, BN_EPS))
    assert rel(y, ref) < 2e-5
    mean, var = r64.mean((0, 2, 3)), r64.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    assert rel(stats[0], mean) < 2e-5 and rel(stats[1], invstd) < 2e-5 and rel(stats[2], t["gamma"].double() * invstd) < 2e-5
    assert rel(stats[3], t["beta"].double() - mean * t["gamma"].double() * invstd) < 2e-5
    if c["bn"][0]:
        assert rel(rm, rm_ref) < 2e-5 and rel(rv, rv_ref) < 2e-5
    if c["bn"][1]:
        assert nbt == 42


@pytest.mark.parametrize("dgrad,scale", [(0, 1), (0, 0), (1, 1), (1, 0)])
def test_gconv_pack_is_the_exact_product_in_its_layout(dgrad, scale):
    """w [Cout][Cin][KK] * scale[co] -> [Cout][Cin KK] (dgrad 0) or [Cin][Cout KK] (dgrad 1): one fp32 product, bit for bit."""
    _M, L = _lib()
    g = torch.Generator().manual_seed(11 + dgrad)
    w, s = torch.randn(37, 5, 3, 7, generator=g), 0.5 + torch.rand(37, generator=g)       # 3885 floats: more than one workgroup, ragged
    got = run_gpack(L, w, s if scale else None, dgrad)
    ws = w * s[:, None, None, None] if scale else w
    want = ws.permute(1, 0, 2, 3).reshape(5, 37 * 21) if dgrad else ws.reshape(37, 5 * 21)
    assert same_bits(got, want.contiguous())


# ----------------------------------------------------------------------------------------------------------------------------
# 3: refusals - the documented code, and the arena untouched.  Every condition is refused on the host, ahead of any launch
# (dconv_fwd / dconv_dgrad / dconv_wgrad's first three lines, gc_run's first five and its `nsplit > 1 && !ws`, the four tests at the
# top of tgsr_bn_train_relu_slice_from_stats).
# ----------------------------------------------------------------------------------------------------------------------------
D_BASE = {(4, 0): _d(4, 0, 2, 3, 8, 8, 8), (4, 1): _d(4, 1, 2, 8, 16, 8, 8), (4, 2): _d(4, 2, 2, 5, 8, 8, 8),
          (3, 0): _d(3, 0, 2, 8, 16, 4, 4), (3, 1): _d(3, 1, 2, 8, 16, 4, 4), (3, 2): _d(3, 2, 2, 8, 16, 4, 4)}
G_BASE = _g("f", (2, 16, 8, 8, 32, 3, 3, 1, 1, 1), bias=1, relu=1)
G_BASE_SPLIT = _g("f", (2, 48, 8, 8, 32, 1, 7, 1, 0, 3))                        # K split: a workspace is required
G_BASE_D = _g("d", (2, 16, 8, 8, 16, 3, 3, 1, 1, 1), mask=1)
S_BASE = _g("s", (2, 16, 8, 8, 32, 3, 3, 1, 1, 1), bn=(1, 1))


def _refusals():
    out = []
    for (kind, op), base in D_BASE.items():
        fn = D_FN[(kind, op)][5:]
        names = {0: ("x", "w"), 1: ("dy", "w"), 2: ("dy", "x")}[op] + ("ws", "out")
        out += [("%s-null_%s" % (fn, n), "d", base, dict(null=n), E) for n in names]
        out += [("%s-no_sample" % fn, "d", base, dict(B=0), E), ("%s-no_channel" % fn, "d", base, dict(Cin=0), E),
                ("%s-one_row" % fn, "d", base, dict(H=1), E)]
        if kind == 4:
            out += [("%s-odd_h" % fn, "d", base, dict(H=7), U), ("%s-odd_w" % fn, "d", base, dict(W=7), U)]
    for n in ("A", "S", "out"):
        out.append(("gconv-null_%s" % n, "g", G_BASE, dict(**{n: None}), E))
    out += [("gconv-72_taps", "g", G_BASE, dict(KH=9, KW=8), U), ("gconv-stride_3", "g", G_BASE, dict(stride=3), U),
            ("gconv-no_tap", "g", G_BASE, dict(KH=0), U), ("gconv-negative_pad", "g", G_BASE, dict(padh=-1), U),
            ("gconv-k_not_whole_filters", "g", G_BASE, dict(K=16 * 9 - 1), E), ("gconv-no_sample", "g", G_BASE, dict(B=0), E),
            ("gconv-dgrad_with_bias", "g", dict(G_BASE_D, bias=1), {}, E), ("gconv-dgrad_with_relu", "g", dict(G_BASE_D, relu=1), {}, E),
            ("gconv-k_split_without_ws", "g", G_BASE_SPLIT, dict(ws=None), E),
            ("gconv_stats-null_stat_partial", "s", S_BASE, dict(stat=None), E), ("gconv_stats-null_out", "s", S_BASE, dict(out=None), E),
            ("gconv_stats-stride_3", "s", S_BASE, dict(stride=3), U),
            ("bn_slice-one_slot_too_many", "b", S_BASE, dict(nslots=2), E), ("bn_slice-slots_do_not_cover", "b", S_BASE, dict(slot_px=64), E),
            ("bn_slice-bstride_inside_the_slice", "b", S_BASE, dict(bstride=32 * 64 - 1), U),
            ("bn_slice-running_mean_alone", "b", S_BASE, dict(rv=None), E), ("bn_slice-running_var_alone", "b", S_BASE, dict(rm=None), E),
            ("bn_slice-null_gamma", "b", S_BASE, dict(gamma=None), E), ("bn_slice-null_stats", "b", S_BASE, dict(stats=None), E),
            ("bn_slice-stat_partial_off_8_bytes", "b", S_BASE, dict(stat="skew"), U)]
    return out


@pytest.mark.parametrize("tag,what,base,over,code", _refusals(), ids=[r[0] for r in _refusals()])
def test_entry_point_refuses_and_writes_nothing(tag, what, base, over, code):
    M, L = _lib()
    if what == "d":
        p = d_plan(L, base)
        c = dict(base, **{k: v for k, v in over.items() if k != "null"})        # (the arena keeps the base shape: a refused call reads nothing)
        a, r, args = place_d(base, p, written=False)
        kind, op = base["kind"], base["op"]
        ptrs = {"x": r.get("x"), "w": r.get("w"), "dy": r.get("dy"), "ws": r["ws"], "out": r["out"]}
        v = {n: (None if over.get("null") == n or reg is None else reg.ptr) for n, reg in ptrs.items()}
        dims = [c["B"], c["Cin"], c["H"], c["W"]]
        if op == 0:
            args = [v["x"]] + dims + [v["w"], c["Cout"]] + ([0] if kind == 4 else []) + [v["ws"], v["out"]]
        elif op == 1:
            args = [v["dy"]] + dims + [v["w"], c["Cout"], v["ws"], v["out"]]
        else:
            args = [v["dy"], v["x"]] + dims + [c["Cout"], v["ws"], v["out"]]
        assert getattr(L, D_FN[(kind, op)])(*args, _stream()) == code
        a.check()
        return
    p = g_plan(L, base)
    g = torch.Generator().manual_seed(5)
    A = torch.randn(p["M"], p["K"], generator=g)                  # a refused call reads no pack: any floats will do
    a, r, kw_ = place_g(L, base, p, A, written=False)
    if what == "b":
        b = Arena(DEV)                                            # partials of the right size, one word off their 8-byte alignment
        skewed = b.place_input(torch.zeros(p["M"], p["nslots"], 2), align=8, skew=1)
        assert skewed.address % 8 == 4
        ov = {k: (skewed.ptr if v == "skew" else v) for k, v in over.items()}
        assert call_bn(L, r, kw_, p, **ov) == code
        b.check()
    else:
        kw_.update(over)
        assert call_g(L, GSTATS if what == "s" else GCONV, kw_) == code
    a.check()                                                     # out, stat_partial and stats still hold their prefill


def test_planners_refuse_an_unknown_op_and_a_shape_the_calls_refuse():
    _M, L = _lib()
    for form, ws in ((L.tgsr_conv4x4s2_split_form, L.tgsr_conv4x4s2_ws_elems), (L.tgsr_conv3x3_gemm_split_form, L.tgsr_conv3x3_gemm_ws_elems)):
        for op in (-1, 3):
            assert form(op, 2, 16, 8, 8, 32) == 0 and ws(op, 2, 16, 8, 8, 32) == 0
        assert form(0, 0, 16, 8, 8, 32) == 0 and form(0, 2, 16, 1, 8, 32) == 0
    assert L.tgsr_conv4x4s2_split_form(0, 2, 16, 7, 8, 32) == 0
    assert L.tgsr_gconv_stats_nslots(0, 32, 8, 8, 144) == 0 and L.tgsr_gconv_stats_slot_pixels(2, 0, 8, 8, 144) == 0


# ----------------------------------------------------------------------------------------------------------------------------
# 4: the trunk's strided companions (csrc/tgsr_igemm.hip): every access is a dword access, every batch stride padded
# ----------------------------------------------------------------------------------------------------------------------------
def twice(a, outs, call):
    """`call` twice on the arena (re-armed in between): the documented code, the contract, the same bits; returns the outputs."""
    M, _ = _lib()
    assert call() == M.OK
    a.check()
    got = [o.read() for o in outs]
    a.rearm()
    assert call() == M.OK
    a.check()
    for g_, o in zip(got, outs):
        assert same_bits(g_, o.read()), "two calls on the same operands differ"
    return got


def _rand(*shape, seed=0, levels=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randint(0, levels, shape, generator=g).float() if levels else torch.randn(*shape, generator=g)


def test_maxpool3s2_forward_and_backward_with_ties():
    """Values on four levels: most windows hold their maximum more than once, and the backward routes dy to the FIRST one (torch's
    rule).  All three batch strides padded; the backward accumulates under a strided mask."""
    _M, L = _lib()
    B, C, H, W = 2, 5, 9, 11
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    x, dy, base = _rand(B, C, H, W, levels=4), _rand(B, C, OH, OW, seed=1), _rand(B, C, H, W, seed=2)
    mask = (_rand(B, C, H, W, seed=3) > 0).float()
    xbs, ybs, dbs = (C + 2) * H * W + 1, (C + 3) * OH * OW + 3, (C + 1) * H * W + 5
    a = Arena(DEV)
    xr, out = a.place_input(x, bstride=xbs), a.place_output((B, C, OH, OW), bstride=ybs)
    (y,) = twice(a, [out], lambda: L.tgsr_maxpool3s2_fwd(xr.ptr, xbs, B, C, H, W, out.ptr, ybs, _stream()))
    assert same_bits(y, F.max_pool2d(x, 3, 2))
    a = Arena(DEV)
    xr, gr, mr = a.place_input(x, bstride=xbs), a.place_input(dy, bstride=ybs), a.place_input(mask, bstride=dbs)
    dx = a.place_inout(base, bstride=dbs)
    (got,) = twice(a, [dx], lambda: L.tgsr_maxpool3s2_bwd(xr.ptr, xbs, gr.ptr, ybs, B, C, H, W, dx.ptr, dbs, 1, mr.ptr, _stream()))
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 2).backward(dy.double())
    assert rel(got, base.double() + torch.where(mask > 0, x64.grad, torch.zeros_like(x64.grad))) < 1e-6
    a = Arena(DEV)                                                   # ... and plain: no mask, no accumulate
    xr, gr, dx = a.place_input(x, bstride=xbs), a.place_input(dy, bstride=ybs), a.place_output((B, C, H, W), bstride=dbs)
    (got,) = twice(a, [dx], lambda: L.tgsr_maxpool3s2_bwd(xr.ptr, xbs, gr.ptr, ybs, B, C, H, W, dx.ptr, dbs, 0, None, _stream()))
    assert rel(got, x64.grad) < 1e-6


def test_avgpool3_accumulates_under_a_strided_mask():
    _M, L = _lib()
    B, C, H, W = 2, 3, 7, 10
    x, base, mask = _rand(B, C, H, W), _rand(B, C, H, W, seed=1), (_rand(B, C, H, W, seed=2) > 0).float()
    xbs, obs = (C + 2) * H * W + 3, (C + 1) * H * W + 1
    a = Arena(DEV)
    xr, mr, out = a.place_input(x, bstride=xbs), a.place_input(mask, bstride=obs), a.place_inout(base, bstride=obs)
    (got,) = twice(a, [out], lambda: L.tgsr_avgpool3(xr.ptr, xbs, B, C, H, W, out.ptr, obs, 1, mr.ptr, _stream()))
    ref = F.avg_pool2d(x.double(), 3, 1, 1)
    assert rel(got, base.double() + torch.where(mask > 0, ref, torch.zeros_like(ref))) < 1e-6
    a = Arena(DEV)
    xr, out = a.place_input(x, bstride=xbs), a.place_output((B, C, H, W), bstride=obs)
    (got,) = twice(a, [out], lambda: L.tgsr_avgpool3(xr.ptr, xbs, B, C, H, W, out.ptr, obs, 0, None, _stream()))
    assert rel(got, ref) < 1e-6


def test_relu_mask_with_three_different_strides():
    _M, L = _lib()
    B, per = 3, 5 * 7 * 9
    dy, y = _rand(B, per), _rand(B, per, seed=1)
    a = Arena(DEV)
    gr, yr, out = a.place_input(dy, bstride=per + 11), a.place_input(y, bstride=per + 64), a.place_output((B, per), bstride=per + 3)
    (got,) = twice(a, [out], lambda: L.tgsr_relu_mask(gr.ptr, per + 11, yr.ptr, per + 64, out.ptr, per + 3, B, per, _stream()))
    assert same_bits(got, torch.where(y > 0, dy, torch.zeros_like(dy)))


def _classes(planes, H, W, seed):
    return [_rand(planes, (H - py + 1) // 2, (W - px + 1) // 2, seed=seed + 2 * py + px) if (H > py and W > px) else None
            for py in (0, 1) for px in (0, 1)]                      # t00, t01, t10, t11


def _weave(ts, planes, H, W):
    out = torch.zeros(planes, H, W)
    for i, t in enumerate(ts):
        if t is not None:
            out[:, i // 2::2, i % 2::2] = t
    return out


@pytest.mark.parametrize("H,W,acc", [(5, 7, 1), (6, 4, 0), (1, 5, 0), (4, 1, 1), (1, 1, 0)])
def test_interleave2x2(H, W, acc):
    """Odd sizes (the classes differ in size), accumulate under a mask, and the H = 1 / W = 1 forms whose absent classes are NULL."""
    M, L = _lib()
    planes = 3
    ts = _classes(planes, H, W, seed=H * 10 + W)
    base, mask = _rand(planes, H, W, seed=50), (_rand(planes, H, W, seed=51) > 0).float()
    a = Arena(DEV)
    tr = [a.place_input(t) if t is not None else None for t in ts]
    mr = a.place_input(mask) if acc else None
    dx = a.place_inout(base) if acc else a.place_output((planes, H, W))
    (got,) = twice(a, [dx], lambda: L.tgsr_interleave2x2(_p(tr[0]), _p(tr[1]), _p(tr[2]), _p(tr[3]), dx.ptr, planes, H, W, acc, _p(mr), _stream()))
    woven = _weave(ts, planes, H, W)
    assert same_bits(got, base + torch.where(mask > 0, woven, torch.zeros_like(woven)) if acc else woven)
    assert [t is None for t in ts] == [False, W == 1, H == 1, H == 1 or W == 1]


@pytest.mark.parametrize("H,W,missing", [(4, 6, 1), (4, 6, 2), (4, 6, 3), (4, 6, 0), (1, 6, 1), (4, 1, 2)])
def test_interleave2x2_refuses_a_missing_class_and_writes_nothing(H, W, missing):
    M, L = _lib()
    ts = _classes(2, H, W, seed=7)
    a = Arena(DEV)
    tr = [a.place_input(t) if t is not None else None for t in ts]
    dx = a.place_output((2, H, W), written=False)
    ptrs = [None if i == missing else _p(t) for i, t in enumerate(tr)]
    assert L.tgsr_interleave2x2(*ptrs, dx.ptr, 2, H, W, 0, None, _stream()) == M.EINVAL
    a.check()


@pytest.mark.parametrize("n", [1, 4])
def test_sum_stack(n):
    """out[k] = ((parts[0][k] + parts[1][k]) + parts[2][k]) + parts[3][k]: fp32 adds in that order, bit for bit; m % 4 != 0 and a
    pointer off 16 bytes are refused (the kernel is 16-byte loads and stores) with nothing written."""
    M, L = _lib()
    m = 4 * 517                                                      # 517 float4s: three workgroups, the last one short
    parts = _rand(n, m, seed=n)
    a = Arena(DEV)
    pr, out = a.place_input(parts), a.place_output((m,))
    (got,) = twice(a, [out], lambda: L.tgsr_sum_stack(pr.ptr, n, m, out.ptr, _stream()))
    want = parts[0].clone()
    for z in range(1, n):
        want = want + parts[z]
    assert same_bits(got, want)
    for skew_p, skew_o, mm in ((1, 0, m), (0, 1, m), (2, 0, m), (0, 0, m - 2)):
        a = Arena(DEV)
        pr, out = a.place_input(parts, skew=skew_p), a.place_output((m,), skew=skew_o, written=False)
        assert L.tgsr_sum_stack(pr.ptr, n, mm, out.ptr, _stream()) == M.EUNSUPPORTED
        a.check()


@pytest.mark.parametrize("planes,HW", [(7, 64), (5, 23 * 17), (2, 3)])
def test_plane_mean_and_its_backward(planes, HW):
    """One wave per plane, four planes per workgroup: planes that are no multiple of 4, HW below, at and above a wave's 64 lanes."""
    _M, L = _lib()
    x, dm = _rand(planes, HW), _rand(planes, seed=1)
    a = Arena(DEV)
    xr, out = a.place_input(x), a.place_output((planes,))
    (got,) = twice(a, [out], lambda: L.tgsr_plane_mean(xr.ptr, out.ptr, planes, HW, _stream()))
    assert rel(got, x.double().mean(1)) < 1e-6
    a = Arena(DEV)
    gr, dx = a.place_input(dm), a.place_output((planes, HW))
    (got,) = twice(a, [dx], lambda: L.tgsr_plane_mean_bwd(gr.ptr, dx.ptr, planes, HW, _stream()))
    assert rel(got, (dm.double() / HW)[:, None].expand(planes, HW)) < 1e-6


@pytest.mark.parametrize("H,W,OH,OW", [(5, 7, 12, 11), (13, 9, 6, 5)], ids=["up", "down"])
def test_bilinear_forward_and_backward(H, W, OH, OW):
    _M, L = _lib()
    planes = 3
    x, dy = _rand(planes, H, W), _rand(planes, OH, OW, seed=1)
    a = Arena(DEV)
    xr, out = a.place_input(x), a.place_output((planes, OH, OW))
    (got,) = twice(a, [out], lambda: L.tgsr_bilinear_fwd(xr.ptr, planes, H, W, OH, OW, out.ptr, _stream()))
    x64 = x.double()[None].requires_grad_(True)
    ref = F.interpolate(x64, size=(OH, OW), mode="bilinear", align_corners=False)
    assert rel(got, ref[0].detach()) < 3e-5
    ref.backward(dy.double()[None])
    a = Arena(DEV)
    gr, dx = a.place_input(dy), a.place_output((planes, H, W))
    (got,) = twice(a, [dx], lambda: L.tgsr_bilinear_bwd(gr.ptr, planes, H, W, OH, OW, dx.ptr, _stream()))
    assert rel(got, x64.grad[0]) < 3e-5


def test_leaky_relu_forward_and_backward():
    """n = 1000: no multiple of the 256-thread workgroup.  x > 0 passes unchanged (the same bits); x <= 0 is one fp32 product with 0.2f."""
    _M, L = _lib()
    n = 1000
    x, g = _rand(n), _rand(n, seed=1)
    a = Arena(DEV)
    xr, out = a.place_input(x), a.place_output((n,))
    (y,) = twice(a, [out], lambda: L.tgsr_leaky_relu(xr.ptr, None, out.ptr, n, _stream()))
    assert same_bits(y[x > 0], x[x > 0])
    close(y, F.leaky_relu(x.double(), 0.2), 0.0, 2e-7, "forward")
    a = Arena(DEV)
    gr, yr, out = a.place_input(g), a.place_input(y), a.place_output((n,))
    (dx,) = twice(a, [out], lambda: L.tgsr_leaky_relu(gr.ptr, yr.ptr, out.ptr, n, _stream()))
    close(dx, g.double() * torch.where(x > 0, 1.0, 0.2).double(), 0.0, 2e-7, "backward")
    a = Arena(DEV)
    xr, out = a.place_input(x), a.place_output((n,), written=False)
    assert L.tgsr_leaky_relu(None, None, out.ptr, n, _stream()) == E and L.tgsr_leaky_relu(xr.ptr, None, None, n, _stream()) == E
    assert L.tgsr_leaky_relu(xr.ptr, None, out.ptr, 0, _stream()) == E
    a.check()
