"""GPU: the fp32 inference convolutions held to their C ABI contract, called directly through ctypes.

    tgsr_conv3x3_fwd            tgsr_upconv3x3_glu_fwd        tgsr_upwino_glu_fwd / tgsr_upwino_fwd     tgsr_upwino4_fwd
    tgsr_wino_conv3x3_fwd / _stats_fwd      tgsr_wino4_conv3x3_fwd / _stats_fwd      tgsr_wino4_wide_conv3x3_fwd / _stats_fwd
    tgsr_conv_to3_fwd (the scalar form and the 5x5 MFMA form: tests/test_hip_head_finish.py holds the streaming forms)
    and the packs that feed them

tests/test_hip_parity.py reaches these kernels through tgsr_amd.ops / custom_ops only: dense operands from the caching allocator,
finite prefill, torch CPU fp32 as the reference of most forms, refusals raised by the Python wrappers.  Here every operand of a
call lives in a guarded arena (tests/arena.py): x a slice of a wider buffer (NaN pattern between the samples, an odd pad where the
form permits one), out / residual written into / read from wider buffers, the packed filter produced by its pack kernel into
exactly tgsr_packed_*_elems floats, stat_partial exactly Cout x nslots x 2 floats.  After the call the guard bands, gaps and inputs
hold their bits, every output word is written and finite, a second call gives the same bits, and the values are within the
project's caps of the same operation in fp64 on the CPU (F.conv2d on the repeat_interleave'd input for the up forms, the affine,
GLU with torch.sigmoid).

TABLE has one row per (entry point, kernel instance) with the dispatch condition in words; a test asserts from the library's own
planners that its case reaches the instance the row names - tgsr_conv3x3_form_plan, the one place the fp32 forward launches are
planned (csrc/tgsr_conv_plan.h: the function the launchers call), and tgsr_conv_to3_plan for the image heads.  Shapes are the
smallest that reach the instance with a ragged last tile in both directions and, where the tile-count thresholds leave room, two
tile rows and two tile columns.

Besides the caps every convolution carries the ratio bound of tests/test_hip_parity_margin.py: its mean distance from fp64 against
the distance of torch's CPU fp32 evaluation of the same operation from the same fp64 (R_DIRECT / R_F22 / R_F44 below).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from arena import GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA = 0.5

# mean |kernel - f64| / mean |torch CPU fp32 of the same operation - f64| over a case's output: 1.5 x the largest measured ratio of
# the group, rounded up to one decimal (the reduction order differs from torch's, so the ratio moves with the shape)
R_DIRECT = 1.8          # tgsr_conv3x3_fwd (23 cases: 0.95 .. 1.19; 0.95 .. 1.01 at Cin = 3, 1.14 .. 1.19 at Cin = 20 - the fp32 MFMA is one fma
                        # chain over taps and channels, torch's CPU convolution a blocked sum), tgsr_upconv3x3_glu_fwd (2 cases: 0.81, 0.85:
                        # 4 Cin products per output instead of 9 Cin).  Measured on the MI355X, as the two below.
R_F22 = 2.0             # tgsr_wino_conv3x3_fwd / _stats_fwd (7 cases: 0.88 .. 1.28, largest at one 4-channel stage), tgsr_upwino_glu_fwd /
                        # tgsr_upwino_fwd (4 cases: 0.87 .. 1.15)
R_F44 = 6.7             # tgsr_wino4_conv3x3_fwd / _stats_fwd (4 cases: 2.20 .. 3.24), tgsr_wino4_wide_* (6 cases: 2.17 .. 2.76),
                        # tgsr_upwino4_fwd (4 cases: 3.68 .. 4.45; largest |err| 2.4e-5 against the cap of 1e-4): the transforms hold 4, 5, 8
                        # and 1/24 - F(4x4)'s price for a quarter of the multiplies (include/tgsr_hip.h)

DIRECT, UPCONV, UPWINO, UPWINO4, WINO, WINO4, WIDE, TO3 = (
    "tgsr_conv3x3_fwd", "tgsr_upconv3x3_glu_fwd", "tgsr_upwino_glu_fwd / tgsr_upwino_fwd", "tgsr_upwino4_fwd",
    "tgsr_wino_conv3x3_fwd / _stats_fwd", "tgsr_wino4_conv3x3_fwd / _stats_fwd", "tgsr_wino4_wide_conv3x3_fwd / _stats_fwd",
    "tgsr_conv_to3_fwd")
CONVS = (DIRECT, UPCONV, UPWINO, UPWINO4, WINO, WINO4, WIDE)
GROUP = {DIRECT: "direct", UPCONV: "direct", WINO: "f22", UPWINO: "f22", WINO4: "f44", WIDE: "f44", UPWINO4: "f44"}


# ----------------------------------------------------------------------------------------------------------------------------
# The instance table.  Convolution cases: B, Cin, Cout, H, W (pre-upsample sizes), glu, up, aff (scale / shift given; else both NULL),
# res (a residual), stats (the *_stats_fwd entry point); xextra / oextra / rextra = channels of the wider buffers x is a slice of /
# out is written into / the residual is read from, xpad / opad = further floats on the batch stride (odd where the form permits);
# multi = at least two tile rows and two tile columns.  conv_to3 cases: + K, act, addend, and `skew` = words the named operands are
# moved off their 16-byte alignment.
# ----------------------------------------------------------------------------------------------------------------------------
def _c(B, Cin, Cout, H, W, glu=0, up=0, aff=True, res=False, stats=False, xextra=8, xpad=0, oextra=4, opad=0, rextra=2, multi=True):
    return dict(B=B, Cin=Cin, Cout=Cout, H=H, W=W, glu=glu, up=up, aff=aff, res=res, stats=stats, xextra=xextra, xpad=xpad,
                oextra=oextra, opad=opad, rextra=rextra, multi=multi)


def _t(B, Cin, H, W, K, act, addend=True, xextra=2, xpad=0, skew=None, multi=True):
    return dict(B=B, Cin=Cin, H=H, W=W, K=K, act=act, addend=bool(addend and act), xextra=xextra, xpad=xpad, skew=skew or {},
                multi=multi)


_D = "conv3x3_mfma_kernel<%s,4>"      # <NOB, GLU, UP, R, 4>
_S = "conv_to3_kernel<%s>"            # <K, ACT, VEC4 = false, TH, KS>
_P0 = "first pass: the first candidate with >= 512 tiles is "
_P1 = "second pass (the first found nothing ahead of its last candidate): the first candidate with >= 256 tiles is "
_FT = "neither pass finds a candidate (none reaches 256 tiles): the smallest tile, "
TABLE = [
    # entry point, kernel instance, dispatch condition (tgsr_conv3x3_fwd_plan), case
    (DIRECT, _D % "1,false,false,4", "Cout % 64 != 0: nob 1; " + _P1 + "(1, 16 rows)", _c(1, 20, 96, 17, 1345, res=True, xpad=3, opad=1)),
    (DIRECT, _D % "1,false,false,2", "Cout % 64 == 0; " + _P1 + "(1, 8 rows)", _c(2, 20, 128, 9, 481, aff=False, xpad=1, opad=3)),
    (DIRECT, _D % "1,false,false,1", _FT + "(1, 4 rows)", _c(1, 20, 96, 5, 33, xpad=1, opad=1, res=True)),
    (DIRECT, _D % "1,false,true,4", "upsample; Cout % 64 != 0; " + _P1 + "(1, 16 rows)", _c(1, 20, 96, 9, 673, up=1, aff=False, xpad=1)),
    (DIRECT, _D % "1,false,true,2", "upsample; " + _P1 + "(1, 8 rows)", _c(2, 20, 128, 61, 17, up=1, res=True, opad=1)),
    (DIRECT, _D % "1,false,true,1", "upsample; " + _FT + "(1, 4 rows)", _c(1, 3, 96, 3, 17, up=1, xpad=1, opad=1)),
    (DIRECT, _D % "1,true,false,4", "GLU, Cout % 128 != 0: nob 1; " + _P1 + "(1, 16 rows)", _c(1, 3, 192, 17, 1345, glu=1, xpad=1, opad=1)),
    (DIRECT, _D % "1,true,false,4", "GLU, Cout % 128 == 0; " + _P1 + "(1, 16 rows), behind both 2-block candidates (H = 1: one tile row)",
     _c(2, 20, 128, 1, 2051, glu=1, aff=False, xpad=1, multi=False)),
    (DIRECT, _D % "1,true,false,2", "GLU; " + _P1 + "(1, 8 rows)", _c(2, 20, 128, 9, 993, glu=1, aff=False, opad=1)),
    (DIRECT, _D % "1,true,false,1", "GLU; " + _FT + "(1, 4 rows)", _c(1, 20, 128, 5, 33, glu=1, xpad=3, opad=3)),
    (DIRECT, _D % "1,true,true,4", "GLU, upsample, Cout % 128 != 0; " + _P1 + "(1, 16 rows)", _c(1, 3, 192, 9, 673, glu=1, up=1, opad=1)),
    (DIRECT, _D % "1,true,true,2", "GLU, upsample; " + _P1 + "(1, 8 rows)", _c(3, 20, 192, 57, 17, glu=1, up=1, aff=False, xpad=1)),
    (DIRECT, _D % "1,true,true,1", "GLU, upsample; " + _FT + "(1, 4 rows)", _c(1, 20, 128, 3, 17, glu=1, up=1, xpad=1, opad=1)),
    (DIRECT, _D % "2,false,false,4", "Cout % 64 == 0: nob 2; " + _P0 + "(2, 16 rows)", _c(3, 3, 192, 17, 897, xpad=1, opad=1)),
    (DIRECT, _D % "2,false,false,2", _P0 + "(2, 8 rows)", _c(2, 3, 128, 9, 2017, res=True, aff=False, xpad=1, opad=1)),
    (DIRECT, _D % "2,false,false,1", _P1 + "(2, 4 rows)", _c(3, 20, 192, 57, 33, xpad=1, res=True)),
    (DIRECT, _D % "2,false,true,4", "upsample; " + _P0 + "(2, 16 rows)", _c(3, 3, 192, 9, 449, up=1, aff=False, xpad=1, opad=1)),
    (DIRECT, _D % "2,false,true,2", "upsample; " + _P0 + "(2, 8 rows)", _c(2, 3, 128, 5, 1009, up=1, xpad=1)),
    (DIRECT, _D % "2,false,true,1", "upsample; " + _P1 + "(2, 4 rows)", _c(2, 20, 128, 63, 17, up=1, aff=False, opad=1)),
    (DIRECT, "conv3x3_mfma_kernel<2,true,*,4,4>", "not instantiated: 2 blocks x GLU = 4 accumulator blocks take rows <= 8 "
     "(dispatch_r: NCB <= 2)", None),
    (DIRECT, _D % "2,true,false,2", "GLU, Cout % 128 == 0: nob 2; " + _P0 + "(2, 8 rows)", _c(3, 3, 128, 17, 1793, glu=1, xpad=1, opad=1)),
    (DIRECT, _D % "2,true,false,1", "GLU; " + _P1 + "(2, 4 rows)", _c(2, 20, 128, 5, 2017, glu=1, aff=False, xpad=1)),
    (DIRECT, _D % "2,true,true,2", "GLU, upsample; " + _P0 + "(2, 8 rows)", _c(2, 3, 128, 5, 2033, glu=1, up=1, aff=False, opad=1)),
    (DIRECT, _D % "2,true,true,1", "GLU, upsample; " + _P1 + "(2, 4 rows)", _c(3, 20, 128, 57, 33, glu=1, up=1, xpad=1, opad=1)),
    # one instance each: 4 source rows x 32 source columns per workgroup
    (UPCONV, "upconv_glu_mfma_kernel", "always", _c(2, 20, 128, 5, 37, glu=1, up=1, xpad=1, opad=2)),
    (UPCONV, "upconv_glu_mfma_kernel", "... three channel groups, one sample, Cin = 3, no affine", _c(1, 3, 192, 7, 33, glu=1, up=1, aff=False, xpad=3)),
    # upwino_kernel<glu>: 2 source rows x 16 source columns per workgroup
    (UPWINO, "upwino_kernel<true>", "tgsr_upwino_glu_fwd", _c(2, 12, 128, 3, 20, glu=1, up=1, opad=2)),
    (UPWINO, "upwino_kernel<true>", "... one stage, three channel groups, no affine", _c(1, 4, 192, 5, 36, glu=1, up=1, aff=False, xpad=4)),
    (UPWINO, "upwino_kernel<false>", "tgsr_upwino_fwd", _c(3, 8, 64, 3, 20, up=1, xpad=4, opad=2)),
    (UPWINO, "upwino_kernel<false>", "... no affine (the training forward's raw output)", _c(1, 24, 128, 5, 24, up=1, aff=False)),
    # upwino4_kernel<glu>: 4 x 64 outputs per workgroup
    (UPWINO4, "upwino4_kernel<true>", "glu != 0", _c(2, 8, 128, 3, 36, glu=1, up=1, opad=4)),
    (UPWINO4, "upwino4_kernel<true>", "... three channel groups, three stage pairs, no affine", _c(1, 24, 192, 5, 40, glu=1, up=1, aff=False, xpad=4)),
    (UPWINO4, "upwino4_kernel<false>", "glu == 0", _c(3, 16, 64, 3, 36, up=1, xpad=4)),
    (UPWINO4, "upwino4_kernel<false>", "... no affine", _c(1, 8, 128, 5, 44, up=1, aff=False, opad=4)),
    # wino_conv3x3_kernel<GLU, NH, STATS>: NH = 2 where Cout % 64 == 0 (4 x 32 outputs per workgroup), else 1 (8 x 32)
    (WINO, "wino_conv3x3_kernel<true,2,false>", "GLU, Cout % 64 == 0", _c(2, 12, 128, 5, 36, glu=1, opad=2)),
    (WINO, "wino_conv3x3_kernel<false,2,false>", "plain, Cout % 64 == 0, residual", _c(1, 4, 192, 7, 40, res=True, xpad=4)),
    (WINO, "wino_conv3x3_kernel<false,2,false>", "... no affine, five stages", _c(3, 20, 64, 5, 44, aff=False, opad=2)),
    (WINO, "wino_conv3x3_kernel<false,2,true>", "tgsr_wino_conv3x3_stats_fwd, Cout % 64 == 0", _c(2, 8, 128, 5, 36, aff=False, stats=True)),
    (WINO, "wino_conv3x3_kernel<true,1,false>", "GLU, Cout % 64 != 0", _c(2, 16, 96, 9, 36, glu=1, xpad=4)),
    (WINO, "wino_conv3x3_kernel<false,1,false>", "plain, Cout % 64 != 0, residual", _c(1, 24, 96, 11, 40, res=True, opad=2)),
    (WINO, "wino_conv3x3_kernel<false,1,true>", "tgsr_wino_conv3x3_stats_fwd, Cout % 64 != 0", _c(3, 4, 96, 9, 44, aff=False, stats=True, opad=2)),
    # wino4_conv3x3_kernel<GLU, STATS>: 8 x 64 outputs per workgroup
    (WINO4, "wino4_conv3x3_kernel<false,false>", "plain, residual", _c(2, 12, 128, 9, 68, res=True, opad=4)),
    (WINO4, "wino4_conv3x3_kernel<false,false>", "... one stage, no affine", _c(1, 4, 64, 11, 72, aff=False, xpad=4)),
    (WINO4, "wino4_conv3x3_kernel<true,false>", "GLU", _c(3, 8, 192, 9, 68, glu=1)),
    (WINO4, "wino4_conv3x3_kernel<false,true>", "tgsr_wino4_conv3x3_stats_fwd", _c(2, 16, 128, 11, 76, aff=False, stats=True, opad=4)),
    # wino4w_conv3x3_kernel<GLU, NB, STATS>: NB = 8 where Cout % 128 == 0, else 4; 4 x 64 outputs per workgroup
    (WIDE, "wino4w_conv3x3_kernel<false,8,false>", "plain, Cout % 128 == 0, residual", _c(2, 8, 128, 5, 68, res=True, opad=4)),
    (WIDE, "wino4w_conv3x3_kernel<true,8,false>", "GLU, Cout % 128 == 0", _c(1, 16, 128, 7, 72, glu=1, xpad=4)),
    (WIDE, "wino4w_conv3x3_kernel<false,8,true>", "tgsr_wino4_wide_conv3x3_stats_fwd, Cout % 128 == 0", _c(3, 8, 128, 5, 68, aff=False, stats=True)),
    (WIDE, "wino4w_conv3x3_kernel<false,4,false>", "plain, Cout % 128 != 0, no affine", _c(1, 24, 192, 5, 76, aff=False, opad=4)),
    (WIDE, "wino4w_conv3x3_kernel<true,4,false>", "GLU, Cout % 128 != 0", _c(2, 8, 192, 7, 68, glu=1)),
    (WIDE, "wino4w_conv3x3_kernel<false,4,true>", "tgsr_wino4_wide_conv3x3_stats_fwd, Cout % 128 != 0", _c(2, 16, 64, 7, 72, aff=False, stats=True, xpad=4, opad=4)),
    # conv_to3_kernel<K, ACT, false, TH, KS> (tgsr_conv_to3_plan: form SCALAR): TH = 16 / KS = 1 from 512 tiles of 16 x 64, TH = 8 /
    # KS = 2 from 512 tiles of 8 x 64, else TH = 4 / KS = 4
    (TO3, _S % "3,0,false,16,1", "W % 4 != 0; 512 tiles of 16 rows", _t(2, 5, 241, 1021, 3, 0, xpad=1)),
    (TO3, _S % "3,1,false,16,1", "W % 4 != 0, addend; 512 tiles of 16 rows", _t(2, 6, 241, 1021, 3, 1)),
    (TO3, _S % "5,0,false,16,1", "x_bstride % 4 != 0 at W % 4 == 0", _t(2, 3, 241, 964, 5, 0, xpad=2)),
    (TO3, _S % "5,1,false,16,1", "out off 16 bytes", _t(2, 5, 241, 964, 5, 1, skew={"out": 1})),
    (TO3, _S % "3,0,false,8,2", "x off 16 bytes; 256 tiles of 16 rows, 512 of 8", _t(2, 5, 121, 964, 3, 0, skew={"x": 1})),
    (TO3, _S % "3,1,false,8,2", "addend off 16 bytes", _t(2, 6, 121, 964, 3, 1, skew={"addend": 2})),
    (TO3, _S % "5,0,false,8,2", "W % 4 != 0", _t(2, 6, 121, 1021, 5, 0, xpad=1)),
    (TO3, _S % "5,1,false,8,2", "W % 4 != 0, no addend", _t(2, 5, 121, 1021, 5, 1, addend=False)),
    (TO3, _S % "3,0,false,4,4", "W % 4 != 0; fewer than 512 tiles of 8 rows", _t(1, 5, 9, 70, 3, 0, xpad=1)),
    (TO3, _S % "3,1,false,4,4", "x off 16 bytes, three samples", _t(3, 9, 7, 68, 3, 1, skew={"x": 3})),
    (TO3, _S % "5,0,false,4,4", "out off 16 bytes", _t(2, 3, 9, 72, 5, 0, skew={"out": 2})),
    (TO3, _S % "5,1,false,4,4", "W % 4 != 0, addend", _t(1, 20, 5, 131, 5, 1, xpad=3)),
    # conv_to3_mfma_kernel<5, ACT, 8, 8> (form MFMA): whole tiles only - W % 64 == 0 and H % 8 == 0 are part of its condition
    (TO3, "conv_to3_mfma_kernel<5,0,8,8>", "K = 5, Cin % 16 == 0, W % 64 == 0, H % 8 == 0, >= 512 tiles of 8 x 64, x aligned",
     _t(2, 16, 128, 1024, 5, 0, xextra=4, multi=False)),
    (TO3, "conv_to3_mfma_kernel<5,1,8,8>", "... with tanh and the addend, three samples", _t(3, 16, 128, 704, 5, 1, xextra=4, multi=False)),
    (TO3, "conv_to3_pipe_kernel / conv_to3_kernel<.,.,true,.,.>", "forms PIPE / VEC4: tests/test_hip_head_finish.py", None),
]


def _rows(*entries):
    return [r for r in TABLE if r[0] in entries and r[3] is not None]


def row_id(r):
    c = r[3]
    inst = r[1].replace("_kernel", "").replace("<", "_").replace(">", "").replace(",", "_")
    if r[0] == TO3:
        return "%s-%dto3-B%d-%dx%d%s" % (inst, c["Cin"], c["B"], c["H"], c["W"], "".join("-%s+%d" % kv for kv in sorted(c["skew"].items())))
    return "%s-%dto%d-B%d-%dx%d%s%s%s" % (inst, c["Cin"], c["Cout"], c["B"], c["H"], c["W"], "-aff" if c["aff"] else "",
                                         "-res" if c["res"] else "", "-stats" if c["stats"] else "")


# ----------------------------------------------------------------------------------------------------------------------------
# What a case reaches, from the library's planners
# ----------------------------------------------------------------------------------------------------------------------------
def _b(v):
    return "true" if v else "false"


def fn_of(entry, c):
    """The exported function a case calls."""
    if entry == UPWINO:
        return "tgsr_upwino_glu_fwd" if c["glu"] else "tgsr_upwino_fwd"
    if entry in (WINO, WINO4, WIDE):
        stem = {WINO: "tgsr_wino_conv3x3", WINO4: "tgsr_wino4_conv3x3", WIDE: "tgsr_wino4_wide_conv3x3"}[entry]
        return stem + ("_stats_fwd" if c["stats"] else "_fwd")
    return entry


FORM_OF = {DIRECT: "direct", UPCONV: "upconv", UPWINO: "upwino", UPWINO4: "upwino4", WINO: "wino", WINO4: "wino4", WIDE: "wino4w"}


def form_plan(L, form, kw, stats=0):
    """tgsr_conv3x3_form_plan - the function the launchers plan with - on the named arguments of a call (place_conv's or fake_conv's):
    (status, plan[TGSR_CONV_PLAN_FIELDS], prefilled with -7)."""
    from tgsr_amd import _lib as M
    buf = (ctypes.c_int * M.CONV_PLAN_FIELDS)(*([-7] * M.CONV_PLAN_FIELDS))
    rc = L.tgsr_conv3x3_form_plan(M.CONV_FORMS.index(form), kw["x"], kw["xbs"], kw["B"], kw["Cin"], kw["H"], kw["W"], kw["pack"], kw["Cout"],
                                  kw["scale"], kw["shift"], kw["res"], kw["rbs"], kw["out"], kw["obs"], kw["epilogue"], kw["upsample"],
                                  int(stats), buf)
    return rc, list(buf)


def instance_of(plan):
    """The kernel instance a plan names: its family with the template integers it takes."""
    from tgsr_amd import _lib as M
    fam = M.CONV_FAMILIES[plan[M.CONV_PLAN_FAMILY]]
    specs = [fam[i + 1] for i in range(len(fam) - 1) if fam[i] == "%"]
    return fam % tuple(t if k == "d" else _b(t) for k, t in zip(specs, plan[M.CONV_PLAN_T:]))


def fake_conv(c, skew=None):
    """place_conv's named arguments with the operands at made-up addresses, 16-byte aligned plus their skew in words: all the planner,
    which reads through no pointer, needs."""
    skew = skew or {}
    xbs, obs, rbs = conv_strides(c)

    def at(i, name):
        return (i << 24) + 4 * skew.get(name, 0)
    return dict(x=at(1, "x"), xbs=xbs, B=c["B"], Cin=c["Cin"], H=c["H"], W=c["W"], pack=at(2, "pack"), Cout=c["Cout"],
                scale=at(3, "scale") if c["aff"] else None, shift=at(4, "shift") if c["aff"] else None,
                res=at(5, "res") if c["res"] else None, rbs=rbs if c["res"] else 0, out=at(6, "out"), obs=obs, epilogue=c["glu"],
                upsample=c["up"], glu=c["glu"], stat=at(7, "stat") if c["stats"] else None)


def conv_plan(L, entry, c, kw=None):
    """(instance, tile rows, tile columns) in output pixels of a convolution case, as the library's planner states them for the call
    `kw` (default: the case's operands at aligned made-up addresses)."""
    from tgsr_amd import _lib as M
    rc, plan = form_plan(L, FORM_OF[entry], kw or fake_conv(c), c["stats"])
    assert rc == 0, "the planner refuses the case with %d" % rc
    if entry in (WINO, WINO4, WIDE):
        assert nslots_of(L, entry, c) == plan[M.CONV_PLAN_NSLOTS]
    return instance_of(plan), plan[M.CONV_PLAN_TILE_H], plan[M.CONV_PLAN_TILE_W]


def ops_forms():
    from tgsr_amd import ops
    return ops.FORMS


def nslots_of(L, entry, c):
    fn = {WINO: L.tgsr_wino_stats_nslots, WINO4: L.tgsr_wino4_stats_nslots, WIDE: L.tgsr_wino4_wide_stats_nslots}[entry]
    return fn(c["B"], c["H"], c["W"], c["Cout"])


def to3_xbs(c):
    return (c["Cin"] + c["xextra"]) * c["H"] * c["W"] + c["xpad"]


def to3_plan(L, c, x_addr, add_addr, out_addr):
    """(instance, tile rows) of a conv_to3 case whose operands lie at these addresses."""
    form, th = ctypes.c_int(), ctypes.c_int()
    rc = L.tgsr_conv_to3_plan(ctypes.c_void_p(x_addr), to3_xbs(c), c["B"], c["Cin"], c["H"], c["W"], c["K"],
                              ctypes.c_void_p(add_addr) if c["addend"] else None, ctypes.c_void_p(out_addr), ctypes.byref(form),
                              ctypes.byref(th))
    assert rc == 0
    ks = {16: 1, 8: 2, 4: 4}[th.value]
    name = {0: "conv_to3_mfma_kernel<%d,%d,8,8>" % (c["K"], c["act"]), 1: "conv_to3_pipe_kernel",
            2: "conv_to3_kernel<%d,%d,true,%d,%d>" % (c["K"], c["act"], th.value, ks),
            3: "conv_to3_kernel<%d,%d,false,%d,%d>" % (c["K"], c["act"], th.value, ks)}[form.value]
    return name, th.value


def conv_dims(c):
    co = c["Cout"] // 2 if c["glu"] else c["Cout"]
    Ho, Wo = (2 * c["H"], 2 * c["W"]) if c["up"] else (c["H"], c["W"])
    return co, Ho, Wo


def conv_strides(c):
    """(x_bstride, out_bstride, res_bstride) of a convolution case."""
    co, Ho, Wo = conv_dims(c)
    return ((c["Cin"] + c["xextra"]) * c["H"] * c["W"] + c["xpad"], (co + c["oextra"]) * Ho * Wo + c["opad"],
            (co + c["rextra"]) * Ho * Wo)


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs and references (CPU; computed once per case and shared)
# ----------------------------------------------------------------------------------------------------------------------------
def _ckey(c):
    return (c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["glu"], c["up"], c["aff"], c["res"])


@functools.lru_cache(maxsize=None)
def conv_inputs(key):
    """x ~ N(0, 1), w ~ N(0, 1) / (3 sqrt(Cin)), the affine and the residual as tests/test_hip_parity.py draws them."""
    B, Cin, Cout, H, W, glu, up, aff, res = key
    g = torch.Generator().manual_seed(B * 1000 + Cin + Cout + H + 7 * W + glu + 2 * up)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    scale = 0.5 + torch.rand(Cout, generator=g)
    shift = 0.3 * torch.randn(Cout, generator=g)
    co = Cout // 2 if glu else Cout
    s = 2 if up else 1
    r = torch.randn(B, co, s * H, s * W, generator=g) if res else None
    return x, w, (scale if aff else None), (shift if aff else None), r


def conv_reference(x, w, scale, shift, res, glu, up, dtype):
    """The operation of every convolution entry point on the CPU in `dtype`."""
    x = x.to(dtype)
    xi = x.repeat_interleave(2, 2).repeat_interleave(2, 3) if up else x
    y = F.conv2d(xi, w.to(dtype), None, 1, 1)
    if scale is not None:
        y = y * scale.to(dtype)[None, :, None, None] + shift.to(dtype)[None, :, None, None]
    if glu:
        co = y.shape[1] // 2
        y = y[:, :co] * torch.sigmoid(y[:, co:])
    return y + res.to(dtype) if res is not None else y


@functools.lru_cache(maxsize=None)
def conv_refs(key):
    x, w, scale, shift, r = conv_inputs(key)
    return (conv_reference(x, w, scale, shift, r, key[5], key[6], torch.float64),
            conv_reference(x, w, scale, shift, r, key[5], key[6], torch.float32))


def conv_tol(entry):
    """(atol, rtol) of an entry point: 2e-5 direct and sub-pixel, 3e-5 F(2x2); the F(4x4) forms: max |err| < 1e-4, no relative part."""
    return {"direct": (2e-5, 2e-5), "f22": (3e-5, 3e-5), "f44": (1e-4, 0.0)}[GROUP[entry]]


def _tkey(c):
    return (c["B"], c["Cin"], c["H"], c["W"], c["K"], c["act"], c["addend"])


@functools.lru_cache(maxsize=None)
def to3_inputs(key):
    B, Cin, H, W, K, act, addend = key
    g = torch.Generator().manual_seed(1000 * K + 7 * H + W + Cin + act)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(3, Cin, K, K, generator=g) / (K * Cin ** 0.5)
    add = torch.randn(B, 3, H, W, generator=g) if addend else None
    return x, w, add


def to3_reference(x, w, add, act, dtype=torch.float64):
    y = F.conv2d(x.to(dtype), w.to(dtype), None, 1, w.shape[2] // 2)
    if act:
        y = torch.tanh(y)
        y = y + ALPHA * add.to(dtype) if add is not None else y
    return y


@functools.lru_cache(maxsize=None)
def to3_refs(key):
    x, w, add = to3_inputs(key)
    return to3_reference(x, w, add, key[5])


TO3_TOL = 2e-5            # atol = rtol of tests/test_hip_parity.py::test_conv_to3


def close(got, ref, atol, rtol, what=""):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err >= atol + rtol * ref.abs() if rtol == 0.0 else err > atol + rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d of %d values beyond atol %.3g rtol %.3g, worst |err| %.3g at |ref| %.3g" % (
        what, int(bad.sum()), bad.numel(), atol, rtol, float(err.max()), float(ref.abs().flatten()[int(err.argmax())]))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------------------------------------------------------
# The packs: every pack kernel runs into an arena output of exactly tgsr_packed_*_elems floats
# ----------------------------------------------------------------------------------------------------------------------------
PACKS = {   # name -> (elems function, its extra arguments after (Cout, Cin), the pack's extra arguments after (Cout, Cin))
    "tgsr_pack_conv_weight": ("tgsr_packed_weight_elems", (3,), (3,)),
    "tgsr_pack_conv_weight_dgrad": ("tgsr_packed_weight_elems", (3,), (3,)),
    "tgsr_pack_upconv_weight": ("tgsr_packed_upconv_weight_elems", (), ()),
    "tgsr_pack_upwino_weight": ("tgsr_packed_upwino_weight_elems", (), None),          # None: (glu,)
    "tgsr_pack_upwino4_weight": ("tgsr_packed_upwino4_weight_elems", (), None),
    "tgsr_pack_wino_weight": ("tgsr_packed_wino_weight_elems", (), None),
    "tgsr_pack_wino_weight_dgrad": ("tgsr_packed_wino_weight_elems", (), ()),
    "tgsr_pack_wino4_weight": ("tgsr_packed_wino4_weight_elems", (), None),
    "tgsr_pack_wino4_weight_dgrad": ("tgsr_packed_wino4_weight_elems", (), ()),
    "tgsr_pack_wino4_wide_weight": ("tgsr_packed_wino4_weight_elems", (), None),
    "tgsr_pack_wino4_wide_weight_dgrad": ("tgsr_packed_wino4_weight_elems", (), ()),
}
PACK_OF = {DIRECT: "tgsr_pack_conv_weight", UPCONV: "tgsr_pack_upconv_weight", UPWINO: "tgsr_pack_upwino_weight",
           UPWINO4: "tgsr_pack_upwino4_weight", WINO: "tgsr_pack_wino_weight", WINO4: "tgsr_pack_wino4_weight",
           WIDE: "tgsr_pack_wino4_wide_weight"}


def pack_elems(L, name, Cout, Cin):
    elems, eargs, _ = PACKS[name]
    return int(getattr(L, elems)(Cout, Cin, *eargs))


def run_pack(L, name, w, Cout, Cin, glu=0):
    """The pack of `w` on the device, in an arena of its own: every word written and finite, nothing written past it."""
    n = pack_elems(L, name, Cout, Cin)
    extra = PACKS[name][2]
    extra = (int(glu),) if extra is None else extra
    a = Arena(DEV)
    wr, pk = a.place_input(w), a.place_output((n,))
    assert getattr(L, name)(wr.ptr, pk.ptr, Cout, Cin, *extra, _stream()) == 0
    a.check()
    return pk.read()


# ----------------------------------------------------------------------------------------------------------------------------
# Calling an entry point: named arguments in the order of its C signature
# ----------------------------------------------------------------------------------------------------------------------------
_UP = "x xbs B Cin H W pack Cout scale shift out obs"
_EPI = "x xbs B Cin H W pack Cout scale shift res rbs out obs epilogue"
_ST = "x xbs B Cin H W pack Cout out obs stat"
ORDER = {
    "tgsr_conv3x3_fwd": _EPI + " upsample", "tgsr_upconv3x3_glu_fwd": _UP, "tgsr_upwino_glu_fwd": _UP, "tgsr_upwino_fwd": _UP,
    "tgsr_upwino4_fwd": _UP + " glu", "tgsr_wino_conv3x3_fwd": _EPI, "tgsr_wino4_conv3x3_fwd": _EPI,
    "tgsr_wino4_wide_conv3x3_fwd": _EPI, "tgsr_wino_conv3x3_stats_fwd": _ST, "tgsr_wino4_conv3x3_stats_fwd": _ST,
    "tgsr_wino4_wide_conv3x3_stats_fwd": _ST, "tgsr_conv_to3_fwd": "x xbs B Cin H W w K act addend alpha out",
}


def call(L, fn, kw):
    return getattr(L, fn)(*[kw[k] for k in ORDER[fn].split()], _stream())


def _p(r):
    return r.ptr if r is not None else None


def place_conv(L, entry, c, pack, skew=None, written=True, stat_rows=None):
    """Every operand of a convolution case in one arena; returns (arena, regions, the named arguments of the call)."""
    skew = skew or {}
    B, Cin, Cout, H, W = c["B"], c["Cin"], c["Cout"], c["H"], c["W"]
    x, _w, scale, shift, res = conv_inputs(_ckey(c))
    co, Ho, Wo = conv_dims(c)
    xbs, obs, rbs = conv_strides(c)
    a = Arena(DEV, guard=max(GUARD, 4 * Wo + 4096))
    r = {"x": a.place_input(x, bstride=xbs, skew=skew.get("x", 0)), "pack": a.place_input(pack, skew=skew.get("pack", 0)),
         "scale": a.place_input(scale) if scale is not None else None, "shift": a.place_input(shift) if shift is not None else None,
         "res": a.place_input(res, bstride=rbs, skew=skew.get("res", 0)) if res is not None else None,
         "out": a.place_output((B, co, Ho, Wo), bstride=obs, skew=skew.get("out", 0), written=written), "stat": None}
    if c["stats"]:
        r["stat"] = a.place_output((Cout, stat_rows or nslots_of(L, entry, c), 2), written=written)
    kw = dict(x=r["x"].ptr, xbs=xbs, B=B, Cin=Cin, H=H, W=W, pack=r["pack"].ptr, Cout=Cout, scale=_p(r["scale"]), shift=_p(r["shift"]),
              res=_p(r["res"]), rbs=rbs if res is not None else 0, out=r["out"].ptr, obs=obs, epilogue=c["glu"], upsample=c["up"],
              glu=c["glu"], stat=_p(r["stat"]))
    return a, r, kw


def place_to3(c, skew=None, written=True):
    skew = dict(c["skew"], **(skew or {}))
    x, w, add = to3_inputs(_tkey(c))
    a = Arena(DEV, guard=max(GUARD, 8 * c["W"] + 4096))
    r = {"x": a.place_input(x, bstride=to3_xbs(c), skew=skew.get("x", 0)), "w": a.place_input(w),
         "addend": a.place_input(add, skew=skew.get("addend", 0)) if add is not None else None,
         "out": a.place_output((c["B"], 3, c["H"], c["W"]), skew=skew.get("out", 0), written=written)}
    kw = dict(x=r["x"].ptr, xbs=to3_xbs(c), B=c["B"], Cin=c["Cin"], H=c["H"], W=c["W"], w=r["w"].ptr, K=c["K"], act=c["act"],
              addend=_p(r["addend"]), alpha=ALPHA, out=r["out"].ptr)
    return a, r, kw


def ragged(c, rows, cols):
    """The last tile is short in both directions (and, for a `multi` case, there are two tile rows and two tile columns)."""
    _, Ho, Wo = conv_dims(c) if "Cout" in c else (0, c["H"], c["W"])
    ok = Ho % rows != 0 and Wo % cols != 0
    return ok and (not c["multi"] or (Ho > rows and Wo > cols))


# ----------------------------------------------------------------------------------------------------------------------------
# 1: every convolution entry point and instance
# ----------------------------------------------------------------------------------------------------------------------------
def check_statistics(raw, stat):
    """Per channel the slots added in fp64 equal the fp64 sums over the kernel's own raw output (the bounds of
    tests/test_hip_parity.py::test_winograd4_training_forms)."""
    s, r = stat.double().sum(1), raw.double()
    torch.testing.assert_close(s[:, 0], r.sum((0, 2, 3)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(s[:, 1], (r * r).sum((0, 2, 3)), rtol=1e-5, atol=0.0)


@pytest.mark.parametrize("row", _rows(*CONVS), ids=row_id)
def test_convolution_entry_points(row):
    entry, instance, _cond, c = row
    M, L = _lib()
    fn = fn_of(entry, c)
    reached, rows, cols = conv_plan(L, entry, c)
    assert reached == instance, "the case reaches %s" % reached
    assert ragged(c, rows, cols) or not c["multi"], "the last tile is not short in both directions"
    _x, w, _scale, _shift, _res = conv_inputs(_ckey(c))
    pack = run_pack(L, PACK_OF[entry], w, c["Cout"], c["Cin"], c["glu"])
    a, r, kw = place_conv(L, entry, c, pack)
    assert call(L, fn, kw) == M.OK
    a.check()
    got, stat = r["out"].read(), (r["stat"].read() if c["stats"] else None)
    a.rearm()
    assert call(L, fn, kw) == M.OK
    a.check()
    assert same_bits(got, r["out"].read()), "two calls on the same operands differ"
    if c["stats"]:
        assert same_bits(stat, r["stat"].read())
        check_statistics(got, stat)
    ref64, ref32 = conv_refs(_ckey(c))
    own = float((got.double() - ref64).abs().mean())
    cpu = float((ref32.double() - ref64).abs().mean())
    print("INFER_RATIO %s %s own %.4g cpu %.4g ratio %.3f max|err| %.4g" % (
        GROUP[entry], row_id(row), own, cpu, own / cpu, float((got.double() - ref64).abs().max())))
    atol, rtol = conv_tol(entry)
    close(got, ref64, atol, rtol, "out")
    R = {"direct": R_DIRECT, "f22": R_F22, "f44": R_F44}[GROUP[entry]]
    assert own <= R * cpu, "mean |kernel - f64| = %.3g is %.2f x the CPU fp32 result's %.3g (bound %.1f)" % (own, own / cpu, cpu, R)


# ----------------------------------------------------------------------------------------------------------------------------
# 2: the identities the header states, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in _rows(WINO, WINO4, WIDE) if r[3]["stats"]], ids=row_id)
def test_stats_forward_raw_output_equals_the_plain_forward_without_affine(row):
    entry, _instance, _cond, c = row
    M, L = _lib()
    w = conv_inputs(_ckey(c))[1]
    pack = run_pack(L, PACK_OF[entry], w, c["Cout"], c["Cin"], 0)
    a, r, kw = place_conv(L, entry, c, pack)
    assert call(L, fn_of(entry, c), kw) == M.OK
    a.check()
    plain = dict(c, stats=False)
    b, rb, kwb = place_conv(L, entry, plain, pack)
    assert kwb["scale"] is None and kwb["shift"] is None and kwb["res"] is None
    assert call(L, fn_of(entry, plain), kwb) == M.OK
    b.check()
    assert same_bits(r["out"].read(), rb["out"].read())


@pytest.mark.parametrize("row", [r for r in _rows(WIDE) if not r[3]["stats"]], ids=row_id)
def test_wide_form_equals_wino4_where_cin_is_a_multiple_of_8(row):
    _entry, _instance, _cond, c = row
    M, L = _lib()
    assert c["Cin"] % 8 == 0
    w = conv_inputs(_ckey(c))[1]
    outs = []
    for entry in (WIDE, WINO4):
        pack = run_pack(L, PACK_OF[entry], w, c["Cout"], c["Cin"], c["glu"])
        a, r, kw = place_conv(L, entry, c, pack)
        assert call(L, fn_of(entry, c), kw) == M.OK
        a.check()
        outs.append(r["out"].read())
    assert same_bits(outs[0], outs[1])


SCALAR_BY = [("skew_x", {"x": 1}, 0), ("skew_out", {"out": 1}, 0), ("skew_addend", {"addend": 1}, 0), ("x_bstride", {}, 2)]


@pytest.mark.parametrize("K,act", [(3, 0), (3, 1), (5, 0), (5, 1)], ids=lambda v: str(v))
def test_conv_to3_scalar_form_equals_the_vec4_form_bit_for_bit(K, act):
    """W % 4 == 0: the aligned call takes the 16-byte copy form (tgsr_conv_to3_set_pipe(0): VEC4 itself), the same values off their
    alignment the scalar form; W % 4 != 0 has no vec4 form to compare with and is held to fp64 by the table's cases."""
    M, L = _lib()
    base = _t(2, 5, 11, 72, K, act)
    was = L.tgsr_conv_to3_set_pipe(0)
    try:
        outs = {}
        for tag, skew, xpad in [("vec4", {}, 0)] + [s for s in SCALAR_BY if act or s[0] != "skew_addend"]:
            c = dict(base, xpad=xpad)
            a, r, kw = place_to3(c, skew=skew)
            name, _th = to3_plan(L, c, r["x"].address, r["addend"].address if r["addend"] else 0, r["out"].address)
            assert name == "conv_to3_kernel<%d,%d,%s,4,4>" % (K, act, _b(tag == "vec4")), (tag, name)
            assert call(L, "tgsr_conv_to3_fwd", kw) == M.OK
            a.check()
            outs[tag] = r["out"].read()
    finally:
        L.tgsr_conv_to3_set_pipe(was)
    for tag, got in outs.items():
        assert same_bits(got, outs["vec4"]), tag
    close(outs["vec4"], to3_refs(_tkey(base)), TO3_TOL, TO3_TOL, "out")


# ----------------------------------------------------------------------------------------------------------------------------
# 3: the image heads' scalar and MFMA forms
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", _rows(TO3), ids=row_id)
def test_conv_to3_entry_point(row):
    _entry, instance, _cond, c = row
    M, L = _lib()
    a, r, kw = place_to3(c)
    name, th = to3_plan(L, c, r["x"].address, r["addend"].address if r["addend"] else 0, r["out"].address)
    assert name == instance, "the case reaches %s" % name
    assert ragged(c, th, 64) or not c["multi"]
    assert call(L, "tgsr_conv_to3_fwd", kw) == M.OK
    a.check()
    got = r["out"].read()
    a.rearm()
    assert call(L, "tgsr_conv_to3_fwd", kw) == M.OK
    a.check()
    assert same_bits(got, r["out"].read())
    close(got, to3_refs(_tkey(c)), TO3_TOL, TO3_TOL, "out")


# ----------------------------------------------------------------------------------------------------------------------------
# 4: the packs
# ----------------------------------------------------------------------------------------------------------------------------
def _w(Cout, Cin, seed=0):
    g = torch.Generator().manual_seed(Cout + 3 * Cin + seed)
    return torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)


@pytest.mark.parametrize("name,glu", [(n, g) for n, v in PACKS.items() if "dgrad" not in n for g in ((0, 1) if v[2] is None else (0,))],
                         ids=lambda v: str(v))
def test_pack_pads_the_channels_with_zeros(name, glu):
    """Cin = 6: the pack holds two channels of padding.  Every word is written and finite (run_pack), and the pack equals the pack
    of the same filter with two explicit zero channels, value for value - the padding is zero, not a stale value."""
    _M, L = _lib()
    Cout, Cin = 128, 6
    w = _w(Cout, Cin)
    assert pack_elems(L, name, Cout, Cin) == pack_elems(L, name, Cout, 8) > pack_elems(L, name, Cout, 4)
    got = run_pack(L, name, w, Cout, Cin, glu)
    padded = run_pack(L, name, torch.cat([w, torch.zeros(Cout, 2, 3, 3)], 1), Cout, 8, glu)
    assert torch.equal(got, padded)
    assert int((got == 0).sum()) >= got.numel() // 4 and int((got != 0).sum()) >= Cout * Cin * 4


@pytest.mark.parametrize("name", [n for n in PACKS if "dgrad" in n])
def test_dgrad_pack_equals_the_pack_of_the_transposed_flipped_filter(name):
    """w'[co][ci][ky][kx] = w[ci][co][2 - ky][2 - kx] (tgsr_pack_conv_weight_dgrad's comment): the same words as the plain pack of w'."""
    _M, L = _lib()
    Cout, Cin = 64, 6                                            # the data-gradient convolution maps Cin -> Cout channels
    wf = _w(Cin, Cout, seed=1)                                   # the forward layer's weight [Cin][Cout][3][3]
    got = run_pack(L, name, wf, Cout, Cin)
    plain = run_pack(L, name.replace("_dgrad", ""), wf.permute(1, 0, 2, 3).flip(2, 3).contiguous(), Cout, Cin, 0)
    assert same_bits(got, plain)


PACK_MODULUS = {"tgsr_pack_wino_weight": 32, "tgsr_pack_wino_weight_dgrad": 32, "tgsr_pack_upwino_weight": 64,
                "tgsr_pack_upwino4_weight": 64, "tgsr_pack_wino4_weight": 64, "tgsr_pack_wino4_weight_dgrad": 64,
                "tgsr_pack_wino4_wide_weight": 64, "tgsr_pack_wino4_wide_weight_dgrad": 64}


@pytest.mark.parametrize("name", list(PACKS))
def test_pack_refuses_and_writes_nothing(name):
    """A NULL filter or pack and a size < 1 are TGSR_EINVAL; the Winograd packs refuse a Cout their kernels have no channel group for."""
    M, L = _lib()
    Cout, Cin = 64, 4
    extra = PACKS[name][2]
    extra = (0,) if extra is None else extra
    a = Arena(DEV)
    wr, pk = a.place_input(_w(Cout, Cin)), a.place_output((pack_elems(L, name, Cout, Cin),), written=False)
    fn = getattr(L, name)
    assert fn(None, pk.ptr, Cout, Cin, *extra, _stream()) == M.EINVAL
    assert fn(wr.ptr, None, Cout, Cin, *extra, _stream()) == M.EINVAL
    assert fn(wr.ptr, pk.ptr, 0, Cin, *extra, _stream()) == M.EINVAL
    assert fn(wr.ptr, pk.ptr, Cout, 0, *extra, _stream()) == M.EINVAL
    if name in PACK_MODULUS:
        assert fn(wr.ptr, pk.ptr, PACK_MODULUS[name] // 2 * 3, Cin, *extra, _stream()) == M.EUNSUPPORTED
    a.check()


# ----------------------------------------------------------------------------------------------------------------------------
# 5: refusals - the documented code, and the outputs untouched.  Every condition is refused on the host, ahead of any launch.
# ----------------------------------------------------------------------------------------------------------------------------
E, U = -1, -2         # TGSR_EINVAL, TGSR_EUNSUPPORTED


def _r(tag, code, skew=None, kw=None, case=None, null=(), only=None):
    return dict(tag=tag, code=code, skew=skew or {}, kw=kw or {}, case=case or {}, null=null, only=only)


NULLS = [_r("null_x", E, null=("x",)), _r("null_pack", E, null=("pack",)), _r("null_out", E, null=("out",)),
         _r("no_sample", E, kw=dict(B=0))]
AFFINE = [_r("scale_without_shift", E, null=("shift",)), _r("shift_without_scale", E, null=("scale",))]
EPILOGUE = [_r("unknown_epilogue", E, kw=dict(epilogue=2)), _r("glu_with_residual", E, case=dict(res=True), kw=dict(epilogue=1))]
F22_IO = [_r("w_not_x4", U, case=dict(W=6)), _r("x_bstride_not_x4", U, case=dict(xpad=2)), _r("x_off_16_bytes", U, skew={"x": 1}),
          _r("x_8_byte_aligned_only", U, skew={"x": 2}), _r("out_off_8_bytes", U, skew={"out": 1}), _r("out_bstride_odd", U, case=dict(opad=1))]
F44_IO = [_r("w_not_x4", U, case=dict(W=6)), _r("x_bstride_not_x4", U, case=dict(xpad=2)), _r("x_off_16_bytes", U, skew={"x": 1}),
          _r("out_off_16_bytes", U, skew={"out": 2}), _r("out_bstride_not_x4", U, case=dict(opad=2))]
F22_RES = [_r("residual_off_8_bytes", U, case=dict(res=True), skew={"res": 1}),
           _r("residual_bstride_odd", U, case=dict(res=True), kw=dict(rbs_add=1))]
F44_RES = [_r("residual_off_16_bytes", U, case=dict(res=True), skew={"res": 2}),
           _r("residual_bstride_not_x4", U, case=dict(res=True), kw=dict(rbs_add=2))]
STATS = [_r("null_stat_partial", E, null=("stat",))]
# tgsr_*_stats_fwd take no scale / shift / residual / epilogue: "statistics with an affine" (the launchers' `stat && (glu || residual ||
# scale)`) cannot be asked for through the exported signatures
REFUSALS = {
    "tgsr_conv3x3_fwd": (_c(1, 4, 64, 3, 8), NULLS + AFFINE + EPILOGUE + [
        _r("cout_not_x32", U, case=dict(Cout=48)), _r("glu_cout_not_x64", U, case=dict(Cout=96, glu=1)), _r("no_channel", E, kw=dict(Cin=0))]),
    "tgsr_upconv3x3_glu_fwd": (_c(1, 4, 64, 3, 8, glu=1, up=1), NULLS + AFFINE + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("out_off_8_bytes", U, skew={"out": 1}), _r("out_bstride_odd", U, case=dict(opad=1))]),
    "tgsr_upwino_glu_fwd": (_c(1, 4, 64, 3, 8, glu=1, up=1), NULLS + AFFINE + F22_IO + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("cin_not_x4", U, case=dict(Cin=6))]),
    "tgsr_upwino_fwd": (_c(1, 4, 64, 3, 8, up=1), NULLS + AFFINE + F22_IO + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("cin_not_x4", U, case=dict(Cin=6))]),
    "tgsr_upwino4_fwd": (_c(1, 8, 64, 3, 8, glu=1, up=1), NULLS + AFFINE + F44_IO + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("cin_not_x8", U, case=dict(Cin=12)), _r("cin_not_x4", U, case=dict(Cin=6)),
        _r("upack_off_16_bytes", U, skew={"pack": 2})]),
    "tgsr_wino_conv3x3_fwd": (_c(1, 4, 64, 3, 8), NULLS + AFFINE + EPILOGUE + F22_IO + F22_RES + [
        _r("cout_not_x32", U, case=dict(Cout=48)), _r("cin_not_x4", U, case=dict(Cin=6))]),
    "tgsr_wino_conv3x3_stats_fwd": (_c(1, 4, 64, 3, 8, aff=False, stats=True), NULLS + STATS + F22_IO + [
        _r("cout_not_x32", U, case=dict(Cout=48)), _r("cin_not_x4", U, case=dict(Cin=6))]),
    "tgsr_wino4_conv3x3_fwd": (_c(1, 4, 64, 3, 8), NULLS + AFFINE + EPILOGUE + F44_IO + F44_RES + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("cin_not_x4", U, case=dict(Cin=6))]),
    "tgsr_wino4_conv3x3_stats_fwd": (_c(1, 4, 64, 3, 8, aff=False, stats=True), NULLS + STATS + F44_IO + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("cin_not_x4", U, case=dict(Cin=6))]),
    "tgsr_wino4_wide_conv3x3_fwd": (_c(1, 8, 64, 3, 8), NULLS + AFFINE + EPILOGUE + F44_IO + F44_RES + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("cin_not_x8", U, case=dict(Cin=12)), _r("upack_off_16_bytes", U, skew={"pack": 2})]),
    "tgsr_wino4_wide_conv3x3_stats_fwd": (_c(1, 8, 64, 3, 8, aff=False, stats=True), NULLS + STATS + F44_IO + [
        _r("cout_not_x64", U, case=dict(Cout=96)), _r("cin_not_x8", U, case=dict(Cin=12)), _r("upack_off_16_bytes", U, skew={"pack": 2})]),
}
ENTRY_OF = {"tgsr_conv3x3_fwd": DIRECT, "tgsr_upconv3x3_glu_fwd": UPCONV, "tgsr_upwino_glu_fwd": UPWINO, "tgsr_upwino_fwd": UPWINO,
            "tgsr_upwino4_fwd": UPWINO4, "tgsr_wino_conv3x3_fwd": WINO, "tgsr_wino_conv3x3_stats_fwd": WINO,
            "tgsr_wino4_conv3x3_fwd": WINO4, "tgsr_wino4_conv3x3_stats_fwd": WINO4, "tgsr_wino4_wide_conv3x3_fwd": WIDE,
            "tgsr_wino4_wide_conv3x3_stats_fwd": WIDE}


def _refusal_params():
    return [pytest.param(fn, rf, id="%s-%s" % (fn[5:], rf["tag"])) for fn, (_base, rfs) in REFUSALS.items() for rf in rfs]


@pytest.mark.parametrize("fn,rf", _refusal_params())
def test_convolution_entry_point_refuses_and_writes_nothing(fn, rf):
    M, L = _lib()
    base = REFUSALS[fn][0]
    entry = ENTRY_OF[fn]
    c = dict(base, xextra=2, oextra=2, rextra=2, **rf["case"])
    g = torch.Generator().manual_seed(5)
    pack = torch.randn(4096, generator=g)                       # a refused call reads no pack: any floats will do
    a, r, kw = place_conv(L, entry, c, pack, skew=rf["skew"], written=False, stat_rows=8)
    over = dict(rf["kw"])
    kw["rbs"] += over.pop("rbs_add", 0)
    kw.update(over)
    for name in rf["null"]:
        kw[name] = None
    assert fn == fn_of(entry, c)
    for name, mis in rf["skew"].items():
        assert r[name].address % 16 == 4 * mis
    assert call(L, fn, kw) == rf["code"]
    a.check()                                                    # out (and stat_partial) still hold their prefill


TO3_REFUSALS = [
    ("kernel_4", dict(K=4), {}, U), ("kernel_7", dict(K=7), {}, U), ("kernel_1", dict(K=1), {}, U),
    ("unknown_act", dict(act=2), {}, E), ("act_none_with_addend", dict(act=0), dict(keep_addend=True), E),
    ("null_x", dict(x=None), {}, E), ("null_w", dict(w=None), {}, E), ("null_out", dict(out=None), {}, E), ("no_sample", dict(B=0), {}, E),
]


@pytest.mark.parametrize("tag,over,opt,code", TO3_REFUSALS, ids=[t[0] for t in TO3_REFUSALS])
def test_conv_to3_refuses_and_writes_nothing(tag, over, opt, code):
    M, L = _lib()
    c = _t(2, 5, 6, 12, 3, 1)
    a, r, kw = place_to3(c, written=False)
    kw.update(over)
    if kw["act"] != 1 and not opt.get("keep_addend"):
        kw["addend"] = None
    assert call(L, "tgsr_conv_to3_fwd", kw) == code
    form, th = ctypes.c_int(-7), ctypes.c_int(-7)                # the planner refuses what the call refuses that it can see
    if tag.startswith("kernel") or tag in ("null_x", "null_out", "no_sample"):
        assert L.tgsr_conv_to3_plan(kw["x"], kw["xbs"], kw["B"], kw["Cin"], kw["H"], kw["W"], kw["K"], kw["addend"], kw["out"],
                                    ctypes.byref(form), ctypes.byref(th)) == code
        assert form.value == -7 and th.value == -7
    a.check()
