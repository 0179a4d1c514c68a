"""GPU: the image pyramid kernels (tgsr_amd/csrc/tgsr_io.hip) held to their C ABI contract, called directly through ctypes.

    tgsr_resize_bilinear_u8   tgsr_gaussian_blur_u8   tgsr_u8_normalize

The rest of the suite reaches them through ops.resize_bilinear_u8 / gaussian_blur_u8 / u8_normalize only: dense allocator memory,
square pyramids of sides 16 .. 256, one blur (1, 4473924, 1677722) x 3 passes, no launch past the grid cap, no refusal.  Here every
operand of a call - image, tables, tmp, out - lies in a guarded arena (tests/arena.py); tmp has exactly the byte count
include/tgsr_hip.h states.  After a call the guard bands, the inputs and the tables hold their bits, every output byte is written,
a second call gives the same bytes, and the bytes EQUAL the numpy restatement of Pillow's integer arithmetic
(oracle/tgsr_oracle_io.py, itself equal to Pillow on these cases: tests/test_io_abi_host.py).  There is no tolerance anywhere.

The kernels load and store single bytes and promise no alignment: the byte-lead cases place `in`, `tmp` and `out` 1, 2 and 3
bytes off a word (u8_normalize's `out` is float32 and stays word aligned).

TABLE has one row per (entry point, kernel instance or branch, dispatch condition copied from the launcher, case, the wrong
kernels the case is there to catch); refusals are rows with case None (test_refusals).  tests/test_io_abi_host.py checks the
table against the launches in the source, the launch arithmetic restated here (every case named for a second trip makes one,
and no other), every case against Pillow, and that each listed wrong kernel - a variant of the numpy models below - changes at
least one output byte on that row's input.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from arena import Arena
from oracle import tgsr_oracle_io as IO

pytestmark = pytest.mark.gpu
DEV = "cuda"

RESIZE, BLUR, NORM = "tgsr_resize_bilinear_u8", "tgsr_gaussian_blur_u8", "tgsr_u8_normalize"
K_H, K_V, K_COPY = "resample_kernel<0>", "resample_kernel<1>", "hipMemcpyAsync"
K_BH, K_BV, K_NORM = "box_blur_kernel<0>", "box_blur_kernel<1>", "u8_normalize_kernel"
K_BOTH, K_BLUR = K_H + " + " + K_V, K_BH + " + " + K_BV

GRID_CAP, BLOCK = 8192, 256                        # io_grid
LEADS = ((0, 0), (1, 3), (2, 2), (3, 1))           # (bytes `in` is off a word, bytes `out` is); tmp: see _tmp_lead

# the wrong kernels, as variants of the numpy models below
V_RESIZE = ("vertical_first", "no_rounding_between", "no_half", "first_ignored", "row_stride", "other_axis_bounds", "no_clip")
V_BLUR = ("wrap_border", "zero_border", "far_at_r", "no_half", "one_pass_fewer", "horizontal_both", "one_launch_early")
V_NORM = ("reciprocal", "fused")


# ----------------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------------
def _rs(name, hin, win, hout, wout, N=6, flat=False, tables="pillow", leads=False):
    """A resize case: N random planes of hin x win -> hout x wout; flat: an all-0 and an all-255 plane behind them; tables: Pillow's
    (the product's host tables) or the hand-written ones; leads: also 1, 2 and 3 bytes off a word."""
    return dict(name=name, N=N + (2 if flat else 0), hin=hin, win=win, hout=hout, wout=wout, flat=flat, tables=tables, leads=leads)


def _bl(name, H, W, params, passes=3, N=3, fill="random", pil=None, leads=False):
    """A blur case: N planes of H x W, (radius, ww, fw) x passes; pil: how Pillow says it, ("gauss" | "box", radius), or None."""
    return dict(name=name, N=N, H=H, W=W, params=tuple(int(p) for p in params), passes=passes, fill=fill, pil=pil, leads=leads)


def _nm(name, n, leads=False):
    return dict(name=name, n=n, leads=leads)


G2, G05, G5 = IO.gaussian_box_params(2.0, 3), IO.gaussian_box_params(0.5, 3), IO.gaussian_box_params(5.0, 3)
B1375, B37 = IO.box_blur_params(1.375), IO.box_blur_params(3.7)
G25_2 = IO.gaussian_box_params(2.5, 2)                      # (2, 2816175, 1348170); two passes per axis: nothing Pillow offers

RS_DOWN, RS_UP = _rs("down-37x53-16x16", 37, 53, 16, 16, flat=True, leads=True), _rs("up-5x3-13x17", 5, 3, 13, 17)
RS_H, RS_V, RS_COPY = _rs("h-7x53-7x20", 7, 53, 7, 20), _rs("v-37x9-12x9", 37, 9, 12, 9), _rs("copy-5x7", 5, 7, 5, 7)
RS_1_UP, RS_TO_1, RS_1_1 = _rs("1x1-4x3", 1, 1, 4, 3), _rs("4x3-1x1", 4, 3, 1, 1), _rs("1x1-1x1", 1, 1, 1, 1)
RS_17 = _rs("past16-1x300-1x7", 1, 300, 1, 7, N=1)
RS_HAND = _rs("hand-9x11-6x8", 9, 11, 6, 8, tables="hand")
RS_TRIP_V, RS_TRIP_H = _rs("second-trip-v-40x40-840x840", 40, 40, 840, 840, N=3), _rs("second-trip-h-700x10-700x1000", 700, 10, 700, 1000, N=3)

BL_MAIN = _bl("r2-37x53", 37, 53, G2, N=6, pil=("gauss", 2.0), leads=True)
BL_SMALL = [_bl("r2-%dx%d" % s, s[0], s[1], G2, pil=("gauss", 2.0)) for s in ((1, 1), (1, 2), (2, 1), (3, 3), (1, 64), (64, 1))]
BL_R0 = [_bl("r0-%dx%d" % s, s[0], s[1], G05, pil=("gauss", 0.5)) for s in ((3, 3), (9, 13))]
BL_R4 = [_bl("r4-%dx%d" % s, s[0], s[1], G5, pil=("gauss", 5.0)) for s in ((3, 3), (9, 13))]
BL_P1A, BL_P1B = _bl("passes1-box1.375-9x13", 9, 13, B1375, passes=1, pil=("box", 1.375)), _bl("passes1-box3.7-9x13", 9, 13, B37, passes=1,
                                                                                               pil=("box", 3.7))
BL_P2 = _bl("passes2-9x13", 9, 13, G25_2, passes=2)
BL_255, BL_0 = _bl("all255-9x13", 9, 13, G2, fill=255, pil=("gauss", 2.0)), _bl("all0-9x13", 9, 13, G2, fill=0, pil=("gauss", 2.0))
BL_TRIP = _bl("second-trip-840x840", 840, 840, G2, pil=("gauss", 2.0))

NM_1, NM_3, NM_256, NM_TRIP = _nm("n1", 1), _nm("n3", 3, leads=True), _nm("n256", 256), _nm("second-trip-n2097156", 2097156)

_ALL_BLUR = V_BLUR


def _but(variants, *without):
    return tuple(v for v in variants if v not in without)



TABLE = (
    # entry point, kernel instance / branch, dispatch condition (copied from the launcher), case (None: refused), variants caught
    [(RESIZE, K_BOTH, "doh && dov (Wout != Win, Hout != Hin): dst = tmp, then out; 37 x 53 -> 16 x 16, ksize 9 and 7; N = 8 with an "
      "all-0 and an all-255 plane; in / tmp / out 0 .. 3 bytes off a word", RS_DOWN,
      ("vertical_first", "no_rounding_between", "no_half", "first_ignored", "row_stride", "other_axis_bounds")),
     (RESIZE, K_BOTH, "doh && dov: 5 x 3 -> 13 x 17, both passes up, ksize 3", RS_UP,
      ("vertical_first", "no_rounding_between", "no_half", "first_ignored", "row_stride", "other_axis_bounds")),
     (RESIZE, K_H, "doh && !dov (Hout == Hin): dst = out; 7 x 53 -> 7 x 20; vbounds = vcoef = tmp = NULL, vk = 0", RS_H,
      ("no_half", "first_ignored", "row_stride", "other_axis_bounds")),
     (RESIZE, K_V, "!doh && dov (Wout == Win): cur = in; 37 x 9 -> 12 x 9; hbounds = hcoef = tmp = NULL, hk = 0", RS_V,
      ("no_half", "first_ignored", "row_stride", "other_axis_bounds")),
     (RESIZE, K_COPY, "!doh && !dov: 5 x 7 -> 5 x 7, every table and tmp NULL: out is a copy of in", RS_COPY, ()),
     (RESIZE, K_BOTH, "doh && dov: 1 x 1 -> 4 x 3, every tap count 1", RS_1_UP, ("row_stride",)),
     (RESIZE, K_BOTH, "doh && dov: 4 x 3 -> 1 x 1, ksize 7 and 9, one output per plane", RS_TO_1, ("no_rounding_between", "no_half")),
     (RESIZE, K_COPY, "!doh && !dov: 1 x 1 -> 1 x 1", RS_1_1, ()),
     (RESIZE, K_H, "doh && !dov: 1 x 300 -> 1 x 7, past 16 : 1: ksize 87 as the coefficient row stride; N = 1", RS_17,
      ("no_half", "first_ignored", "row_stride", "other_axis_bounds")),
     (RESIZE, K_BOTH, "doh && dov: 9 x 11 -> 6 x 8 with hand-written tables (negative taps, rows that sum to 2 x 2^22 and to below "
      "0, other values behind the tap count): `ss < 0` and `ss > 255` both hold", RS_HAND,
      ("vertical_first", "no_rounding_between", "no_half", "first_ignored", "row_stride", "other_axis_bounds", "no_clip")),
     (RESIZE, K_BOTH, "doh && dov: 40 x 40 -> 840 x 840 at N = 3: the vertical pass has 2 116 800 outputs > 8192 x 256: a second trip of "
      "its grid-stride loop (the horizontal pass, 100 800, has none)", RS_TRIP_V,
      ("vertical_first", "no_rounding_between", "no_half", "first_ignored", "row_stride", "other_axis_bounds")),
     (RESIZE, K_H, "doh && !dov: 700 x 10 -> 700 x 1000 at N = 3: 2 100 000 outputs: a second trip of the horizontal pass", RS_TRIP_H,
      ("no_half", "first_ignored", "row_stride", "other_axis_bounds")),
     (RESIZE, "no instance", "in or out NULL; N, Hin, Win, Hout or Wout < 1; doh and hbounds or hcoef NULL or hk < 1; dov and vbounds or "
      "vcoef NULL or vk < 1; doh && dov and tmp NULL; in overlapping out; doh && dov and tmp overlapping in or out: refused", None, ()),
     (BLUR, K_BLUR, "k < passes: " + K_BH + ", else " + K_BV + "; dst = ((launches - 1 - k) & 1) ? tmp : out; radius 2 = (1, 4473924, "
      "1677722), passes 3, N = 6 at 37 x 53; in / tmp / out 0 .. 3 bytes off a word", BL_MAIN, _ALL_BLUR)]
    + [(BLUR, K_BLUR, "radius 2, passes 3 at %d x %d: L <= radius + 1 on %s" % (c["H"], c["W"], "both axes" if max(c["H"], c["W"]) <= 2
                                                                             else "one axis" if min(c["H"], c["W"]) <= 2 else "neither, L = 3"),
        c, catch) for c, catch in zip(BL_SMALL, (
            ("zero_border",), _but(_ALL_BLUR, "far_at_r", "one_launch_early"), _but(_ALL_BLUR, "far_at_r"), _ALL_BLUR,
            _but(_ALL_BLUR, "one_launch_early"), _ALL_BLUR))]
    + [(BLUR, K_BLUR, "radius 0.5 = (0, 15379114, 699051): the tap loop is one tap; %d x %d" % (c["H"], c["W"]), c, _ALL_BLUR) for c in BL_R0]
    + [(BLUR, K_BLUR, "radius 5 = (4, 1694668, 762602): %d x %d%s" % (c["H"], c["W"], ", the integer radius exceeds the side" if c["H"] == 3 else ""),
        c, _but(_ALL_BLUR, "far_at_r") if c["H"] == 3 else _ALL_BLUR) for c in BL_R4]
    + [(BLUR, K_BLUR, "passes = 1, BoxBlur(1.375) = (1, 4473924, 1677722): launch 0 writes tmp, launch 1 out", BL_P1A, _ALL_BLUR),
       (BLUR, K_BLUR, "passes = 1, BoxBlur(3.7) = (3, 1997287, 1398103)", BL_P1B, _ALL_BLUR),
       (BLUR, K_BLUR, "passes = 2, gaussian_box_params(2.5, 2) = (2, 2816175, 1348170): launches 0 and 2 write tmp, 1 and 3 out", BL_P2, _ALL_BLUR),
       (BLUR, K_BLUR, "all 255 at 9 x 13: the output is the input", BL_255, ("zero_border",)),
       (BLUR, K_BLUR, "all 0 at 9 x 13: the output is the input", BL_0, ()),
       (BLUR, K_BLUR, "N = 3 at 840 x 840: 2 116 800 outputs > 8192 x 256: a second trip in each of the six launches", BL_TRIP, _ALL_BLUR),
       (BLUR, "no instance", "in, tmp or out NULL; N, H or W < 1; radius < 0; passes < 1; (2 radius + 1) ww + 2 fw > 2^24 in 64 bits; radius "
        ">= 2^23; two of in, tmp, out overlapping: refused", None, ()),
       (NORM, K_NORM, "always; n = 1", NM_1, V_NORM),
       (NORM, K_NORM, "n = 3: 0, 99, 255; in 0 .. 3 bytes off a word", NM_3, V_NORM),
       (NORM, K_NORM, "n = 256: every byte value in order", NM_256, V_NORM),
       (NORM, K_NORM, "n = 2 097 156 > 8192 x 256: a second trip", NM_TRIP, V_NORM),
       (NORM, "no instance", "in or out NULL, n < 1: refused", None, ())])


def _rows(*entries):
    return [r for r in TABLE if r[0] in entries and r[3] is not None]


def row_id(r):
    return r[0][5:] + "-" + r[3]["name"]


# ----------------------------------------------------------------------------------------------------------------------------
# The launchers' arithmetic, restated
# ----------------------------------------------------------------------------------------------------------------------------
def io_plan(n):
    """io_grid and the kernels' grid-stride loop over n outputs: blocks of 256 threads, capped at 8192; trips of the busiest thread."""
    blocks = max(1, min(-(-n // BLOCK), GRID_CAP))
    return dict(blocks=blocks, trips=-(-n // (blocks * BLOCK)))


def resize_launches(c):
    """tgsr_resize_bilinear_u8: [(instance, destination, outputs)] in launch order."""
    doh, dov = c["wout"] != c["win"], c["hout"] != c["hin"]
    out = []
    if doh:
        out.append((K_H, "tmp" if dov else "out", c["N"] * c["hin"] * c["wout"]))
    if dov:
        out.append((K_V, "out", c["N"] * c["hout"] * c["wout"]))
    if not doh and not dov:
        out.append((K_COPY, "out", c["N"] * c["hin"] * c["win"]))
    return out


def resize_branch(c):
    return " + ".join(k for k, _, _ in resize_launches(c))


def resize_tmp_bytes(c):
    """include/tgsr_hip.h: N*Hin*Wout bytes when both passes run."""
    return c["N"] * c["hin"] * c["wout"] if len(resize_launches(c)) == 2 else 0


def blur_launches(c):
    """tgsr_gaussian_blur_u8: 2 * passes launches, [(instance, destination)]: dst = ((launches - 1 - k) & 1) ? tmp : out."""
    n = 2 * c["passes"]
    return [(K_BH if k < c["passes"] else K_BV, "tmp" if (n - 1 - k) & 1 else "out") for k in range(n)]


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs, tables, references
# ----------------------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


@functools.lru_cache(maxsize=None)
def _resize_input(N, hin, win, flat):
    a = _rng(N, hin, win, 1).integers(0, 256, (N, hin, win), dtype=np.uint8)
    if flat:
        a[-2], a[-1] = 0, 255
    a.setflags(write=False)
    return a


def resize_input(c):
    return _resize_input(c["N"], c["hin"], c["win"], c["flat"])


HAND_PAD = 777777          # what lies behind the tap count of a hand-written row: nothing a right kernel reads


def hand_tables():
    """Tables Pillow would never make, for 9 x 11 -> 6 x 8: ((hbounds [8][2], hcoef [8][4], 4), (vbounds [6][2], vcoef [6][5], 5)).
    One unit of Pillow's fixed point is 2^22.  Rows with negative lobes that sum to 2^22, rows that sum to 2 x 2^22 (`ss > 255`
    wherever the pixels are bright), rows that sum to below 0 (`ss < 0`).  No sum of |tap| x 255 + 2^21 reaches 2^31."""
    h = [(0, [3 << 21, 1 << 21]), (1, [-(1 << 20), 3 << 21, -(1 << 20)]), (2, [1 << 22, 1 << 22]), (4, [1 << 21] * 4),
         (5, [-(1 << 21), -(1 << 20)]), (6, [1 << 22, -(1 << 21), 1 << 20]), (8, [1 << 20, 1 << 21, 1 << 20]), (10, [1 << 22])]
    v = [(0, [1 << 22]), (0, [1 << 21, 1 << 21, 1 << 22]), (2, [-(1 << 20), 1 << 21, 1 << 21, 1 << 21, -(1 << 20)]),
         (4, [-(1 << 22), 1 << 21]), (5, [1 << 21] * 4), (8, [1 << 22])]

    def table(rows, ksize, size):
        bounds = np.array([(f, len(t)) for f, t in rows], np.int32)
        coef = np.full((len(rows), ksize), HAND_PAD, np.int32)
        for k, (f, t) in enumerate(rows):
            assert f + len(t) <= size and len(t) <= ksize and sum(abs(x) for x in t) * 255 + (1 << 21) < 1 << 31
            coef[k, :len(t)] = t
        return bounds, coef, ksize
    return table(h, 4, 11), table(v, 5, 9)


def resize_tables(c):
    """(htab, vtab), each (bounds, taps, ksize) as the call takes them or None where the pass does not run: the product's host
    tables (tgsr_amd.datasets._resize_tables, what GpuImagePyramid uploads) or the hand-written ones."""
    if c["tables"] == "hand":
        assert (c["hin"], c["win"], c["hout"], c["wout"]) == (9, 11, 6, 8)
        return hand_tables()
    from tgsr_amd.datasets import _resize_tables
    return (_resize_tables(c["win"], c["wout"]) if c["wout"] != c["win"] else None,
            _resize_tables(c["hin"], c["hout"]) if c["hout"] != c["hin"] else None)


@functools.lru_cache(maxsize=None)
def _resize_reference(name):
    c = next(r[3] for r in _rows(RESIZE) if r[3]["name"] == name)
    a = resize_input(c)
    if c["tables"] == "hand":
        h, v = hand_tables()
        ref = IO.resize_bilinear_tables(a, h[:2], v[:2])
    else:
        ref = IO.resize_bilinear(a, c["hout"], c["wout"])
    ref = np.ascontiguousarray(ref)
    ref.setflags(write=False)
    return ref


def resize_reference(c):
    """The oracle's bytes: Pillow's arithmetic from the oracle's OWN tables, or the same formula fed with the hand-written ones."""
    return _resize_reference(c["name"])


def _gather(a0, first, j):
    """a0 [N][P][L] at index first + j along the last axis, first [P][O] -> [N][P][O] (the index clamped: a caller masks the tap)."""
    idx = np.minimum(first + j, a0.shape[-1] - 1)
    return np.take_along_axis(a0, np.broadcast_to(idx[None], (a0.shape[0],) + idx.shape), axis=-1)


def resample_model(a, tab, axis, variant="", raw_in=False, raw_out=False, stats=None):
    """resample_kernel<AXIS> in numpy, all outputs at once: a [N][H][W], tab = (bounds, taps, ksize), axis 2 (AXIS 0, along W) or 1.
    variant: no_half - the 2^21 omitted; first_ignored - every window starts at 0; row_stride - the taps of row o read at
    o * (ksize - 1); other_axis_bounds - (first, count) of the row the OTHER coordinate names (y in the horizontal pass, x in the
    vertical one; modulo the table's rows, so the model stays inside the image); no_clip - the low byte instead of the clip.
    raw_out / raw_in: the exact sums pass to the next pass unshifted and unrounded (no_rounding_between).
    stats: a dict that gains the number of outputs below 0 and above 255 in front of the clip."""
    bounds, coef, ksize = tab
    bounds, coef = np.asarray(bounds, np.int64), np.asarray(coef, np.int64)
    nout = len(bounds)
    a0 = (a if axis == 2 else np.swapaxes(a, 1, 2)).astype(np.int64)          # [N][P][L]
    P = a0.shape[1]
    taps = coef
    if variant == "row_stride":
        flat = coef.reshape(-1)
        taps = flat[np.minimum(np.arange(nout)[:, None] * (ksize - 1) + np.arange(ksize)[None, :], flat.size - 1)]
    rows = np.broadcast_to(np.arange(nout)[None, :], (P, nout))
    if variant == "other_axis_bounds":
        rows = np.broadcast_to((np.arange(P) % nout)[:, None], (P, nout))
    first, count = bounds[rows, 0], bounds[rows, 1]                             # [P][O]
    if variant == "first_ignored":
        first = np.zeros_like(first)
    ss = np.zeros((a0.shape[0], P, nout), np.int64)
    for j in range(int(count.max())):
        ss += _gather(a0, first, j) * np.where(j < count, taps[None, :, j], 0)[None]
    if raw_out:
        out = ss
    else:
        shift = 44 if raw_in else 22
        ss = (ss + (0 if variant == "no_half" else 1 << (shift - 1))) >> shift
        if stats is not None:
            stats["low"] = stats.get("low", 0) + int((ss < 0).sum())
            stats["high"] = stats.get("high", 0) + int((ss > 255).sum())
        out = ((ss & 255) if variant == "no_clip" else np.clip(ss, 0, 255)).astype(np.uint8)
    return out if axis == 2 else np.swapaxes(out, 1, 2)


def resize_model(a, htab, vtab, variant="", stats=None):
    """tgsr_resize_bilinear_u8 in numpy.  variant: vertical_first - the vertical pass runs first; no_rounding_between - the
    horizontal pass hands its exact sums on, one rounding at the end; the others are resample_model's, in every pass."""
    per_pass = variant if variant in ("no_half", "first_ignored", "row_stride", "other_axis_bounds", "no_clip") else ""
    passes = [(t, ax) for t, ax in ((htab, 2), (vtab, 1)) if t is not None]
    if variant == "vertical_first":
        passes.reverse()
    keep = variant == "no_rounding_between" and len(passes) == 2
    for k, (t, ax) in enumerate(passes):
        a = resample_model(a, t, ax, per_pass, raw_in=keep and k == 1, raw_out=keep and k == 0, stats=stats)
    return np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def _blur_input(N, H, W, fill):
    a = _rng(N, H, W, 2).integers(0, 256, (N, H, W), dtype=np.uint8) if fill == "random" else np.full((N, H, W), fill, np.uint8)
    a.setflags(write=False)
    return a


def blur_input(c):
    return _blur_input(c["N"], c["H"], c["W"], c["fill"])


@functools.lru_cache(maxsize=None)
def _blur_reference(name):
    c = next(r[3] for r in _rows(BLUR) if r[3]["name"] == name)
    ref = IO.box_blur(blur_input(c), *c["params"], c["passes"])
    ref.setflags(write=False)
    return ref


def blur_reference(c):
    return _blur_reference(c["name"])


def box_pass_model(a, r, ww, fw, axis, variant=""):
    """box_blur_kernel<AXIS> in numpy: a [N][H][W], axis 2 (AXIS 0) or 1; uint32 arithmetic.  variant: wrap_border / zero_border -
    instead of the clamp; far_at_r - the far pixels at +-r instead of +-(r + 1); no_half - the 2^23 omitted."""
    a0 = a if axis == 2 else np.swapaxes(a, 1, 2)
    L = a0.shape[-1]
    idx = np.arange(L)

    def at(q):
        if variant == "wrap_border":
            return a0[..., q % L].astype(np.uint64)
        v = a0[..., np.clip(q, 0, L - 1)].astype(np.uint64)
        return np.where((q < 0) | (q >= L), 0, v).astype(np.uint64) if variant == "zero_border" else v
    acc = np.zeros(a0.shape, np.uint64)
    for d in range(-r, r + 1):
        acc += at(idx + d)
    f = r if variant == "far_at_r" else r + 1
    bulk = (acc * np.uint64(ww) + (at(idx - f) + at(idx + f)) * np.uint64(fw)) & np.uint64(0xFFFFFFFF)
    out = (((bulk + np.uint64(0 if variant == "no_half" else 1 << 23)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.uint8)
    return out if axis == 2 else np.swapaxes(out, 1, 2)


def blur_model(a, r, ww, fw, passes, variant=""):
    """tgsr_gaussian_blur_u8 in numpy: `passes` launches along W, then as many along H.  variant: one_pass_fewer - passes - 1 per
    axis; horizontal_both - every launch along W; one_launch_early - what the last launch but one wrote (the ping-pong parity
    off by one: `out` holds it); the others are box_pass_model's."""
    axes = [2] * passes + [1] * passes
    if variant == "one_pass_fewer":
        axes = [2] * (passes - 1) + [1] * (passes - 1)
    if variant == "horizontal_both":
        axes = [2] * (2 * passes)
    if variant == "one_launch_early":
        axes = axes[:-1]
    per_pass = variant if variant in ("wrap_border", "zero_border", "far_at_r", "no_half") else ""
    for ax in axes:
        a = box_pass_model(a, r, ww, fw, ax, per_pass)
    return np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def _norm_input(n):
    if n == 1:
        a = np.array([48], np.uint8)                 # a byte at which both wrong forms of test_io_abi_host.py give other bits
    elif n == 3:
        a = np.array([0, 99, 255], np.uint8)
    elif n == 256:
        a = np.arange(256, dtype=np.uint8)
    else:
        a = _rng(n, 3).integers(0, 256, n, dtype=np.uint8)
        a[:256], a[-256:] = np.arange(256), np.arange(255, -1, -1)
    a.setflags(write=False)
    return a


def norm_input(c):
    return _norm_input(c["n"])


def norm_model(a, variant=""):
    """u8_normalize_kernel in numpy's float32: (u / 255 - 0.5) / 0.5, three correctly rounded operations.  variant: reciprocal - u
    times the rounded 1 / 255; fused - u * (2 / 255) - 1."""
    f = np.float32
    u = a.astype(np.float32)
    if variant == "reciprocal":
        return (u * (f(1.0) / f(255.0)) - f(0.5)) / f(0.5)
    if variant == "fused":
        return u * (f(2.0) / f(255.0)) - f(1.0)
    return (u / f(255.0) - f(0.5)) / f(0.5)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


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
    """The call, the arena's contract, the call again from the same state: the contract again and the same bytes in every output."""
    M, _ = _lib()
    assert call() == M.OK
    a.check()
    got = [o.read() for o in outs]
    a.rearm()
    assert call() == M.OK
    a.check()
    for g, o in zip(got, outs):
        again = o.read()
        same = torch.equal(g.view(torch.int32), again.view(torch.int32)) if g.dtype == torch.float32 else torch.equal(g, again)
        assert same, "a second call gives other bytes"
    return got


def _tmp_lead(lead_in, lead_out):
    """tmp off a word by another count than either image, wherever either image is."""
    return (lead_in + 2) % 4 if (lead_in or lead_out) else 0


def _leads(c):
    return LEADS if c["leads"] else LEADS[:1]


def _equal_bytes(got, ref, what):
    got = got.numpy()
    assert got.shape == ref.shape and got.dtype == np.uint8
    diff = got != ref
    assert not diff.any(), "%s: %d of %d bytes differ from the reference, first at %s: %d, not %d" % (
        what, int(diff.sum()), diff.size, tuple(int(i) for i in np.argwhere(diff)[0]), int(got[diff][0]), int(ref[diff][0]))


def run_resize(L, c, lead_in=0, lead_out=0):
    x, ref = resize_input(c), resize_reference(c)
    htab, vtab = resize_tables(c)
    a = Arena(DEV)
    xin = a.place_input_u8(torch.from_numpy(x.copy()), lead=lead_in)
    hb, hc = (a.place_input(torch.from_numpy(htab[0])), a.place_input(torch.from_numpy(htab[1]))) if htab else (None, None)
    vb, vc = (a.place_input(torch.from_numpy(vtab[0])), a.place_input(torch.from_numpy(vtab[1]))) if vtab else (None, None)
    nbytes = resize_tmp_bytes(c)
    tmp = a.place_ws_u8(nbytes, lead=_tmp_lead(lead_in, lead_out)) if nbytes else None
    out = a.place_output_u8(ref.shape, lead=lead_out, expect=torch.from_numpy(ref.copy()))
    assert xin.address % 4 == lead_in and out.address % 4 == lead_out and (tmp is None or tmp.address % 4 == _tmp_lead(lead_in, lead_out))
    return _twice(a, lambda: L.tgsr_resize_bilinear_u8(xin.ptr, c["N"], c["hin"], c["win"], c["hout"], c["wout"], _p(hb), _p(hc),
                                                       htab[2] if htab else 0, _p(vb), _p(vc), vtab[2] if vtab else 0, _p(tmp), out.ptr,
                                                       _stream()), [out])[0]


@pytest.mark.parametrize("row", _rows(RESIZE), ids=row_id)
def test_resize(row):
    _entry, instance, _cond, c, _catch = row
    assert instance == resize_branch(c)
    _, L = _lib()
    ref = resize_reference(c)
    assert ref.shape == (c["N"], c["hout"], c["wout"])
    if instance == K_COPY:
        assert np.array_equal(ref, resize_input(c))
    for lead_in, lead_out in _leads(c):
        _equal_bytes(run_resize(L, c, lead_in, lead_out), ref, "%s in +%d out +%d" % (c["name"], lead_in, lead_out))


def run_blur(L, c, lead_in=0, lead_out=0):
    x, ref = blur_input(c), blur_reference(c)
    r, ww, fw = c["params"]
    a = Arena(DEV)
    xin = a.place_input_u8(torch.from_numpy(x.copy()), lead=lead_in)
    tmp = a.place_ws_u8(x.size, lead=_tmp_lead(lead_in, lead_out))               # include/tgsr_hip.h: exactly N*H*W bytes
    out = a.place_output_u8(ref.shape, lead=lead_out, expect=torch.from_numpy(ref.copy()))
    assert xin.address % 4 == lead_in and out.address % 4 == lead_out and tmp.address % 4 == _tmp_lead(lead_in, lead_out)
    return _twice(a, lambda: L.tgsr_gaussian_blur_u8(xin.ptr, c["N"], c["H"], c["W"], r, ww, fw, c["passes"], tmp.ptr, out.ptr, _stream()),
                  [out])[0]


@pytest.mark.parametrize("row", _rows(BLUR), ids=row_id)
def test_blur(row):
    _entry, instance, _cond, c, _catch = row
    launches = blur_launches(c)
    assert instance == K_BLUR and launches[-1][1] == "out" and (2 * c["params"][0] + 1) * c["params"][1] + 2 * c["params"][2] <= 1 << 24
    _, L = _lib()
    ref = blur_reference(c)
    if c["fill"] != "random":
        assert np.array_equal(ref, blur_input(c)), "a flat image blurs to itself"
    for lead_in, lead_out in _leads(c):
        _equal_bytes(run_blur(L, c, lead_in, lead_out), ref, "%s in +%d out +%d" % (c["name"], lead_in, lead_out))


def run_normalize(L, x, lead_in=0):
    a = Arena(DEV)
    xin = a.place_input_u8(torch.from_numpy(x.copy()), lead=lead_in)
    out = a.place_output((x.size,))
    assert xin.address % 4 == lead_in
    return _twice(a, lambda: L.tgsr_u8_normalize(xin.ptr, out.ptr, x.size, _stream()), [out])[0].numpy()


@pytest.mark.parametrize("row", _rows(NORM), ids=row_id)
def test_normalize(row):
    c = row[3]
    _, L = _lib()
    x = norm_input(c)
    ref = IO.normalize(x)
    assert ref.dtype == np.float32
    for lead_in, _ in _leads(c):
        got = run_normalize(L, x, lead_in)
        bad = bits(got) != bits(ref)
        assert not bad.any(), "%d of %d values differ in their bits from numpy's float32 expression, first for byte %d" % (
            int(bad.sum()), bad.size, int(x[bad][0]))
    if c["n"] == 256:
        assert bits(got[0]) == bits(np.float32(-1.0)) and bits(got[255]) == bits(np.float32(1.0))
        assert bool((np.diff(got.astype(np.float64)) > 0).all()), "not strictly increasing over the byte values"


def test_normalize_then_to_uint8_gives_the_byte_back():
    """tgsr_to_uint8(tgsr_u8_normalize(b)) == b for all 256 bytes, on the device (tests/test_metrics_host.py: on the model)."""
    _, L = _lib()
    x = norm_input(NM_256)
    f = run_normalize(L, x)
    a = Arena(DEV)
    fin = a.place_input(torch.from_numpy(f.copy()))
    out = a.place_output_u8((256,), expect=torch.from_numpy(x.copy()))
    back = _twice(a, lambda: L.tgsr_to_uint8(fin.ptr, out.ptr, 256, _stream()), [out])[0]
    _equal_bytes(back, x, "to_uint8(u8_normalize(b))")


# ----------------------------------------------------------------------------------------------------------------------------
# Refusals: every one a host-side return in front of the first launch - the code, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------
REF_RS = dict(N=2, Hin=4, Win=5, Hout=3, Wout=2)          # the valid small calls the refusals start from
REF_BL = dict(N=2, H=4, W=5, radius=1, ww=4473924, fw=1677722, passes=3)
REF_NM = dict(n=40)

# the arguments in order (the stream follows): (kind, name); "img": a byte operand of `bytes` bytes, "tab": an int32 table
SPEC = {
    RESIZE: [("img", "in", 40), ("num", "N"), ("num", "Hin"), ("num", "Win"), ("num", "Hout"), ("num", "Wout"), ("tab", "hbounds"),
             ("tab", "hcoef"), ("num", "hk"), ("tab", "vbounds"), ("tab", "vcoef"), ("num", "vk"), ("img", "tmp", 16), ("img", "out", 40)],
    BLUR: [("img", "in", 40), ("num", "N"), ("num", "H"), ("num", "W"), ("num", "radius"), ("num", "ww"), ("num", "fw"), ("num", "passes"),
           ("img", "tmp", 40), ("img", "out", 40)],
    NORM: [("img", "in", 40), ("f32", "out", 40), ("num", "n")],
}
NULLS = {RESIZE: ("in", "out", "hbounds", "hcoef", "vbounds", "vcoef", "tmp"), BLUR: ("in", "tmp", "out"), NORM: ("in", "out")}
SIZES = {RESIZE: ("N", "Hin", "Win", "Hout", "Wout"), BLUR: ("N", "H", "W"), NORM: ("n",)}


def _refusal_call(L, a, entry, null=None, alias=None, **nums):
    """A call of `entry` on valid small operands - real tables, images of the 40 bytes the largest variant needs (the resize writes
    N*Hout*Wout = 12 of `out`), tmp of exactly N*Hin*Wout = 16 - with one thing wrong.  Nothing may
    be written: tmp and out are placed as outputs the call must leave alone.  null: the operand handed over as NULL; alias = (name,
    target, offset): `name` points `offset` bytes into `target`; every other keyword replaces the number of that name."""
    from tgsr_amd.datasets import _resize_tables
    base = dict({RESIZE: REF_RS, BLUR: REF_BL, NORM: REF_NM}[entry])
    tabs = {}
    if entry == RESIZE:
        hb, hc, hk = _resize_tables(base["Win"], base["Wout"])
        vb, vc, vk = _resize_tables(base["Hin"], base["Hout"])
        tabs, base["hk"], base["vk"] = dict(hbounds=hb, hcoef=hc, vbounds=vb, vcoef=vc), hk, vk
    assert all(k in base for k in nums), nums
    base.update(nums)
    held = {}
    for kind, name, *arg in SPEC[entry]:
        if kind == "img":
            held[name] = (a.place_input_u8(torch.arange(arg[0], dtype=torch.uint8)) if name == "in"
                          else a.place_output_u8((arg[0],), written=False))
        elif kind == "f32":
            held[name] = a.place_output((arg[0],), written=False)
        elif kind == "tab":
            held[name] = a.place_input(torch.from_numpy(tabs[name]))
    args = []
    for kind, name, *arg in SPEC[entry]:
        if kind == "num":
            args.append(base[name])
        elif name == null:
            args.append(None)
        elif alias is not None and alias[0] == name:
            args.append(ctypes.c_void_p(held[alias[1]].address + alias[2]))
        else:
            args.append(held[name].ptr)
    fn = getattr(L, entry)
    return lambda: fn(*args, _stream())


def refusals():
    """(name, entry point, arguments of _refusal_call).  Every one answers TGSR_EINVAL.  None of them, were it let through, would
    make a kernel read or write outside its operands or run long: the tables stay valid, the overlapping operands stay inside the
    arena, the weights that wrap 32-bit arithmetic come with radius 1 and 0."""
    out = []
    for e, names in NULLS.items():
        out += [("%s-%s-null" % (e[5:], n), e, dict(null=n)) for n in names]
    for e, names in SIZES.items():
        out += [("%s-%s-%d" % (e[5:], n, v), e, {n: v}) for n in names for v in (0, -1)]
    rs, bl = RESIZE[5:], BLUR[5:]
    out += [
        (rs + "-hk-0", RESIZE, dict(hk=0)), (rs + "-hk-negative", RESIZE, dict(hk=-1)), (rs + "-vk-0", RESIZE, dict(vk=0)),
        (rs + "-vk-negative", RESIZE, dict(vk=-1)),
        (rs + "-hbounds-null-horizontal-only", RESIZE, dict(null="hbounds", Hout=4)), (rs + "-hk-0-horizontal-only", RESIZE, dict(hk=0, Hout=4)),
        (rs + "-vcoef-null-vertical-only", RESIZE, dict(null="vcoef", Wout=5)), (rs + "-vk-0-vertical-only", RESIZE, dict(vk=0, Wout=5)),
        (rs + "-out-is-in", RESIZE, dict(alias=("out", "in", 0))), (rs + "-out-is-in-copy-branch", RESIZE, dict(alias=("out", "in", 0), Hout=4, Wout=5)),
        (rs + "-out-on-the-last-byte-of-in", RESIZE, dict(alias=("out", "in", 39))),
        (rs + "-in-on-the-last-byte-of-out", RESIZE, dict(alias=("in", "out", 11))),          # in = out + 11: out's 12th byte is in's first
        (rs + "-tmp-is-in", RESIZE, dict(alias=("tmp", "in", 0))), (rs + "-tmp-on-the-last-byte-of-in", RESIZE, dict(alias=("tmp", "in", 39))),
        (rs + "-tmp-is-out", RESIZE, dict(alias=("tmp", "out", 0))), (rs + "-tmp-on-the-last-byte-of-out", RESIZE, dict(alias=("tmp", "out", 11))),
        (rs + "-out-on-the-last-byte-of-tmp", RESIZE, dict(alias=("out", "tmp", 15))),
        (bl + "-radius-negative", BLUR, dict(radius=-1)), (bl + "-passes-0", BLUR, dict(passes=0)), (bl + "-passes-negative", BLUR, dict(passes=-1)),
        (bl + "-weights-2^24+2", BLUR, dict(fw=1677723)), (bl + "-weights-2^24+3", BLUR, dict(ww=4473925)),
        (bl + "-radius-2-with-the-weights-of-1", BLUR, dict(radius=2)),                           # 5 ww + 2 fw
        (bl + "-3ww-wraps-32-bits-to-5", BLUR, dict(ww=1431655767, fw=0)), (bl + "-2fw-wraps-32-bits-to-0", BLUR, dict(radius=0, ww=0, fw=1 << 31)),
        (bl + "-radius-2^23-without-weights", BLUR, dict(radius=1 << 23, ww=0, fw=0)),
        (bl + "-out-is-in", BLUR, dict(alias=("out", "in", 0))), (bl + "-tmp-is-in", BLUR, dict(alias=("tmp", "in", 0))),
        (bl + "-tmp-is-out", BLUR, dict(alias=("tmp", "out", 0))), (bl + "-out-on-the-last-byte-of-in", BLUR, dict(alias=("out", "in", 39))),
        (bl + "-in-on-the-last-byte-of-tmp", BLUR, dict(alias=("in", "tmp", 39))), (bl + "-tmp-on-the-last-byte-of-out", BLUR, dict(alias=("tmp", "out", 39))),
    ]
    return out


def test_refusals():
    """Every NULL the launchers test, every size below 1, a tap-row length below 1 for a pass that runs, tmp missing with both
    passes, a negative radius, no pass, weights whose sum can wrap, overlapping operands: TGSR_EINVAL, no byte written."""
    M, L = _lib()
    for name, entry, kw in refusals():
        a = Arena(DEV, guard=64)
        call = _refusal_call(L, a, entry, **kw)
        assert call() == M.EINVAL, name
        v = a.violations()
        assert not v, name + ": " + "; ".join(v)


# ----------------------------------------------------------------------------------------------------------------------------
# The wrappers of tgsr_amd/ops.py
# ----------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_what_the_kernels_would_misread():
    """ops.gaussian_blur_u8 and ops.u8_normalize on a float32 tensor used to read its bytes as pixels; all three wrappers now say
    what is wrong with a tensor of another type, of too few dimensions or empty, and with a size or a pass count below 1."""
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    from tgsr_amd.datasets import _resize_tables
    u = torch.from_numpy(resize_input(RS_UP).copy()).to(DEV)                       # [6, 5, 3] uint8
    f = u.float()
    tab = lambda i, o: tuple(torch.from_numpy(t).to(DEV) if isinstance(t, np.ndarray) else t for t in _resize_tables(i, o))  # noqa: E731
    h, v = tab(3, 17), tab(5, 13)
    for bad, what in ((f, "uint8"), (f.half(), "uint8"), (u.to(torch.int32), "uint8"), (u[0, 0], "dimension"), (u[:0], "empty")):
        with pytest.raises(TgsrError, match=what):
            ops.resize_bilinear_u8(bad, 13, 17, h, v)
        with pytest.raises(TgsrError, match=what):
            ops.gaussian_blur_u8(bad, *G2, 3)
    for bad, what in ((f, "uint8"), (u.to(torch.int8), "uint8"), (u[0, 0, 0], "dimension"), (u[:, :0], "empty")):
        with pytest.raises(TgsrError, match=what):
            ops.u8_normalize(bad)
    for oh, ow in ((0, 17), (13, 0), (-1, 17)):
        with pytest.raises(TgsrError, match="at least 1 x 1"):
            ops.resize_bilinear_u8(u, oh, ow, h, v)
    for passes in (0, -1):
        with pytest.raises(TgsrError, match="passes"):
            ops.gaussian_blur_u8(u, *G2, passes)
    with pytest.raises(TgsrError, match="EINVAL"):                                 # the entry's own refusal: weights that can wrap
        ops.gaussian_blur_u8(u, G2[0], G2[1], G2[2] + 1, 3)
    # and what they accept still gives the reference's bytes
    _equal_bytes(ops.resize_bilinear_u8(u, 13, 17, h, v).cpu(), resize_reference(RS_UP), "ops.resize_bilinear_u8")
    same = ops.resize_bilinear_u8(u, 5, 3, None, None)
    assert same.data_ptr() != u.data_ptr() and torch.equal(same, u)
    _equal_bytes(ops.gaussian_blur_u8(u, *G2, 3).cpu(), IO.box_blur(resize_input(RS_UP), *G2, 3), "ops.gaussian_blur_u8")
    one = ops.u8_normalize(u[0, 0])                                                # one dimension is enough here
    assert np.array_equal(bits(one.cpu().numpy()), bits(IO.normalize(resize_input(RS_UP)[0, 0])))
