"""GPU: the whole-image path - tile gather / stitch (tgsr_amd/csrc/tgsr_tiles.hip), the x8 self-ensemble gather / merge
(tgsr_ensemble.hip) and the image scores (tgsr_metrics.hip) - held to their C ABI contract, called directly through ctypes.

    tgsr_tile_gather   tgsr_tile_stitch   tgsr_d8_gather   tgsr_d8_merge   tgsr_sr_metrics (+ _ws_elems)   tgsr_rgb_to_y_u8

The rest of the suite reaches them through ops.* on allocator memory.  Here every device operand of a call - images, device
tables, tile batches, destinations, the fp64 workspace - lies in ONE guarded arena (tests/arena.py); host tables and the by-value
lists (src, dst, C, scale, out_u8, src_stride) are host arrays, as include/tgsr_hip.h says.  After every accepted call: the arena's
check (guard bands of 16 384 words, the gaps of a strided source, every input and device table bit-unchanged, nothing written
outside what the call owns, everything it owns written), a second call from the re-armed state (workspaces then hold a finite
constant instead of the pattern) gives the same bits, and the values are the numpy models' (tiles_model, ensemble_model,
metrics_model): gather, stitch, merge, rgb_to_y and the two SSE columns BIT-EXACT, the SSIM column by metrics_model.check_rows with
test_hip_metrics.SSIM_TOL = 1e-9 (derived there).  The arena's pattern read as a double is a finite 3e307, not a NaN: a workspace
element read before it is written shows as a wildly wrong sum, one never written as the bit comparison.

A destination is placed with what it held before (finite floats, random bytes) and a mask of the elements the call owns: a hole no
tile owns, the rectangle of a window whose DEVICE table row fails the kernels' own check, keep their bits.  Such a row is a
documented input: the kernels test the six numbers and return before they form any address from them.

TABLE has one row per (entry point, kernel instance or branch, dispatch condition copied from the launcher, case, the wrong kernels
the case is there to catch); refusals are rows with case None (test_refusals), a branch no test can afford is a row whose case says
`unreachable`.  tests/test_upscale_abi_host.py checks the table against the three sources, the grid arithmetic restated here (every
case named for a second trip makes one, no other does), every case against its description, the models against independent
restatements and that each listed wrong kernel - a variant of the models below - changes at least one output bit on that row's
input.

One wrong kernel that suggests itself cannot exist: `srcB row index row * nk instead of row * 4` - srcB is read only when nk == 4, the
two are the same kernel.  Its place is taken by `srcb_row_k` (row * 4 + k, the index srcA's variants have).  Two refusals of the
launchers cannot be reached either: n N > 65535 and 2 N > 65535 lie behind n <= 12 and N <= 4096 (12 x 4096 = 49 152).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ensemble_model as EM
import metrics_model as MM
import tiles_model as TM
from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
SSIM_TOL = 1e-9            # test_hip_metrics.SSIM_TOL; its derivation stands in that file's docstring

GATHER, STITCH, D8G, D8M = "tgsr_tile_gather", "tgsr_tile_stitch", "tgsr_d8_gather", "tgsr_d8_merge"
METRICS, WS_ELEMS, RGB2Y = "tgsr_sr_metrics", "tgsr_sr_metrics_ws_elems", "tgsr_rgb_to_y_u8"
K_G = {"u8": "tile_gather_kernel<uint8_t>", "f32": "tile_gather_kernel<float>"}
K_S = "tile_stitch_kernel"
K_DG = {"u8": "d8_gather_kernel<uint8_t>", "f32": "d8_gather_kernel<float>"}
K_DM = "d8_merge_kernel"
K_FIN, K_Y = "sr_metrics_finish_kernel", "rgb_to_y_u8_kernel"
K_M = {(sr, hr): "sr_metrics_tile_kernel<%s,%s>" % ("true" if sr == "f" else "false", "true" if hr == "f" else "false")
       for sr in "fu" for hr in "fu"}
PAIRS = (("f", "f"), ("f", "u"), ("u", "f"), ("u", "u"))
STITCH_MAX = 12

V_GATHER = ("quad_floor", "pitch_tw", "tail_dropped", "prev_row", "img2_from_img")
V_STITCH = ("whole_window", "origin_unscaled", "first_quad_dropped", "last_quad_whole", "stride_block", "col_not_offset", "u8_trunc")
V_D8G = ("mirror_first", "b0b1_swapped", "transposed_as_thtw")
V_D8M = ("mirror_first", "b0b1_swapped", "transposed_as_thtw", "desc_sum", "pairwise_sum", "srcb_row_k", "u8_trunc")
V_METRICS = ("tiles_swapped", "shave_one_side", "centres_Hc5", "ws_wrong_count", "y_no_half", "ssey_unshaved")
V_Y = ("y_no_half",)
FILL = np.float32(12345.0)          # what a model's wrong kernel leaves where it writes nothing


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def _frozen(a):
    a.setflags(write=False)
    return a


# ----------------------------------------------------------------------------------------------------------------------------
# Window tables
# ----------------------------------------------------------------------------------------------------------------------------
def _wins(th, tw, origins):
    """Rows (y0, x0, ...) of windows that own themselves."""
    return np.array([(y0, x0, y0, y0 + th, x0, x0 + tw) for y0, x0 in origins], np.int32)


def _plan(H, W, th, tw, halo):
    from tgsr_amd.tiles import plan_tiles
    return plan_tiles(H, W, (th, tw), halo).numpy().astype(np.int32)


def desc_ok(d, H, W, th, tw):
    """tile_desc_ok / d8_desc_ok, restated."""
    y0, x0, oy0, oy1, ox0, ox1 = (int(v) for v in d)
    if y0 < 0 or x0 < 0 or y0 > H - th or x0 > W - tw:
        return False
    if oy0 < y0 or oy1 <= oy0 or oy1 > y0 + th:
        return False
    return not (ox0 < x0 or ox1 <= ox0 or ox1 > x0 + tw)


def dev_table(c):
    """The device copy of a case's table: the host's, or with `bad` = (row, how) one row that fails desc_ok - "x0": x0 = W - tw + 1,
    "oy": oy1 = oy0.  The kernels return on it before they form an address."""
    t = c["table"].copy()
    if c.get("bad"):
        i, how = c["bad"]
        if how == "x0":
            t[i, 1] = c["W"] - c["tw"] + 1
        else:
            t[i, 3] = t[i, 2]
    return t


def good_rows(c):
    return [t for t in range(len(c["table"])) if not c.get("bad") or t != c["bad"][0]]


# ----------------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------------
def _ga(name, H, W, th, tw, table, want, two=True, mis=(), bad=None, N=None, k0=None, nk=None):
    """A gather case (tile or d8): mis - which of img, img2, out, out2 lies one byte (uint8) / one word off its alignment; want =
    (vec_in, vec_out), written by hand."""
    return dict(name=name, H=H, W=W, th=th, tw=tw, table=_frozen(np.asarray(table, np.int32)), want=want, two=two, mis=tuple(mis), bad=bad,
                N=N, k0=k0, nk=nk)


O6 = ((0, 0), (4, 4), (1, 8), (2, 1), (3, 3), (4, 6))                       # x0 in {0, 4, 8, 1, 3, 6}
_G = ("quad_floor", "pitch_tw", "prev_row", "img2_from_img")
G_CASES = (
    (_ga("vec-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, O6), (1, 1)),
     "img, img2, out, out2 aligned, W = 16, tw = 8: vec_in = vec_out = 1; x0 in {0, 4, 8, 1, 3, 6}: vin = vec_in && x0 % 4 == 0 holds for three "
     "windows and fails for three in one launch", _G),
    (_ga("W14-6x14-3x4", 6, 14, 3, 4, _wins(3, 4, ((0, 0), (1, 4), (3, 10), (2, 1))), (0, 1)),
     "W % 4 == 0 fails alone (W = 14): vec_in = 0, vec_out = 1", _G),
    (_ga("tw7-9x16-5x7", 9, 16, 5, 7, _wins(5, 7, ((0, 0), (4, 4), (2, 9), (1, 1))), (1, 0)),
     "tw % 4 == 0 fails alone (tw = 7): vec_out = 0, a tail group of 3, no vector store", V_GATHER),
    (_ga("img-off-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, O6), (0, 1), mis=("img",)),
     "aligned_to(img, in_align) fails alone: vec_in = 0", _G),
    (_ga("img2-off-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, O6), (0, 1), mis=("img2",)),
     "(!img2 || aligned_to(img2, in_align)) fails alone: vec_in = 0", _G),
    (_ga("out2-off-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, O6), (1, 0), mis=("out2",)),
     "(!out2 || aligned_to(out2, 16)) fails alone: vec_out = 0", _G),
    (_ga("no-img2-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, O6), (1, 1), two=False),
     "img2 == NULL: grid.z = img2 ? 2u : 1u = 1, out2 stays untouched", ("quad_floor", "pitch_tw", "prev_row")),
    (_ga("1x1", 1, 1, 1, 1, _wins(1, 1, ((0, 0),)), (0, 0)), "H = W = th = tw = 1: one item", ("img2_from_img",)),
    (_ga("repeat-unordered-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, ((4, 8), (0, 0), (4, 8), (2, 3), (0, 4), (2, 3))), (1, 1)),
     "a window named twice and windows out of raster order: out[t] is row t's window whatever the order", _G),
    (_ga("second-trip-148x148", 150, 152, 148, 148, _wins(148, 148, ((0, 0), (2, 3))), (1, 1)),
     "items = 3 * th * ((tw + 3) / 4) = 16 428 > 64 * 256: a second trip of the stride loop", _G),
    (_ga("second-trip-4096x5", 4096, 8, 4096, 5, _wins(4096, 5, ((0, 0), (0, 3))), (1, 0), two=False),
     "a thin window, items = 3 * 4096 * 2 = 24 576 > 64 * 256: a second trip, every group of the second column a tail of 1",
     ("quad_floor", "pitch_tw", "tail_dropped", "prev_row")),
    (_ga("dev-row-x0-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, O6), (1, 1), bad=(2, "x0")),
     "table_dev row 2 has x0 = W - tw + 1 (the host copy is valid): !tile_desc_ok: the workgroups of the window return, its block keeps its bits",
     _G),
    (_ga("dev-row-oy-9x16-5x8", 9, 16, 5, 8, _wins(5, 8, O6), (1, 1), bad=(3, "oy")),
     "table_dev row 3 has oy1 = oy0: !tile_desc_ok", _G),
)


def _dg(name, H, W, th, tw, origins, want, k0, nk, N=1, **kw):
    return _ga(name, H, W, th, tw, _wins(th, tw, origins), want, N=N, k0=k0, nk=nk, **kw)


_X4 = ((0, 0), (1, 1), (2, 2), (0, 3))                                      # x0 % 4 in {0, 1, 2, 3}
_ALL_D8G = V_D8G
DG_CASES = (
    (_dg("k08-8x8-N3", 11, 16, 8, 8, _X4 + ((3, 8),), (1, 1), 0, 8, N=3),
     "(k0, nk) = (0, 8), sides below 32, N = 3 with img2: blockIdx.z = 2 * image + which; vec_in = vec_out = 1, x0 % 4 in {0, 1, 2, 3}",
     ("mirror_first", "b0b1_swapped")),
    (_dg("k08-32x32", 34, 36, 32, 32, _X4, (1, 1), 0, 8, two=False), "(0, 8), sides equal to 32: one whole block per channel, no img2",
     ("mirror_first", "b0b1_swapped")),
    (_dg("k08-33x33", 36, 36, 33, 33, _X4, (1, 0), 0, 8, two=False),
     "(0, 8), sides 32 + 1: mirrored variants start at r0 = c0 = -31, the last block holds one row and one column; tw % 4 fails: vec_out = 0",
     ("mirror_first", "b0b1_swapped")),
    (_dg("k08-63x63", 64, 68, 63, 63, ((0, 0), (1, 1), (0, 2), (1, 3), (1, 5)), (1, 0), 0, 8, two=False), "(0, 8), sides 32 + 31: r0 = c0 = -1 in the mirrored variants",
     ("mirror_first", "b0b1_swapped")),
) + tuple(
    (_dg("k%d4-%dx%d" % (k0, th, tw), th + 2, (tw + 3 + 3) // 4 * 4, th, tw, _X4[:3] + ((2, 3),), (1, int(th % 4 == 0 and tw % 4 == 0)), k0, 4,
         two=(th, tw) == (33, 32)),
     "(k0, nk) = (%d, 4) on a %d x %d window: %s" % (k0, th, tw, "the transposed group [tw][th]" if k0 else "the group [th][tw]"),
     ("mirror_first", "b0b1_swapped", "transposed_as_thtw") if k0 else ("b0b1_swapped",))
    for k0 in (0, 4) for th, tw in ((33, 32), (63, 32), (32, 33), (32, 63), (8, 12))
) + tuple(
    (_dg("k%d4-8x8" % k0, 11, 16, 8, 8, _X4 + ((3, 8),), (1, 1), k0, 4, N=3), "(k0, nk) = (%d, 4) on square windows, N = 3 with img2" % k0,
     ("mirror_first", "b0b1_swapped") if k0 else ("b0b1_swapped",)) for k0 in (0, 4)
) + (
    (_dg("W18-k08-8x8", 11, 18, 8, 8, _X4 + ((3, 10),), (0, 1), 0, 8), "W % 4 == 0 fails alone (W = 18): vec_in = 0", ("mirror_first", "b0b1_swapped")),
    (_dg("img-off-k08-8x8", 11, 16, 8, 8, _X4, (0, 1), 0, 8, mis=("img",)), "d8_aligned(img, in_align) fails alone: vec_in = 0",
     ("mirror_first", "b0b1_swapped")),
    (_dg("img2-off-k08-8x8", 11, 16, 8, 8, _X4, (0, 1), 0, 8, mis=("img2",)), "(!img2 || d8_aligned(img2, in_align)) fails alone: vec_in = 0",
     ("mirror_first", "b0b1_swapped")),
    (_dg("tw6-k04-8x6", 11, 16, 8, 6, _X4, (1, 0), 0, 4), "tw % 4 == 0 fails alone (8 x 6): vec_out = 0", ("b0b1_swapped",)),
    (_dg("th6-k44-6x8", 11, 16, 6, 8, _X4, (1, 0), 4, 4), "th % 4 == 0 fails alone (6 x 8, the transposed group's rows are 6 long): vec_out = 0",
     ("mirror_first", "b0b1_swapped", "transposed_as_thtw")),
    (_dg("out-off-k08-8x8", 11, 16, 8, 8, _X4, (1, 0), 0, 8, mis=("out",)), "d8_aligned(out, 16) fails alone: vec_out = 0", ("mirror_first", "b0b1_swapped")),
    (_dg("out2-off-k08-8x8", 11, 16, 8, 8, _X4, (1, 0), 0, 8, mis=("out2",)), "(!out2 || d8_aligned(out2, 16)) fails alone: vec_out = 0",
     ("mirror_first", "b0b1_swapped")),
    (_dg("second-trip-k04-4096x65", 4096, 68, 4096, 65, ((0, 3),), (1, 0), 0, 4, two=False),
     "blocks = 3 * 128 * 3 = 1152 > 1024: a second trip of the block loop; N = 1, no img2, nk = 4: a 12.8 MB output (577 x 577: 16 MB)",
     ("b0b1_swapped",)),
    (_dg("dev-row-x0-k08-8x8", 11, 16, 8, 8, _X4 + ((3, 8),), (1, 1), 0, 8, N=3, bad=(2, "x0")),
     "table_dev row 2 has x0 = W - tw + 1: !d8_desc_ok: the window's nk variants of every image keep their bits", ("mirror_first", "b0b1_swapped")),
    (_dg("dev-row-oy-k44-8x12", 11, 16, 8, 12, _X4, (1, 1), 4, 4, bad=(1, "oy")), "table_dev row 1 has oy1 = oy0: !d8_desc_ok",
     ("mirror_first", "b0b1_swapped", "transposed_as_thtw")),
)


def _e(C, s, u8=0, extra=0, soff=0, doff=0, boff=0):
    """A list entry: src_stride = block + extra (the gap guarded), src `soff` words off 16 bytes, srcB `boff` words, dst `doff` words
    (float32) or bytes (uint8) off."""
    return dict(C=C, s=s, u8=u8, extra=extra, soff=soff, doff=doff, boff=boff)


def _st(name, H, W, th, tw, table, entries, bad=None, zero_stride=False, nk=None, N=None):
    return dict(name=name, H=H, W=W, th=th, tw=tw, table=_frozen(np.asarray(table, np.int32)), entries=tuple(entries), bad=bad,
                zero_stride=zero_stride, nk=nk, N=N)


MIX12 = (_e(1, 1), _e(3, 1, 1), _e(18, 1), _e(3, 2), _e(3, 2, 1), _e(18, 2, extra=8), _e(1, 3), _e(3, 3, 1), _e(3, 8), _e(3, 8, 1), _e(1, 64),
         _e(1, 64, 1))
_P716 = _plan(7, 16, 4, 8, 1)          # 3 x 3 windows; owned columns start at 0, 7 and 13, rows at 0, 3 and 5
_ST = ("whole_window", "origin_unscaled", "first_quad_dropped", "col_not_offset", "u8_trunc")
# last_quad_whole lands in the neighbour's columns, which the neighbour writes too: it shows where the neighbour writes nothing
ST_CASES = (
    (_st("n12-7x16-4x8", 7, 16, 4, 8, _P716, MIX12),
     "n = TGSR_STITCH_MAX = 12 entries in one launch, C in {1, 3, 18}, s in {1, 2, 3, 8, 64}, float32 and uint8: vec_src[e] = (s tw) % 4 == 0 && "
     "aligned_to(src[e], 16) && src_stride[e] % 4 == 0 and vec_dst[e] = (s W) % 4 == 0 && aligned_to(dst[e], out_u8[e] ? 4 : 16) hold for "
     "every entry; vsrc = vec_src && (s x0) % 4 == 0 fails for x0 = 6 at odd s; gx = vdst ? xa & ~3 : xa: partial first and last quads", _ST + ("stride_block",)),
    (_st("stride-odd-7x16-4x8", 7, 16, 4, 8, _P716, (_e(3, 1, extra=1), _e(3, 2, 1, extra=1))),
     "src_stride[e] % 4 == 0 fails alone (src_stride = block + 1): vec_src = 0, vec_dst = 1", _ST + ("stride_block",)),
    (_st("src-off-7x16-4x8", 7, 16, 4, 8, _P716, (_e(3, 1, soff=1), _e(3, 2, 1, soff=1))), "aligned_to(src[e], 16) fails alone: vec_src = 0", _ST),
    (_st("stw-odd-7x16-4x7", 7, 16, 4, 7, _plan(7, 16, 4, 7, 1), (_e(3, 1), _e(3, 3, 1))), "(s tw) % 4 == 0 fails alone (tw = 7, s = 1, 3): vec_src = 0",
     _ST),
    (_st("dst-off-7x16-4x8", 7, 16, 4, 8, _P716, (_e(3, 1, doff=1), _e(3, 2, 1, doff=1), _e(3, 1, 1, doff=2), _e(1, 3, 1, doff=3))),
     "aligned_to(dst[e], out_u8[e] ? 4 : 16) fails alone: float32 one word off, uint8 1, 2 and 3 bytes off: vec_dst = 0, vec_src = 1",
     ("whole_window", "origin_unscaled", "col_not_offset", "u8_trunc")),
    (_st("sW-7x14-4x8", 7, 14, 4, 8, _plan(7, 14, 4, 8, 1), (_e(3, 1), _e(3, 3, 1))), "(s W) % 4 == 0 fails while (s tw) % 4 == 0 (W = 14, s = 1, 3): vec_dst = 0",
     ("whole_window", "origin_unscaled", "col_not_offset", "u8_trunc")),
    (_st("crop-7x16-4x8", 7, 16, 4, 8, _P716, (_e(3, 2, extra=384), _e(3, 1, 1, extra=96))),
     "src_stride = 2 block: the first 3 channels of a buffer of 6, taken in place; the other 3 neither read nor written", _ST + ("stride_block",)),
    (_st("Tb1-stride0-5x8", 5, 8, 5, 8, _wins(5, 8, ((0, 0),)), (_e(3, 2), _e(1, 3, 1)), zero_stride=True),
     "Tb == 1 with src_stride = 0 < block: accepted (src_stride[e] < block && Tb > 1 refuses)", ("u8_trunc",)),
    (_st("padded-7x16-4x8", 7, 16, 4, 8, np.concatenate([_P716, _P716[-1:]]), (_e(3, 2), _e(3, 1, 1))),
     "a padded last batch: the last window twice, with the same tile values: the same bits written twice", _ST),
    (_st("hole-7x16-4x8", 7, 16, 4, 8, np.delete(_P716, 4, axis=0), (_e(3, 2), _e(3, 1, 1), _e(1, 3, 1, doff=1))),
     "owned rectangles that do not cover the image (the middle window dropped): the hole keeps what dst held, float32 and uint8",
     _ST + ("last_quad_whole",)),
    (_st("second-trip-37x40-37x37", 37, 40, 37, 37, np.array([(0, 0, 0, 37, 0, 37), (0, 3, 0, 37, 37, 40)], np.int32), (_e(3, 8), _e(1, 1, 1))),
     "most = C s th ((s tw + 3) / 4 + 1) = 3 * 8 * 37 * 75 = 66 600 > 256 * 256: grid.x = 256, and window 0, which owns all its 37 columns, has "
     "C rows ng = 3 * 296 * 74 = 65 712 items: a second trip of the item loop", _ST),
    (_st("dev-row-x0-7x16-4x8", 7, 16, 4, 8, _P716, (_e(3, 2), _e(3, 1, 1)), bad=(4, "x0")),
     "table_dev row 4 has x0 = W - tw + 1: !tile_desc_ok: its owned rectangle keeps what dst held", _ST + ("last_quad_whole",)),
    (_st("dev-row-oy-7x16-4x8", 7, 16, 4, 8, _P716, (_e(3, 2), _e(3, 1, 1)), bad=(5, "oy")), "table_dev row 5 has oy1 = oy0: !tile_desc_ok",
     _ST + ("last_quad_whole",)),
)
ST_UNREACHABLE = dict(name="items-64-bit", unreachable=True)

_ORDER = ("desc_sum", "pairwise_sum")
_M8 = ("mirror_first", "b0b1_swapped") + _ORDER + ("u8_trunc",)
_M4 = ("mirror_first", "b0b1_swapped", "srcb_row_k") + _ORDER + ("u8_trunc",)
MIX12_M = tuple(dict(e, extra=(e["extra"] or (4 if i % 5 == 2 else 0))) for i, e in enumerate(MIX12))
_P77 = _plan(7, 7, 4, 4, 1)            # 3 x 3 square windows, owned columns and rows start at 0, 3 and 5


def _cross(th, tw, ys, xs):
    """The product of two hand-written axis plans [(origin, own0, own1)]."""
    return np.array([(y0, x0, a0, a1, b0, b1) for y0, a0, a1 in ys for x0, b0, b1 in xs], np.int32)


_T33 = _cross(2, 2, ((0, 0, 2), (1, 2, 3)), ((0, 0, 2), (1, 2, 3)))                      # 3 x 3 image, 2 x 2 windows
_T38 = _cross(2, 4, ((0, 0, 2), (1, 2, 3)), ((0, 0, 3), (2, 3, 5), (4, 5, 8)))           # 3 x 8, 2 x 4 windows, owned columns from 3 and 5


def _dm(name, nk, N, H, W, th, tw, table, entries, **kw):
    return _st(name, H, W, th, tw, table, entries, nk=nk, N=N, **kw)


DM_CASES = (
    (_dm("nk8-n12-3x3-2x2", 8, 1, 3, 3, 2, 2, _T33, MIX12_M),
     "nk = 8: srcA only, th == tw; n = 12 entries, the scale mix with s = 64, uint8 and float32, strides above the block; vec_src = (s tw) % 4 == 0 "
     "&& (s th) % 4 == 0 && d8_aligned(srcA[e], 16) && (!b || d8_aligned(b, 16)) && src_stride[e] % 4 == 0 holds, vec_dst = (s W) % 4 == 0 "
     "&& ... fails at odd s and holds at s = 8, 64, where x_lo is 0", _M8),
    (_dm("nk4-n12-3x8-2x4", 4, 1, 3, 8, 2, 4, _T38, MIX12_M),
     "nk = 4: srcA holds variants 0..3, srcB the transposed 4..7; n = 12; W = 8: vec_dst holds for every entry, owned columns 3 and 5 give "
     "x_lo in {-3, -2, -1} in block column 0 under vdst", _M4 + ("transposed_as_thtw",)),
    (_dm("nk8-N3-hole-7x8-4x4", 8, 3, 7, 8, 4, 4, np.delete(_plan(7, 8, 4, 4, 1), 5, axis=0), (_e(3, 2), _e(3, 1, 1), _e(1, 3, 1, doff=1))),
     "nk = 8, N = 3: blockIdx.z = entry * N + image; a window dropped: the hole keeps what dst held", _M8),
    (_dm("nk4-N3-padded-7x16-4x8", 4, 3, 7, 16, 4, 8, np.concatenate([_P716, _P716[-1:]]), (_e(3, 2), _e(3, 1, 1))),
     "nk = 4, N = 3, a padded last batch: the last window twice with the same variant values", _M4 + ("transposed_as_thtw",)),
    (_dm("nk4-hole-7x16-4x8", 4, 1, 7, 16, 4, 8, np.delete(_P716, 4, axis=0), (_e(3, 2), _e(3, 1, 1), _e(1, 3, 1, doff=1))),
     "nk = 4, the middle window dropped: the hole keeps what dst held, float32 and uint8", _M4 + ("transposed_as_thtw",)),
    (_dm("nk8-padded-7x7-4x4", 8, 1, 7, 7, 4, 4, np.concatenate([_P77, _P77[-1:]]), (_e(3, 2, extra=4), _e(3, 1, 1))),
     "nk = 8, a padded last batch: the last window twice with the same variant values", _M8),
    (_dm("nk4-srcB-off-7x16-4x8", 4, 1, 7, 16, 4, 8, _P716, (_e(3, 2, boff=1), _e(3, 1, 1, boff=1))),
     "(!b || d8_aligned(b, 16)) fails alone: vec_src = 0", _M4 + ("transposed_as_thtw",)),
    (_dm("nk4-srcA-off-7x16-4x8", 4, 1, 7, 16, 4, 8, _P716, (_e(3, 2, soff=1), _e(3, 1, 1, extra=1))),
     "d8_aligned(srcA[e], 16) fails alone for entry 0, src_stride[e] % 4 == 0 alone for entry 1: vec_src = 0", _M4 + ("transposed_as_thtw",)),
    (_dm("nk4-sth-odd-7x16-5x8", 4, 1, 7, 16, 5, 8, _plan(7, 16, 5, 8, 1), (_e(3, 1), _e(3, 3, 1))),
     "(s th) % 4 == 0 fails alone (th = 5): vec_src = 0", _M4 + ("transposed_as_thtw",)),
    (_dm("nk4-dst-off-7x16-4x8", 4, 1, 7, 16, 4, 8, _P716, (_e(3, 1, doff=1), _e(3, 2, 1, doff=1), _e(3, 1, 1, doff=2), _e(1, 3, 1, doff=3))),
     "d8_aligned(dst[e], out_u8[e] ? 4 : 16) fails alone: vec_dst = 0", _M4 + ("transposed_as_thtw",)),
) + tuple(
    (_dm("nk%d-%dx%d" % (nk, th, tw), nk, 1, th + 3, (tw + 8) // 4 * 4, th, tw, _plan(th + 3, (tw + 8) // 4 * 4, th, tw, 1), (_e(2, 1), _e(1, 1, 1))),
     "nk = %d, window %d x %d at s = 1: sides 32 k + r, the mirrored variants' blocks start at negative r0 / c0, the last block is partial"
     % (nk, th, tw), (_M8 if nk == 8 else _M4 + ("transposed_as_thtw",)))
    for nk, th, tw in ((8, 32, 32), (8, 33, 33), (8, 63, 63), (4, 33, 32), (4, 63, 32), (4, 32, 33), (4, 32, 63))
) + (
    (_dm("second-trip-nk4-4096x1", 4, 1, 4096, 2, 4096, 1, np.array([(0, 0, 0, 4096, 0, 1), (0, 1, 0, 4096, 1, 2)], np.int32), (_e(33, 1),)),
     "C nby nbx = 33 * 128 * 1 = 4224 blocks against min(most, 4096): a second trip of the block loop", _M4[:3] + _ORDER),
    (_dm("dev-row-x0-nk8-7x7-4x4", 8, 1, 7, 7, 4, 4, _P77, (_e(3, 2), _e(3, 1, 1)), bad=(4, "x0")), "table_dev row 4 has x0 = W - tw + 1: !d8_desc_ok", _M8),
    (_dm("dev-row-oy-nk4-7x16-4x8", 4, 1, 7, 16, 4, 8, _P716, (_e(3, 2), _e(3, 1, 1)), bad=(5, "oy")), "table_dev row 5 has oy1 = oy0: !d8_desc_ok",
     _M4 + ("transposed_as_thtw",)),
)


def _mc(hc, wc, shave, B, leads=False, same=False):
    return dict(name="%dx%d-shave%d-B%d%s" % (hc, wc, shave, B, "-identical" if same else ""), hc=hc, wc=wc, shave=shave, B=B, H=hc + 2 * shave,
                W=wc + 2 * shave, leads=leads, same=same)


CROPS = ((11, 11, "one window, the whole halo outside the crop"), (33, 43, "a last tile row of 1 pixel"),
         (37, 70, "tiles_y = 2, tiles_x = 3 (swapped counts show); the last tile row, 5 pixels high, holds no window centre"),
         (43, 43, "a last tile with 6 window centres per axis"))
M_CASES = tuple(
    (_mc(hc, wc, shave, 1 if shave == 3 else 3, leads=(shave != 0)),
     "crop %d x %d: %s; shave %d: the first crop column is %s a word" % (hc, wc, why, shave, "on" if shave % 4 == 0 else "off"),
     tuple(v for v in V_METRICS if not ((v in ("shave_one_side", "ssey_unshaved") and shave == 0) or (v == "tiles_swapped" and -(-hc // 32) == -(-wc // 32))
                                        or (v == "ws_wrong_count" and (shave == 3 or hc <= 32)))))
    for hc, wc, why in CROPS for shave in (0, 3, 4))
M_SAME = _mc(37, 70, 4, 3, same=True)


def _yc(name, B, H, W, leads):
    return dict(name=name, B=B, H=H, W=W, leads=leads)


Y_CASES = ((_yc("B3-5x7", 3, 5, 7, True), "B = 3, a plane of 35 bytes; rgb and y 0 .. 3 bytes off a word, independently"),
           (_yc("B1-3x3", 1, 3, 3, False), "B = 1, a plane of 9 bytes"),
           (_yc("second-trip-B3-1183x1183", 3, 1183, 1183, False),
            "total = 4 198 467 > 16384 * 256: a second trip that crosses into the last image (i / plane = 2)"))

R_GATHER = ("img or out NULL; img2 and out2 not both or neither; table_host or table_dev NULL; Tb outside [1, 65535]; H or W < 1 or > 2^20; th or tw "
            "< 1, > H / W or > 4096; a host row that fails tile_desc_ok: refused")
R_STITCH = ("n outside [1, 12]; src, src_stride, dst, C, scale or out_u8 NULL; a NULL src[e] or dst[e]; C[e] outside [1, 65535]; scale[e] outside "
            "[1, 64]; src_stride[e] < block && Tb > 1; every rule of tgsr_tile_gather's table: refused")
R_D8G = ("tgsr_tile_gather's, and N outside [1, 4096]; (k0, nk) not (0, 8), (0, 4) or (4, 4); (0, 8) with th != tw; N * (two + 1) > 65535 "
         "(unreachable behind N <= 4096): refused")
R_D8M = ("tgsr_tile_stitch's with srcA for src; src_stride[e] < block whatever Tb; nk not 8 or 4, nk = 8 with th != tw; (b != nullptr) != (nk == 4); "
         "n * N > 65535 (unreachable: 12 * 4096): refused")
R_METRICS = "sr, hr, ws or out NULL; B outside [1, 65535]; H or W < 1; shave < 0; a crop under 11 on either side: refused, ws_elems == 0"
R_Y = "rgb or y NULL; B, H or W < 1: refused"

TABLE = (
    [(GATHER, K_G[dt], cond, dict(c, dt=dt, name=dt + "-" + c["name"]), catch) for dt in ("u8", "f32") for c, cond, catch in G_CASES]
    + [(GATHER, "no instance", R_GATHER, None, ())]
    + [(STITCH, K_S, cond, c, catch) for c, cond, catch in ST_CASES]
    + [(STITCH, K_S, "items <= (int64_t)0x7fffffff - step fails: the 64-bit item loop.  items = C rows ng > 2^31 - 65 536 while the destination "
        "holds C (s H)(s W) >= C rows 4 (ng - 1) elements: more than 2^33 - 8 GiB of uint8, 32 GiB of float32 - and the source as many floats: "
        "unreachable in a test", ST_UNREACHABLE, ()),
       (STITCH, "no instance", R_STITCH, None, ())]
    + [(D8G, K_DG[dt], cond, dict(c, dt=dt, name=dt + "-" + c["name"]), catch) for dt in ("u8", "f32") for c, cond, catch in DG_CASES]
    + [(D8G, "no instance", R_D8G, None, ())]
    + [(D8M, K_DM, cond, c, catch) for c, cond, catch in DM_CASES]
    + [(D8M, "no instance", R_D8M, None, ())]
    + [(METRICS, " / ".join(K_M[p] for p in PAIRS) + " + " + K_FIN,
        "sr_f32 && hr_f32, else sr_f32, else hr_f32, else neither: the four pairings, the same bits; grid(tiles_x * tiles_y, B); ws of exactly "
        "tgsr_sr_metrics_ws_elems doubles.  " + cond, c, catch) for c, cond, catch in M_CASES]
    + [(METRICS, K_M[("f", "f")] + " / " + K_M[("u", "u")] + " + " + K_FIN, "identical images: (0, 0, windows * 1.0), every window exactly 1", M_SAME, ()),
       (METRICS, "no instance", R_METRICS, None, ())]
    + [(RGB2Y, K_Y, "always; g > 16384 ? 16384 : g.  " + cond, c, V_Y) for c, cond in Y_CASES]
    + [(RGB2Y, "no instance", R_Y, None, ())])


def _rows(*entries):
    return [r for r in TABLE if r[0] in entries and r[3] is not None and not r[3].get("unreachable")]


def row_id(r):
    return r[0][5:] + "-" + r[3]["name"]


# ----------------------------------------------------------------------------------------------------------------------------
# The launchers' arithmetic, restated
# ----------------------------------------------------------------------------------------------------------------------------
KBLK = 32


def _trips(work, cap):
    return -(-work // max(1, min(work, cap)))


def gather_plan(c):
    """tgsr_tile_gather: items of 4 columns per window, 256 threads, grid.x <= 64."""
    items = 3 * c["th"] * ((c["tw"] + 3) // 4)
    blocks = min((items + 255) // 256, 64)
    return dict(items=items, blocks=blocks, trips=-(-items // (blocks * 256)))


def stitch_plan(c):
    """tgsr_tile_stitch: most = max over the entries of C s th ((s tw + 3) / 4 + 1), grid.x <= 256 blocks of 256."""
    most = max(e["C"] * e["s"] * c["th"] * ((e["s"] * c["tw"] + 3) // 4 + 1) for e in c["entries"])
    blocks = min((most + 255) // 256, 256)
    return dict(most=most, blocks=blocks, trips=-(-most // (blocks * 256)))


def stitch_items(c, e, row):
    """What the kernel walks for one window of one entry: C rows ng with its own gx."""
    s = e["s"]
    xa, xb = s * int(row[4]), s * int(row[5])
    gx = xa & ~3 if stitch_flags(c, e)[1] else xa
    return e["C"] * s * int(row[3] - row[2]) * ((xb - gx + 3) >> 2)


def d8g_plan(c):
    blocks = 3 * (-(-c["th"] // KBLK)) * (-(-c["tw"] // KBLK))
    return dict(blocks=blocks, grid=min(blocks, 1024), trips=_trips(blocks, 1024))


def d8m_plan(c):
    """tgsr_d8_merge: grid.x = min(most, 4096), most over the entries of C ceil(s th / 32) ceil((s tw + 3) / 32); the kernel walks
    C nby nbx blocks of the owned rectangle."""
    most = max(e["C"] * (-(-e["s"] * c["th"] // KBLK)) * (-(-(e["s"] * c["tw"] + 3) // KBLK)) for e in c["entries"])
    grid = min(most, 4096)
    walked = 0
    for e in c["entries"]:
        vdst = merge_flags(c, e)[1]
        for row in c["table"]:
            s = e["s"]
            xa, xb, ya, yb = s * int(row[4]), s * int(row[5]), s * int(row[2]), s * int(row[3])
            gx = xa & ~3 if vdst else xa
            walked = max(walked, e["C"] * (-(-(yb - ya) // KBLK)) * (-(-(xb - gx) // KBLK)))
    return dict(most=most, grid=grid, walked=walked, trips=-(-walked // grid))


def metrics_tiles(c):
    return -(-c["hc"] // 32), -(-c["wc"] // 32)


def y_plan(c):
    total = c["B"] * c["H"] * c["W"]
    blocks = min((total + 255) // 256, 16384)
    return dict(total=total, blocks=blocks, trips=-(-total // (blocks * 256)))


def gather_flags(c, d8=False):
    """(vec_in, vec_out) of tgsr_tile_gather / tgsr_d8_gather from the case's description of where its operands lie."""
    mis, two = c["mis"], c["two"]
    vec_in = c["W"] % 4 == 0 and "img" not in mis and not (two and "img2" in mis)
    vec_out = c["tw"] % 4 == 0 and (not d8 or c["th"] % 4 == 0) and "out" not in mis and not (two and "out2" in mis)
    return int(vec_in), int(vec_out)


def stitch_flags(c, e):
    """(vec_src, vec_dst) of one entry of tgsr_tile_stitch."""
    block = e["C"] * e["s"] ** 2 * c["th"] * c["tw"]
    stride = 0 if c["zero_stride"] else block + e["extra"]
    return (int((e["s"] * c["tw"]) % 4 == 0 and e["soff"] == 0 and stride % 4 == 0), int((e["s"] * c["W"]) % 4 == 0 and e["doff"] == 0))


def merge_flags(c, e):
    block = e["C"] * e["s"] ** 2 * c["th"] * c["tw"]
    vs = (e["s"] * c["tw"]) % 4 == 0 and (e["s"] * c["th"]) % 4 == 0 and e["soff"] == 0 and e["boff"] == 0 and (block + e["extra"]) % 4 == 0
    return int(vs), int((e["s"] * c["W"]) % 4 == 0 and e["doff"] == 0)


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ties():
    k = np.arange(255, dtype=np.float32)
    t = ((k + np.float32(0.5)) / np.float32(127.5) - np.float32(1)).astype(np.float32)
    return _frozen(t[(t + np.float32(1)) * np.float32(127.5) == k + np.float32(0.5)])      # (x + 1) * 127.5 is k + 0.5 exactly


def _float_values(shape, *seed):
    """float32 outputs of a generator, as a destination sees them: most inside [-1, 1], some outside, one in seven on an exact
    rounding tie of tgsr_to_uint8."""
    rng = _rng(*seed)
    x = (rng.standard_normal(shape) * 0.6).astype(np.float32)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 7), replace=False)
    flat[idx] = rng.choice(_ties(), size=idx.size)
    idx = rng.choice(flat.size, size=max(1, flat.size // 50), replace=False)
    flat[idx] = rng.choice(np.array([-3.0, 2.5, -1.0, 1.0, 1.0000001, -1.0000001, 100.0], np.float32), size=idx.size)
    return x


@functools.lru_cache(maxsize=None)
def _image(dt, shape, seed):
    """An image the gathers read: every byte value / floats whose bit copy shows (a negative zero, a subnormal, the largest float)."""
    rng = _rng(seed, *shape)
    if dt == "u8":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
    else:
        a = rng.standard_normal(shape).astype(np.float32)
        flat = a.reshape(-1)
        if flat.size >= 8:
            flat[rng.choice(flat.size, 3, replace=False)] = np.array([-0.0, 1e-40, 3.4028235e38], np.float32)
    return _frozen(a)


def gather_inputs(c):
    shape = ((c["N"],) if c["N"] else ()) + (3, c["H"], c["W"])
    return _image(c["dt"], shape, 1), (_image(c["dt"], shape, 2) if c["two"] else None)


def _base(shape, *seed):
    """What a float32 destination holds before the call: finite, no value a kernel writes."""
    return (_rng(*seed).standard_normal(shape) * 0.01 + 7.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _stitch_inputs(name):
    """Per entry (tiles [Tb][C][s th][s tw], what dst held [C][s H][s W]).  A window named twice has the same tile values twice."""
    c = next(r[3] for r in _rows(STITCH) if r[3]["name"] == name)
    table = c["table"]
    first = [int(np.flatnonzero((table == row).all(1))[0]) for row in table]
    out = []
    for k, e in enumerate(c["entries"]):
        s, C = e["s"], e["C"]
        tiles = _float_values((len(table), C, s * c["th"], s * c["tw"]), k, 11)[first]
        shape = (C, s * c["H"], s * c["W"])
        prior = _rng(k, 12).integers(0, 256, shape, dtype=np.uint8) if e["u8"] else _base(shape, k, 13)
        out.append((_frozen(np.ascontiguousarray(tiles)), _frozen(prior)))
    return out


def owned_mask(table, s, shape):
    """[..., s H, s W] bool: the pixels some row of the table owns."""
    m = np.zeros(shape, bool)
    for _y0, _x0, oy0, oy1, ox0, ox1 in np.asarray(table).tolist():
        m[..., s * oy0:s * oy1, s * ox0:s * ox1] = True
    return m


E24 = np.float32(2.0 ** -24)
ORDER_A = np.array([1, E24, E24, E24, 0, 0, 0, 0], np.float32)     # ascending: 1 (three ties to even); pairwise: 1 + 2^-23
ORDER_B = np.array([E24, E24, 0, 0, 0, 0, 0, 1], np.float32)       # ascending: 1 + 2^-23; descending: 1


@functools.lru_cache(maxsize=None)
def _merge_inputs(name):
    """Per entry (srcA [N Tb nk][C][s th][s tw], srcB [N Tb 4][C][s tw][s th] or None, what dst held [N][C][s H][s W]).  Built on the
    window's side - eight values per pixel - and turned into the variants by ensemble_model.variant: a quarter of the pixels hold
    the same tgsr_to_uint8 tie in all eight (the mean IS the tie), an eighth each ORDER_A and ORDER_B, the rest noise."""
    c = next(r[3] for r in _rows(D8M) if r[3]["name"] == name)
    table, N, nk = c["table"], c["N"], c["nk"]
    first = [int(np.flatnonzero((table == row).all(1))[0]) for row in table]
    out = []
    for k, e in enumerate(c["entries"]):
        s, C = e["s"], e["C"]
        h, w = s * c["th"], s * c["tw"]
        rng = _rng(k, 21)
        win = _float_values((N, len(table), 8, C, h, w), k, 22)
        kind = rng.integers(0, 8, (N, len(table), 1, C, h, w))
        tie = rng.choice(_ties(), size=kind.shape)
        win = np.where(kind < 2, tie, win)
        win = np.where(kind == 2, ORDER_A.reshape(1, 1, 8, 1, 1, 1), win)
        win = np.where(kind == 3, ORDER_B.reshape(1, 1, 8, 1, 1, 1), win).astype(np.float32)[:, first]
        a = np.stack([EM.variant(win[:, :, v], v) for v in range(nk)], axis=2)
        b = np.stack([EM.variant(win[:, :, v], v) for v in range(4, 8)], axis=2) if nk == 4 else None
        shape = (N, C, s * c["H"], s * c["W"])
        prior = _rng(k, 23).integers(0, 256, shape, dtype=np.uint8) if e["u8"] else _base(shape, k, 24)
        out.append((_frozen(np.ascontiguousarray(a.reshape((-1,) + a.shape[3:]))),
                    None if b is None else _frozen(np.ascontiguousarray(b.reshape((-1,) + b.shape[3:]))), _frozen(prior)))
    return out


@functools.lru_cache(maxsize=None)
def _metrics_inputs(name):
    """test_hip_metrics._case's construction: float images with values outside [-1, 1] and inputs on exact rounding ties, and the
    bytes they quantise to: (sr float32, hr float32, sr uint8, hr uint8), each [B][3][H][W]."""
    c = next(r[3] for r in _rows(METRICS) if r[3]["name"] == name)
    shape = (c["B"], 3, c["H"], c["W"])
    hr = _float_values(shape, c["H"], c["W"], 31)
    sr = hr if c["same"] else (hr + (_rng(c["H"], c["W"], 32).standard_normal(shape) * 0.15).astype(np.float32))
    if not c["same"]:
        flat, rng = sr.reshape(-1), _rng(c["H"], c["W"], 33)
        idx = rng.choice(flat.size, size=flat.size // 7, replace=False)
        flat[idx] = rng.choice(_ties(), size=idx.size)
    return tuple(_frozen(x) for x in (sr, hr, MM.quantise(sr), MM.quantise(hr)))


@functools.lru_cache(maxsize=None)
def _y_input(B, H, W):
    return _frozen(_rng(B, H, W, 41).integers(0, 256, (B, 3, H, W), dtype=np.uint8))


# ----------------------------------------------------------------------------------------------------------------------------
# The models' wrong kernels (variant == "": the right one, equal to tiles_model / ensemble_model / metrics_model)
# ----------------------------------------------------------------------------------------------------------------------------
def gather_model(img, img2, table, th, tw, variant=""):
    """tile_gather_kernel.  quad_floor: a window row read from x0 & ~3 (the 16-byte load taken where vin fails); pitch_tw: the image's
    row pitch taken for tw; tail_dropped: the group of fewer than 4 columns not written; prev_row: window t from row t - 1 of the
    table; img2_from_img: out2 gathered from img."""
    table = np.asarray(table)

    def one(x):
        f = TM.normalize_u8(x) if x.dtype == np.uint8 else x
        H, W = x.shape[1:]
        flat, Tb = f.reshape(-1), len(table)
        out = np.empty((Tb, 3, th, tw), np.float32)
        ci, yi, xi = np.meshgrid(np.arange(3), np.arange(th), np.arange(tw), indexing="ij")
        for t in range(Tb):
            y0, x0 = (int(v) for v in table[(t - 1) % Tb if variant == "prev_row" else t][:2])
            if variant == "quad_floor":
                x0 &= ~3
            out[t] = flat[np.minimum((ci * H + y0 + yi) * (tw if variant == "pitch_tw" else W) + x0 + xi, flat.size - 1)]
        if variant == "tail_dropped" and tw % 4:
            out[..., tw // 4 * 4:] = FILL
        return out
    return one(img), (None if img2 is None else one(img if variant == "img2_from_img" else img2))


def _to_u8(v, variant):
    if variant == "u8_trunc":
        return np.clip((np.asarray(v, np.float32) + np.float32(1.0)) * np.float32(127.5), 0, 255).astype(np.uint8)
    return TM.to_uint8(v)


def stitch_model(flat, stride, C, s, table, th, tw, out, vdst, variant="", rows=None):
    """tile_stitch_kernel on the source as it lies in memory: `flat` with tiles `stride` elements apart.  whole_window: the whole
    window written; origin_unscaled: the owned origin in the destination not multiplied by s; first_quad_dropped / last_quad_whole:
    under vdst, the partial first quad not written / the partial last quad written whole (as far as the window reaches);
    stride_block: tiles taken `block` apart; col_not_offset: the source column not offset by s x0; u8_trunc: uint8 by truncation.
    rows: the rows of the table that are stitched (all of them when None)."""
    sth, stw = s * th, s * tw
    block, sW = C * sth * stw, out.shape[-1]
    for t, (y0, x0, oy0, oy1, ox0, ox1) in enumerate(np.asarray(table).tolist()):
        if rows is not None and t not in rows:
            continue
        base = t * (block if variant == "stride_block" else stride)
        tile = flat[base:base + block].reshape(C, sth, stw)
        sy0, sx0, ya, yb, xa, xb = s * y0, s * x0, s * oy0, s * oy1, s * ox0, s * ox1
        if variant == "whole_window":
            ya, yb, xa, xb = sy0, sy0 + sth, sx0, sx0 + stw
        lo, hi = xa, xb
        if vdst and variant == "first_quad_dropped" and xa % 4:
            lo = min(xb, (xa + 3) & ~3)
        if vdst and variant == "last_quad_whole" and xb % 4:
            hi = min((xb + 3) & ~3, sx0 + stw, sW)
        dy, dx = (oy0, ox0 + lo - xa) if variant == "origin_unscaled" else (ya, lo)
        cols = (np.arange(lo, hi) - (0 if variant == "col_not_offset" else sx0)) % stw
        v = tile[:, ya - sy0:yb - sy0][:, :, cols]
        out[:, dy:dy + yb - ya, dx:dx + hi - lo] = _to_u8(v, variant) if out.dtype == np.uint8 else v
    return out


def d8_variant(win, k, variant=""):
    """Variant k of win [..., h, w].  mirror_first: the mirrors before the transpose; b0b1_swapped: bit 0 mirrors the rows, bit 1 the
    columns; transposed_as_thtw: a transposed variant [w][h] addressed with the row pitch of [h][w]."""
    if variant == "b0b1_swapped":
        k = (k & 4) | ((k & 1) << 1) | ((k & 2) >> 1)
    if variant == "mirror_first" and k & 4:
        v = win[..., ::-1, :] if k & 2 else win
        v = v[..., ::-1] if k & 1 else v
        return np.ascontiguousarray(np.swapaxes(v, -1, -2))
    v = EM.variant(win, k)
    return _wrong_pitch(v) if variant == "transposed_as_thtw" and k & 4 else v


def _wrong_pitch(v):
    """v [..., r, c] read at i * r + j instead of i * c + j."""
    r, c = v.shape[-2:]
    i, j = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
    return np.ascontiguousarray(v.reshape(v.shape[:-2] + (r * c,))[..., np.minimum(i * r + j, r * c - 1)])


def d8_back(var, k, variant=""):
    if variant == "b0b1_swapped":
        k = (k & 4) | ((k & 1) << 1) | ((k & 2) >> 1)
    if variant == "transposed_as_thtw" and k & 4:
        var = _wrong_pitch(var)
    if variant == "mirror_first" and k & 4:
        v = np.swapaxes(var, -1, -2)
        v = v[..., ::-1] if k & 1 else v
        return np.ascontiguousarray(v[..., ::-1, :] if k & 2 else v)
    return EM.back(var, k)


def d8_gather_model(imgs, table, th, tw, k0, nk, variant=""):
    f = TM.normalize_u8(imgs) if imgs.dtype == np.uint8 else imgs
    return np.stack([np.stack([np.stack([d8_variant(f[n][:, y0:y0 + th, x0:x0 + tw], k, variant) for k in range(k0, k0 + nk)])
                               for y0, x0 in np.asarray(table)[:, :2]]) for n in range(f.shape[0])])


def merge_model(src_a, src_b, table, th, tw, out, variant="", rows=None):
    """d8_merge_kernel (ensemble_model.merge's arguments).  desc_sum: v7 first; pairwise_sum: ((v0 + v1) + (v2 + v3)) + ((v4 + v5) +
    (v6 + v7)); srcb_row_k: the transposed variant k read at batch row `row * 4 + k` of srcB (modulo its rows), srcA's index;
    u8_trunc: the mean to uint8 by truncation; d8_variant's."""
    table = np.asarray(table)
    N, Tb = out.shape[0], len(table)
    nk = 8 if src_b is None else 4
    s = src_a.shape[2] // th
    a = src_a.reshape((N, Tb, nk) + src_a.shape[1:])
    f32 = np.float32
    for n in range(N):
        for t, (y0, x0, oy0, oy1, ox0, ox1) in enumerate(table.tolist()):
            if rows is not None and t not in rows:
                continue
            vs = []
            for k in range(8):
                if k < nk:
                    var = a[n, t, k]
                else:
                    r = (n * Tb + t) * 4 + (k if variant == "srcb_row_k" else k - 4)
                    var = src_b[r % len(src_b)]
                vs.append(d8_back(var, k, variant))
            if variant == "desc_sum":
                vs = vs[::-1]
            if variant == "pairwise_sum":
                p = [(vs[i] + vs[i + 1]).astype(f32) for i in (0, 2, 4, 6)]
                m = ((((p[0] + p[1]).astype(f32) + (p[2] + p[3]).astype(f32)).astype(f32)) * f32(0.125)).astype(f32)
            else:
                m = EM.mean8(vs)
            m = m[:, s * (oy0 - y0):s * (oy1 - y0), s * (ox0 - x0):s * (ox1 - x0)]
            out[n, :, s * oy0:s * oy1, s * ox0:s * ox1] = _to_u8(m, variant) if out.dtype == np.uint8 else m
    return out


def rgb2y_model(u8, variant=""):
    if variant != "y_no_half":
        return MM.rgb2y(u8)
    f = np.asarray(u8).astype(np.float32) / np.float32(255)
    c = np.array([65.481, 128.553, 24.966], dtype=np.float64) / 255.0
    r, g, b = (f[..., k, :, :].astype(np.float64) for k in range(3))
    return np.uint8((r * c[0] + g * c[1] + b * c[2] + 16 / 255.0) * 255)


def ssim_map(ya, yb):
    """metrics_model.ssim_sum's map, not its sum: [H - 10][W - 10]."""
    w = MM.window()
    a, b = ya.astype(np.float64), yb.astype(np.float64)
    view = np.lib.stride_tricks.sliding_window_view

    def filt(m):
        return np.einsum("ijkl,kl->ij", view(m, (MM.WINDOW, MM.WINDOW)), w, optimize=True)
    mu_a, mu_b = filt(a), filt(b)
    va, vb, cab = filt(a * a) - mu_a * mu_a, filt(b * b) - mu_b * mu_b, filt(a * b) - mu_a * mu_b
    c1, c2 = (MM.K1 * MM.PEAK) ** 2, (MM.K2 * MM.PEAK) ** 2
    return ((2 * mu_a * mu_b + c1) * (2 * cab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (va + vb + c2))


GARBAGE = 3.0e307          # roughly what the arena's pattern is as a double


def metrics_tiled_model(sr_u, hr_u, shave, variant=""):
    """tgsr_sr_metrics as the kernels do it - per 32 x 32 tile of the crop into a workspace, then per image in tile order - on uint8
    [B][3][H][W]: float64 [B][3].  tiles_swapped: tile -> (ty, tx) by tiles_y; shave_one_side: the crop keeps the right and lower
    border; centres_Hc5: window centres admitted at row Hc - 5 (the halo below the crop is zeros); ws_wrong_count: the workspace
    row of (image, tile) is b * tiles_x + tile; y_no_half: Y truncated without the + 0.5; ssey_unshaved: SSE-Y over the whole image."""
    B, _, H, W = sr_u.shape
    crop = (lambda x: x[..., shave:, shave:]) if variant == "shave_one_side" else (lambda x: MM.shaved(x, shave))
    a, b = crop(sr_u).astype(np.int64), crop(hr_u).astype(np.int64)
    ya, yb = rgb2y_model(crop(sr_u), variant), rgb2y_model(crop(hr_u), variant)
    Hc, Wc = a.shape[-2:]
    tiles_y, tiles_x = -(-Hc // 32), -(-Wc // 32)
    nt = tiles_y * tiles_x
    ws = np.full((B * nt + nt, 3), GARBAGE)
    d_rgb, d_y = ((a - b) ** 2).sum(1), (ya.astype(np.int64) - yb.astype(np.int64)) ** 2
    for bi in range(B):
        if variant == "centres_Hc5":
            pad = lambda y: np.concatenate([y[bi], np.zeros((1, Wc), np.uint8)])      # noqa: E731
            m = ssim_map(pad(ya), pad(yb))
        else:
            m = ssim_map(ya[bi], yb[bi])
        for tile in range(nt):
            ty, tx = divmod(tile, tiles_y if variant == "tiles_swapped" else tiles_x)
            ys, xs = slice(ty * 32, min(ty * 32 + 32, Hc)), slice(tx * 32, min(tx * 32 + 32, Wc))
            # window centre (cy, cx) is m[cy - 5, cx - 5]
            my = slice(max(ty * 32 - 5, 0), max(min(ty * 32 + 32 - 5, m.shape[0]), 0))
            mx = slice(max(tx * 32 - 5, 0), max(min(tx * 32 + 32 - 5, m.shape[1]), 0))
            ws[bi * (tiles_x if variant == "ws_wrong_count" else nt) + tile] = (d_rgb[bi][ys, xs].sum(), d_y[bi][ys, xs].sum(), m[my, mx].sum())
    out = np.zeros((B, 3))
    with np.errstate(over="ignore"):                              # sums of what a wrong index left unwritten
        for bi in range(B):
            for tile in range(nt):
                out[bi] += ws[bi * nt + tile]
    if variant == "ssey_unshaved":
        out[:, 1] = ((MM.rgb2y(sr_u).astype(np.int64) - MM.rgb2y(hr_u).astype(np.int64)) ** 2).reshape(B, -1).sum(1)
    return out


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


def _hp(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def _t(x):
    return torch.from_numpy(np.array(x, copy=True))


def _twice(a, call, outs):
    """The call, the arena's contract (inputs and tables bit-unchanged among it), the call again from the re-armed state with every
    workspace holding 1.5f in each word: the contract again and the same bits in every output."""
    M, _ = _lib()
    assert call() == M.OK
    a.check()
    got = [o.read().numpy().copy() for o in outs]
    a.rearm(ws_fill=1.5)
    assert call() == M.OK
    a.check()
    for g, o in zip(got, outs):
        assert g.tobytes() == o.read().numpy().tobytes(), "a second call gives other bits"
    return got


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    word = {1: np.uint8, 4: np.int32, 8: np.int64}[got.dtype.itemsize]
    diff = got.view(word) != ref.view(word)
    assert not diff.any(), "%s: %d of %d elements differ in their bits from the model, first at %s: %r, not %r" % (
        what, int(diff.sum()), diff.size, tuple(int(i) for i in np.argwhere(diff)[0]), got[diff][0], ref[diff][0])


def _place_image(a, x, off):
    """An image the gathers read, `off`: one byte (uint8) / one word (float32) off its alignment."""
    return a.place_input_u8(_t(x), lead=off) if x.dtype == np.uint8 else a.place_input(_t(x), skew=off)


def _aligned(r, n):
    return r is None or r.address % n == 0


def _run_gather(L, c, d8):
    img, img2 = gather_inputs(c)
    table, th, tw, mis = c["table"], c["th"], c["tw"], c["mis"]
    if d8:
        ref, ref2 = (EM.gather(x, table, th, tw, c["k0"], c["nk"]) if x is not None else None for x in (img, img2))
        block = lambda r, t: r[:, t]                                                    # noqa: E731
    else:
        ref, ref2 = (TM.gather(x, table, th, tw) if x is not None else None for x in (img, img2))
        block = lambda r, t: r[t]                                                       # noqa: E731
    a = Arena(DEV)
    xi = _place_image(a, img, int("img" in mis))
    x2 = _place_image(a, img2, int("img2" in mis)) if img2 is not None else None
    td = a.place_input(_t(dev_table(c)))
    outs, exps = [], []
    for k, r in enumerate((ref, ref2)):
        if r is None:
            outs.append(a.place_output(ref.shape, written=False))
            continue
        may, skew = np.ones(r.shape, bool), int(("out", "out2")[k] in mis)
        if c["bad"]:                                           # over a finite base: the skipped window's block keeps its bits
            base = _base(r.shape, k, 51)
            block(may, c["bad"][0])[...] = False
            exps.append(np.where(may, r, base))
            outs.append(a.place_masked(_t(base), _t(may), skew=skew))
        else:
            exps.append(r)
            outs.append(a.place_masked(r.shape, _t(may), skew=skew))
    in_align = 4 if c["dt"] == "u8" else 16
    flags = (int(c["W"] % 4 == 0 and _aligned(xi, in_align) and _aligned(x2, in_align)),
             int(tw % 4 == 0 and (not d8 or th % 4 == 0) and _aligned(outs[0], 16) and (img2 is None or _aligned(outs[1], 16))))
    assert flags == gather_flags(c, d8) == c["want"], (flags, c["want"])
    host = np.ascontiguousarray(table)
    o2 = outs[1].ptr if img2 is not None else None
    if d8:
        call = lambda: L.tgsr_d8_gather(xi.ptr, _p(x2), int(c["dt"] == "u8"), c["N"], c["H"], c["W"], _hp(host), td.ptr, len(table), th, tw,  # noqa: E731
                                        c["k0"], c["nk"], outs[0].ptr, o2, _stream())
    else:
        call = lambda: L.tgsr_tile_gather(xi.ptr, _p(x2), int(c["dt"] == "u8"), c["H"], c["W"], _hp(host), td.ptr, len(table), th, tw,       # noqa: E731
                                          outs[0].ptr, o2, _stream())
    got = _twice(a, call, outs[:len(exps)])
    for k, (g, e) in enumerate(zip(got, exps)):
        _same_bits(g, e, "%s out%s" % (c["name"], "2" if k else ""))
    assert np.array_equal(host, c["table"])


@pytest.mark.parametrize("row", _rows(GATHER), ids=row_id)
def test_tile_gather(row):
    assert row[1] == K_G[row[3]["dt"]]
    _run_gather(_lib()[1], row[3], d8=False)


@pytest.mark.parametrize("row", _rows(D8G), ids=row_id)
def test_d8_gather(row):
    assert row[1] == K_DG[row[3]["dt"]]
    _run_gather(_lib()[1], row[3], d8=True)


def _lists(srcs, dsts, strides, entries):
    n = len(entries)
    return ((ctypes.c_void_p * n)(*[r.address for r in srcs]), (ctypes.c_int64 * n)(*strides), (ctypes.c_void_p * n)(*[r.address for r in dsts]),
            (ctypes.c_int * n)(*[e["C"] for e in entries]), (ctypes.c_int * n)(*[e["s"] for e in entries]), (ctypes.c_int * n)(*[e["u8"] for e in entries]))


def _place_dst(a, e, prior, may, exp):
    if e["u8"]:
        return a.place_inout_u8(_t(prior), lead=e["doff"], may=_t(may), expect=_t(exp))
    return a.place_masked(_t(prior), _t(may), skew=e["doff"])


def _place_rows(a, x, stride, skew):
    """A batch [rows][block] with its rows `stride` elements apart, the gaps guarded."""
    rows = x.reshape(x.shape[0], -1)
    return a.place_input(_t(rows), bstride=stride if rows.shape[0] > 1 and stride != rows.shape[1] else None, skew=skew)


def run_stitch(L, c):
    table, th, tw = c["table"], c["th"], c["tw"]
    good = good_rows(c)
    a = Arena(DEV)
    td = a.place_input(_t(dev_table(c)))
    srcs, dsts, exps, strides = [], [], [], []
    for e, (tiles, prior) in zip(c["entries"], _stitch_inputs(c["name"])):
        block = tiles[0].size
        stride = 0 if c["zero_stride"] else block + e["extra"]
        exp = TM.stitch(tiles[good], table[good], th, prior.copy())
        may = owned_mask(table[good], e["s"], prior.shape)
        srcs.append(_place_rows(a, tiles, stride, e["soff"]))
        dsts.append(_place_dst(a, e, prior, may, exp))
        exps.append(exp)
        strides.append(stride)
    for e, s_, d_, st in zip(c["entries"], srcs, dsts, strides):
        flags = (int((e["s"] * tw) % 4 == 0 and s_.address % 16 == 0 and st % 4 == 0),
                 int((e["s"] * c["W"]) % 4 == 0 and d_.address % (4 if e["u8"] else 16) == 0))
        assert flags == stitch_flags(c, e), (c["name"], e, flags)
    host = np.ascontiguousarray(table)
    S, ST, D, Cs, Ss, U8 = _lists(srcs, dsts, strides, c["entries"])
    call = lambda: L.tgsr_tile_stitch(len(srcs), S, ST, D, Cs, Ss, U8, c["H"], c["W"], _hp(host), td.ptr, len(table), th, tw, _stream())  # noqa: E731
    for k, (g, e) in enumerate(zip(_twice(a, call, dsts), exps)):
        _same_bits(g, e, "%s entry %d" % (c["name"], k))
    assert np.array_equal(host, c["table"])


@pytest.mark.parametrize("row", _rows(STITCH), ids=row_id)
def test_tile_stitch(row):
    run_stitch(_lib()[1], row[3])


def merge_expected(c, e, src_a, src_b, prior):
    """ensemble_model.merge over the rows of the table the device copy keeps."""
    table, good, N, nk = c["table"], good_rows(c), c["N"], c["nk"]
    keep = lambda x, g: None if x is None else np.ascontiguousarray(                    # noqa: E731
        x.reshape((N, len(table), g) + x.shape[1:])[:, good].reshape((-1,) + x.shape[1:]))
    return EM.merge(keep(src_a, nk), keep(src_b, 4), table[good], c["th"], c["tw"], prior.copy())


def run_merge(L, c):
    table, th, tw, N, nk = c["table"], c["th"], c["tw"], c["N"], c["nk"]
    a = Arena(DEV)
    td = a.place_input(_t(dev_table(c)))
    As, Bs, dsts, exps, strides = [], [], [], [], []
    for e, (src_a, src_b, prior) in zip(c["entries"], _merge_inputs(c["name"])):
        stride = src_a[0].size + e["extra"]
        exp = merge_expected(c, e, src_a, src_b, prior)
        may = owned_mask(table[good_rows(c)], e["s"], prior.shape)
        As.append(_place_rows(a, src_a, stride, e["soff"]))
        Bs.append(_place_rows(a, src_b, stride, e["boff"]) if src_b is not None else None)
        dsts.append(_place_dst(a, e, prior, may, exp))
        exps.append(exp)
        strides.append(stride)
    for e, s_, b_, d_, st in zip(c["entries"], As, Bs, dsts, strides):
        flags = (int((e["s"] * tw) % 4 == 0 and (e["s"] * th) % 4 == 0 and s_.address % 16 == 0 and _aligned(b_, 16) and st % 4 == 0),
                 int((e["s"] * c["W"]) % 4 == 0 and d_.address % (4 if e["u8"] else 16) == 0))
        assert flags == merge_flags(c, e), (c["name"], e, flags)
    host = np.ascontiguousarray(table)
    n = len(As)
    S, ST, D, Cs, Ss, U8 = _lists(As, dsts, strides, c["entries"])
    B = (ctypes.c_void_p * n)(*[r.address for r in Bs]) if nk == 4 else None
    call = lambda: L.tgsr_d8_merge(n, S, B, ST, D, Cs, Ss, U8, nk, N, c["H"], c["W"], _hp(host), td.ptr, len(table), th, tw, _stream())  # noqa: E731
    for k, (g, e) in enumerate(zip(_twice(a, call, dsts), exps)):
        _same_bits(g, e, "%s entry %d" % (c["name"], k))
    assert np.array_equal(host, c["table"])


@pytest.mark.parametrize("row", _rows(D8M), ids=row_id)
def test_d8_merge(row):
    run_merge(_lib()[1], row[3])


def run_metrics(L, c, pair, leads=(0, 0)):
    """One call of tgsr_sr_metrics: ws has exactly tgsr_sr_metrics_ws_elems doubles, ws and out lie on 8 bytes and not on 16."""
    sr_f, hr_f, sr_u, hr_u = _metrics_inputs(c["name"])
    a = Arena(DEV)
    ops = [a.place_input(_t(f)) if kind == "f" else a.place_input_u8(_t(u), lead=lead)
           for kind, f, u, lead in zip(pair, (sr_f, hr_f), (sr_u, hr_u), leads)]
    n = L.tgsr_sr_metrics_ws_elems(c["B"], c["H"], c["W"], c["shave"])
    ty, tx = metrics_tiles(c)
    assert n == c["B"] * ty * tx * 3
    ws = a.place_ws(2 * n, skew=2)
    out = a.place_output((c["B"], 3), dtype=torch.float64, skew=2)
    assert ws.address % 16 == 8 and out.address % 16 == 8 and all(o.address % 4 == lead for o, k, lead in zip(ops, pair, leads) if k == "u")
    call = lambda: L.tgsr_sr_metrics(ops[0].ptr, int(pair[0] == "f"), ops[1].ptr, int(pair[1] == "f"), c["B"], c["H"], c["W"], c["shave"],  # noqa: E731
                                     ws.ptr, out.ptr, _stream())
    return _twice(a, call, [out])[0]


@pytest.mark.parametrize("row", _rows(METRICS), ids=row_id)
def test_sr_metrics(row):
    c = row[3]
    _, L = _lib()
    _sr_f, _hr_f, sr_u, hr_u = _metrics_inputs(c["name"])
    if c["same"]:
        windows = (c["hc"] - 10) * (c["wc"] - 10)
        for pair in (("f", "f"), ("u", "u")):
            got = run_metrics(L, c, pair)
            assert (got[:, :2] == 0).all() and (got[:, 2] == float(windows)).all(), got
        return
    first = run_metrics(L, c, PAIRS[0])
    worst = MM.check_rows(first, sr_u, hr_u, c["shave"], SSIM_TOL)
    print("UPSCALE_ABI metrics %s: worst |mean ssim - model| = %.3g" % (c["name"], worst))
    for pair in PAIRS[1:]:
        _same_bits(run_metrics(L, c, pair), first, "%s %s" % (c["name"], pair))
    if c["leads"]:
        for leads in ((1, 3), (2, 2), (3, 1)):
            _same_bits(run_metrics(L, c, ("u", "u"), leads), first, "%s leads %s" % (c["name"], leads))


def run_rgb_to_y(L, c, lead_in=0, lead_out=0):
    x = _y_input(c["B"], c["H"], c["W"])
    ref = MM.rgb2y(x)
    a = Arena(DEV)
    xin = a.place_input_u8(_t(x), lead=lead_in)
    out = a.place_output_u8(ref.shape, lead=lead_out, expect=_t(ref))
    assert xin.address % 4 == lead_in and out.address % 4 == lead_out
    got = _twice(a, lambda: L.tgsr_rgb_to_y_u8(xin.ptr, c["B"], c["H"], c["W"], out.ptr, _stream()), [out])[0]
    _same_bits(got, ref, "%s rgb +%d y +%d" % (c["name"], lead_in, lead_out))


@pytest.mark.parametrize("row", _rows(RGB2Y), ids=row_id)
def test_rgb_to_y(row):
    c = row[3]
    _, L = _lib()
    for lead_in in range(4 if c["leads"] else 1):
        for lead_out in range(4 if c["leads"] else 1):
            run_rgb_to_y(L, c, lead_in, lead_out)


# ----------------------------------------------------------------------------------------------------------------------------
# Refusals: every one a host-side return in front of the first launch - TGSR_EINVAL, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------
REF = dict(H=6, W=8, th=3, tw=3, N=2, C=2, s=2, n=2, B=2, MH=13, MW=14, shave=1)       # the valid small calls the refusals start from
REF_TABLE = np.array([(0, 0, 0, 2, 0, 2), (3, 4, 3, 5, 4, 6)], np.int32)          # 3 x 3 windows that own their first 2 x 2
NULL = object()


def _refusal_call(L, a, entry, **kw):
    """A call of `entry` on valid small operands with one thing wrong; the outputs are placed as operands the call must leave alone.
    Keywords: a pointer's name = NULL; a number's name = its value; row = (index, column, value) of the HOST table; tb = a table of
    that many rows (both copies); entry_null = "src" | "dst" | "srcB": element 1 of that list is NULL; lists: C1 / s1 / stride1 =
    the value of element 1."""
    H, W, th, tw, N = (kw.get(k, REF[k]) for k in ("H", "W", "th", "tw", "N"))
    table = REF_TABLE.copy()
    if "tb" in kw:
        table = np.repeat(REF_TABLE[:1], kw["tb"], axis=0) if kw["tb"] else REF_TABLE[:0].copy()
    Tb = kw.get("Tb", len(table))
    if "row" in kw:
        i, col, v = kw["row"]
        table[i, col] = v
    host = np.ascontiguousarray(table if len(table) else REF_TABLE)
    ptr = lambda name, r: None if kw.get(name) is NULL else (_hp(r) if isinstance(r, np.ndarray) else r.ptr)      # noqa: E731
    if entry in (GATHER, D8G):
        d8 = entry == D8G
        lead = (REF["N"],) if d8 else ()
        nk, k0 = kw.get("nk", 4), kw.get("k0", 0)
        img, img2 = (a.place_input(torch.randn(lead + (3, REF["H"], REF["W"]))) for _ in range(2))
        td = a.place_input(_t(host))
        oshape = lead + (2, 4 if d8 else 1, 3, REF["th"], REF["tw"])
        out, out2 = (a.place_output(oshape, written=False) for _ in range(2))
        if d8:
            return lambda: L.tgsr_d8_gather(ptr("img", img), ptr("img2", img2), 0, N, H, W, ptr("table_host", host), ptr("table_dev", td), Tb, th, tw,
                                            k0, nk, ptr("out", out), ptr("out2", out2), _stream())
        return lambda: L.tgsr_tile_gather(ptr("img", img), ptr("img2", img2), 0, H, W, ptr("table_host", host), ptr("table_dev", td), Tb, th, tw,
                                          ptr("out", out), ptr("out2", out2), _stream())
    if entry in (STITCH, D8M):
        d8 = entry == D8M
        nk = kw.get("nk", 4)
        n, C, s = REF["n"], REF["C"], REF["s"]
        block = C * s * REF["th"] * s * REF["tw"]
        rows = 2 * (REF["N"] * 8 if d8 else 1)
        srcs = [a.place_input(torch.randn(rows, block)) for _ in range(n)]
        srcb = [a.place_input(torch.randn(rows, block)) for _ in range(n)]
        td = a.place_input(_t(host))
        dsts = [a.place_output(((REF["N"],) if d8 else ()) + (C, s * REF["H"], s * REF["W"]), written=False) for _ in range(n)]
        addr = lambda rs, which: (ctypes.c_void_p * n)(*[None if (k == 1 and kw.get("entry_null") == which) else r.address  # noqa: E731
                                                         for k, r in enumerate(rs)])
        S, B, D = addr(srcs, "src"), addr(srcb, "srcB"), addr(dsts, "dst")
        ST = (ctypes.c_int64 * n)(block, kw.get("stride1", block))
        Cs, Ss, U8 = (ctypes.c_int * n)(C, kw.get("C1", C)), (ctypes.c_int * n)(s, kw.get("s1", s)), (ctypes.c_int * n)(0, 0)
        lst = lambda name, v: None if kw.get(name) is NULL else v                       # noqa: E731
        nn = kw.get("n", n)
        if d8:
            B = None if (kw.get("srcB") is NULL or (nk == 8 and not kw.get("keep_srcB"))) else B
            return lambda: L.tgsr_d8_merge(nn, lst("src", S), B, lst("src_stride", ST), lst("dst", D), lst("C", Cs), lst("scale", Ss),
                                           lst("out_u8", U8), nk, N, H, W, ptr("table_host", host), ptr("table_dev", td), Tb, th, tw, _stream())
        return lambda: L.tgsr_tile_stitch(nn, lst("src", S), lst("src_stride", ST), lst("dst", D), lst("C", Cs), lst("scale", Ss), lst("out_u8", U8),
                                          H, W, ptr("table_host", host), ptr("table_dev", td), Tb, th, tw, _stream())
    if entry == METRICS:
        B, MH, MW, shave = (kw.get(k, REF[k]) for k in ("B", "MH", "MW", "shave"))
        sr, hr = (a.place_input(torch.randn(REF["B"], 3, REF["MH"], REF["MW"])) for _ in range(2))
        n = L.tgsr_sr_metrics_ws_elems(REF["B"], REF["MH"], REF["MW"], REF["shave"])
        assert n == REF["B"] * 3
        ws, out = a.place_output((2 * n,), written=False), a.place_output((REF["B"], 3), dtype=torch.float64, written=False)
        if any(k in kw for k in ("B", "MH", "MW", "shave")):
            assert L.tgsr_sr_metrics_ws_elems(B, MH, MW, shave) == 0
        return lambda: L.tgsr_sr_metrics(ptr("sr", sr), 1, ptr("hr", hr), 1, B, MH, MW, shave, ptr("ws", ws), ptr("out", out), _stream())
    assert entry == RGB2Y
    B, H, W = (kw.get(k, v) for k, v in (("B", 2), ("H", 3), ("W", 5)))
    rgb, y = a.place_input_u8(torch.arange(90, dtype=torch.uint8)), a.place_output_u8((30,), written=False)
    return lambda: L.tgsr_rgb_to_y_u8(ptr("rgb", rgb), B, H, W, ptr("y", y), _stream())


def _table_refusals():
    """What tile_args_ok / d8_args_ok and tile_desc_ok refuse, each alone: keyword sets for a call over REF and REF_TABLE."""
    H, W, th, tw = REF["H"], REF["W"], REF["th"], REF["tw"]
    out = [("table_host-null", dict(table_host=NULL)), ("table_dev-null", dict(table_dev=NULL)), ("Tb-0", dict(tb=0, Tb=0)),
           ("Tb-negative", dict(Tb=-1)), ("Tb-65536", dict(tb=65536)), ("H-0", dict(H=0)), ("W-0", dict(W=0)), ("H-2^20+1", dict(H=(1 << 20) + 1)),
           ("W-2^20+1", dict(W=(1 << 20) + 1)), ("th-0", dict(th=0)), ("tw-0", dict(tw=0)), ("th-above-H", dict(th=H + 1)),
           ("tw-above-W", dict(tw=W + 1)), ("th-4097", dict(th=4097, H=5000)), ("tw-4097", dict(tw=4097, W=5000))]
    # row 1 of REF_TABLE is (3, 4, 3, 5, 4, 6) with th = tw = 3 in 6 x 8
    out += [("row-" + name, dict(row=(1, col, v))) for name, col, v in (
        ("y0-negative", 0, -1), ("x0-negative", 1, -1), ("y0-above-H-th", 0, H - th + 1), ("x0-above-W-tw", 1, W - tw + 1),
        ("oy0-below-y0", 2, 2), ("oy1-is-oy0", 3, 3), ("oy1-below-oy0", 3, 2), ("oy1-above-y0+th", 3, 7),
        ("ox0-below-x0", 4, 3), ("ox1-is-ox0", 5, 4), ("ox1-below-ox0", 5, 3), ("ox1-above-x0+tw", 5, 8))]
    return out


def refusals():
    """(name, entry point, keywords of _refusal_call).  Every one answers TGSR_EINVAL in front of the first launch
    (tests/test_upscale_abi_host.py runs them on host memory, where a launch could only fail)."""
    out = []
    for e in (GATHER, D8G):
        out += [(e[5:] + "-" + n, e, kw) for n, kw in _table_refusals()]
        out += [(e[5:] + "-" + n + "-null", e, {n: NULL}) for n in ("img", "out", "img2", "out2")]
    out += [("d8_gather-" + n, D8G, kw) for n, kw in (
        ("N-0", dict(N=0)), ("N-4097", dict(N=4097)), ("k0-1", dict(k0=1)), ("k0-4-nk-8", dict(k0=4, nk=8)), ("nk-2", dict(nk=2)), ("nk-0", dict(nk=0)),
        ("k0-negative", dict(k0=-4)), ("nk-8-th-not-tw", dict(nk=8, th=2)))]
    lists = [(n + "-null", {n: NULL}) for n in ("src", "src_stride", "dst", "C", "scale", "out_u8")]
    lists += [("n-0", dict(n=0)), ("n-13", dict(n=13)), ("n-negative", dict(n=-1)), ("src-entry-null", dict(entry_null="src")),
              ("dst-entry-null", dict(entry_null="dst")), ("C-0", dict(C1=0)), ("C-65536", dict(C1=65536)), ("s-0", dict(s1=0)), ("s-65", dict(s1=65)),
              ("stride-below-block", dict(stride1=REF["C"] * REF["s"] ** 2 * REF["th"] * REF["tw"] - 1))]
    for e in (STITCH, D8M):
        out += [(e[5:] + "-" + n, e, kw) for n, kw in _table_refusals() + lists]
    out += [("d8_merge-" + n, D8M, kw) for n, kw in (
        ("N-0", dict(N=0)), ("N-4097", dict(N=4097)), ("nk-2", dict(nk=2)), ("nk-8-th-not-tw", dict(nk=8, th=2)), ("nk-4-srcB-null", dict(srcB=NULL)),
        ("nk-4-srcB-entry-null", dict(entry_null="srcB")), ("nk-8-with-srcB", dict(nk=8, keep_srcB=True)),
        ("stride-0-Tb-1", dict(tb=1, stride1=0)))]
    out += [("sr_metrics-" + n, METRICS, kw) for n, kw in (
        ("sr-null", dict(sr=NULL)), ("hr-null", dict(hr=NULL)), ("ws-null", dict(ws=NULL)), ("out-null", dict(out=NULL)), ("B-0", dict(B=0)),
        ("B-65536", dict(B=65536)), ("shave-negative", dict(shave=-1)), ("crop-10-high", dict(MH=12)),
        ("crop-10-wide", dict(MW=12)), ("H-0", dict(MH=0, shave=0)), ("W-0", dict(MW=0, shave=0)))]
    out += [("rgb_to_y_u8-" + n, RGB2Y, kw) for n, kw in (
        ("rgb-null", dict(rgb=NULL)), ("y-null", dict(y=NULL)), ("B-0", dict(B=0)), ("H-0", dict(H=0)), ("W-0", dict(W=0)), ("B-negative", dict(B=-1)),
        ("H-negative", dict(H=-1)), ("W-negative", dict(W=-1)))]
    return out


def test_refusals():
    """Every NULL, every count, size, scale and stride outside its range, every rule of the host table, the variant groups that do
    not exist, srcB against nk: TGSR_EINVAL, no byte written.  The one stitch call with src_stride < block that IS accepted (Tb == 1)
    is a case of test_tile_stitch; tgsr_d8_merge refuses it (stride-0-Tb-1)."""
    M, L = _lib()
    for name, entry, kw in refusals():
        a = Arena(DEV, guard=64)
        call = _refusal_call(L, a, entry, **kw)
        a.buffer()
        assert call() == M.EINVAL, name
        v = a.violations()
        assert not v, name + ": " + "; ".join(v)
