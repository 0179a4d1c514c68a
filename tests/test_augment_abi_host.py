"""CPU: what tests/test_hip_augment_abi.py rests on - its tables, its numpy models and its refusals - checked without a GPU.

The GPU file calls tgsr_resize_coeffs, tgsr_augment_ws_elems and tgsr_augment_u8 (tgsr_amd/csrc/tgsr_augment.hip) through ctypes with
every device operand inside one guarded arena (tests/arena.py) and compares every output BIT-EXACT with the models below.  They live
here so that the GPU file imports no Pillow and no scipy:

  * `augment_model`: crop, oracle.tgsr_oracle_io.resize_bilinear, window, mirror - test_hip_augment._oracle on the packed buffer;
  * `kernel_model`: the same bytes from the kernel's own structure (flat addresses into `packed`, the window's rows of the two
    coefficient tables, horizontal pass, rounded intermediate, vertical pass with the kAugRows clip, mirrored store), and with
    `variant` one of V_AUGMENT a wrong kernel.  The variant-free form equals augment_model on every row.

COEFF_TABLE / AUG_TABLE hold one row per case and one refusal row (case None) per entry point; `catch` names the wrong kernels whose
output differs from the right one on that row's input (test_each_row_catches_what_it_lists, test_every_variant_is_caught).

Here: the constants and formulas against the source text; every refusal on host memory (the entry returns before any HIP call);
the cases are the ones their rows describe; the LDS bound of augment_u8_kernel (it clips nrows at kAugRows silently) from
IO.resize_coeffs; where Pillow is importable, every row's model output against Pillow's own crop / resize / crop / transpose.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from arena import Arena
from oracle import tgsr_oracle_io as IO

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgsr_amd", "csrc")
COEFFS, WS_ELEMS, AUGMENT = "tgsr_resize_coeffs", "tgsr_augment_ws_elems", "tgsr_augment_u8"
DESC, MAX_TAPS, WS_ROW, TH, TW, ROWS, MAX_SIDE, MAX_OUT, MAX_RATIO = 12, 33, 35, 8, 64, 148, 4096, 65536, 16
NULL = object()
FILL = 0xA5          # what a wrong kernel of the model leaves where it writes nothing: the arena's byte

V_AUGMENT = ("no_window_origin", "mirror_first", "vertical_first", "no_rounding", "crop_origin", "taps_WH", "pitch_crop", "no_offset",
             "mirror_rows", "cols64_dropped", "rows_cut8")


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream(dev):
    if torch.device(dev).type != "cuda":
        return None
    from tgsr_amd import ops
    return ops._stream()


def _hp(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def _t(x):
    return torch.from_numpy(np.array(x, copy=True))


def ksize(i, o):
    """Pillow's 2 ceil(max(in / out, 1)) + 1."""
    return 2 * int(np.ceil(max(i / o, 1.0))) + 1


@functools.lru_cache(maxsize=None)
def coeffs(i, o):
    b, k = IO.resize_coeffs(i, o)
    b.setflags(write=False)
    k.setflags(write=False)
    return b, k


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_resize_coeffs
# ----------------------------------------------------------------------------------------------------------------------------
def _cc(i, o, why, dirty=False, skew=0):
    return dict(name="%d-to-%d%s" % (i, o, "-dirty" if dirty else ""), i=i, o=o, dirty=dirty, skew=skew), why


R_COEFFS = ("bounds or taps NULL; in_size or out_size outside [1, 65536]; in_size > 16 out_size; ksize not Pillow's: TGSR_EINVAL; bounds or "
            "taps off 4 bytes: TGSR_EUNSUPPORTED: refused, nothing launched or written")
COEFF_TABLE = [(COEFFS, "resize_coeffs_kernel", why, c) for c, why in (
    _cc(1, 1, "one output, one tap of 2^22"), _cc(1, 16, "every output reads the one input"), _cc(16, 1, "33 taps, a single output"),
    _cc(3, 7, "up, odd sizes", skew=1), _cc(7, 3, "down, odd sizes", skew=3), _cc(304, 256, "the training reduction: two workgroups"),
    _cc(256, 304, "up: two workgroups, 48 lanes in the second", skew=2), _cc(255, 257, "two workgroups, one lane in the second"),
    _cc(4096, 256, "exactly 16x"), _cc(65536, 4096, "both limits at once: 4096 x 33 ints"),
    _cc(7, 3, "a second trip into outputs that hold other numbers: every word written, the zeros behind the count too", dirty=True))
] + [(COEFFS, "no instance", R_COEFFS, None)]


def coeff_refusals():
    """(name, keywords, code name).  The call they change is 7 -> 3 with ksize 7."""
    out = [("bounds-null", dict(bounds=NULL)), ("taps-null", dict(taps=NULL)), ("in-0", dict(i=0, k=3)), ("out-0", dict(o=0, k=3)),
           ("in-65537", dict(i=65537, o=65537, k=3)), ("out-65537", dict(i=65536, o=65537, k=3)), ("33-to-2", dict(i=33, o=2, k=35)),
           ("ksize-plus-2", dict(k=9)), ("ksize-minus-2", dict(k=5)), ("in-negative", dict(i=-1, k=3))]
    out = [(n, kw, "EINVAL") for n, kw in out]
    return out + [("bounds-off-4", dict(off=("bounds", 2)), "EUNSUPPORTED"), ("taps-off-4", dict(off=("taps", 1)), "EUNSUPPORTED")]


def coeff_refusal_call(L, a, dev, **kw):
    i, o, k = kw.get("i", 7), kw.get("o", 3), kw.get("k", 7)
    bounds = a.place_output((3, 2), dtype=torch.int32, written=False)
    taps = a.place_output((3, 7), dtype=torch.int32, written=False)
    ptr = lambda name, r: None if kw.get(name) is NULL else ctypes.c_void_p(r.address + (kw["off"][1] if kw.get("off", ("",))[0] == name else 0))  # noqa: E731
    return lambda: L.tgsr_resize_coeffs(i, o, k, ptr("bounds", bounds), ptr("taps", taps), _stream(dev))


# ----------------------------------------------------------------------------------------------------------------------------
# tgsr_augment_u8: the cases
# ----------------------------------------------------------------------------------------------------------------------------
def _ac(name, S, images, leads, why, catch, order=None, bad=None):
    """images: ((H, W), (x1, y1, x2, y2, oh, ow, top, left, flip)) in packing order (`order`: the images of the row it permutes);
    leads = (packed, out) bytes off a word; bad = (image, column, value) of table_dev only."""
    return dict(name=name, S=S, images=tuple(images), leads=leads, order=order, bad=bad), why, tuple(catch)


_RAG = (((5, 7), (1, 0, 7, 5, 9, 11, 2, 3, 1)), ((6, 5), (0, 1, 5, 6, 8, 6, 0, 0, 0)), ((3, 3), (0, 0, 3, 3, 6, 12, 0, 5, 1)))
_GEOM = ("no_window_origin", "mirror_first", "vertical_first", "no_rounding", "crop_origin", "taps_WH", "pitch_crop", "mirror_rows")
AUG_CASES = (
    _ac("identity", 5, (((9, 11), (2, 1, 9, 8, 7, 7, 1, 2, 0)),), (1, 3),
        "S = 5, oh == y2 - y1 and ow == x2 - x1: both passes have the taps (2^22, 0); one partial 8 x 64 tile",
        ("no_window_origin", "crop_origin", "pitch_crop", "taps_WH")),
    _ac("remainders", 70, (((200, 71), (3, 10, 70, 187, 75, 140, 5, 33, 1)), ((75, 333), (11, 1, 330, 74, 151, 90, 40, 20, 0))), (2, 1),
        "S = 70: two column tiles (64 + 6) and nine row tiles (8 x 8 + 6); boxes strictly inside; up on one axis and down on the other, both "
        "ways round; both flips", _GEOM + ("no_offset", "cols64_dropped", "rows_cut8")),
    _ac("down16", 9, (((150, 150), (3, 4, 147, 148, 9, 9, 0, 0, 1)),), (3, 2),
        "S = 9: a second row tile of one row; crop 144 x 144 -> 9 x 9: 33 taps, the LDS intermediate at its tallest",
        ("vertical_first", "no_rounding", "crop_origin", "taps_WH", "pitch_crop", "mirror_rows", "rows_cut8")),
    _ac("up17", 64, (((4, 4), (0, 0, 4, 4, 68, 68, 4, 4, 0)), ((4, 4), (0, 0, 4, 4, 68, 68, 0, 0, 1))), (0, 0),
        "source 4 x 4, oh = ow = 68, S = 64: the far window (4, 4) and the near one (0, 0)", ("no_window_origin", "mirror_first", "no_offset", "mirror_rows")),
    _ac("one-pixel", 3, (((1, 1), (0, 0, 1, 1, 3, 3, 0, 0, 1)),), (3, 1), "H = W = 1, oh = ow = S = 3: every output is the one pixel", ()),
    # one-pixel catches no wrong kernel of the list (every index is 0): it stays for the smallest extent of every operand
    _ac("tall", 8, (((4096, 1), (0, 0, 1, 4096, 65536, 8, 65536 - 8, 0, 0)),), (1, 0),
        "H = 4096, W = 1, oh = 65536, ow = S = 8, top = 65536 - 8: the fp64 centre at the largest index the contract admits",
        ("no_window_origin",)),
    _ac("ragged", 3, _RAG, (2, 3), "B = 3, offsets 0, 105, 195: the second and third odd; the last image ends exactly at nbytes; mixed flips",
        _GEOM + ("no_offset",)),
    _ac("ragged-reversed", 3, _RAG[::-1], (0, 1), "the same three images packed in reverse order: the same outputs", _GEOM + ("no_offset",), order=(2, 1, 0)),
    _ac("skipped", 3, _RAG, (1, 2), "table_dev row 1 has flip = 2 (table_host is valid): !aug_desc_ok: image 1 keeps its prior bytes, a kernel "
        "that fails to skip still reads only inside packed", _GEOM + ("no_offset",), bad=(1, 11, 2)),
    _ac("second-trip", 9, (((40, 30), (2, 3, 29, 38, 12, 50, 3, 20, 1)),), (0, 3), "run twice, ws refilled with a finite value in between: the same bytes",
        _GEOM),
)
R_AUGMENT = ("packed, table_host, table_dev, ws or out NULL; nbytes outside [1, 2^31); B outside [1, 65535]; S outside [1, 4096]; a host "
             "descriptor that fails aug_desc_ok: TGSR_EINVAL; table_host, table_dev or ws off 4 bytes: TGSR_EUNSUPPORTED: refused, nothing "
             "launched or written")
AUG_TABLE = [(AUGMENT, "augment_coeffs_kernel + augment_u8_kernel", why, c, catch) for c, why, catch in AUG_CASES] + [
    (AUGMENT, "no instance", R_AUGMENT, None, ())]


def row_id(r):
    return r[3]["name"]


def rows(table):
    return [r for r in table if r[3] is not None]


@functools.lru_cache(maxsize=None)
def _pixels(H, W, seed):
    a = np.random.default_rng([17, H, W, seed]).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def aug_inputs(c):
    """(packed uint8 [nbytes], table int32 [B][12]): the images back to back, nothing behind the last."""
    ids = c["order"] or tuple(range(len(c["images"])))
    srcs = [_pixels(H, W, i) for i, ((H, W), _d) in zip(ids, c["images"])]
    offs = np.cumsum([0] + [s.size for s in srcs])
    table = np.array([(int(o), H, W) + tuple(d) for o, ((H, W), d) in zip(offs, c["images"])], np.int32)
    return np.concatenate([s.reshape(-1) for s in srcs]), table


def dev_table(c, table):
    t = table.copy()
    if c["bad"]:
        t[c["bad"][0], c["bad"][1]] = c["bad"][2]
    return t


def desc_ok(d, S, nbytes):
    """aug_desc_ok, restated."""
    off, H, W, x1, y1, x2, y2, oh, ow, top, left, flip = (int(v) for v in d)
    if off < 0 or H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE or off + 3 * H * W > nbytes:
        return False
    if x1 < 0 or x2 <= x1 or x2 > W or y1 < 0 or y2 <= y1 or y2 > H:
        return False
    if oh < S or ow < S or oh > MAX_OUT or ow > MAX_OUT or top < 0 or top > oh - S or left < 0 or left > ow - S:
        return False
    return x2 - x1 <= MAX_RATIO * ow and y2 - y1 <= MAX_RATIO * oh and flip in (0, 1)


# ----------------------------------------------------------------------------------------------------------------------------
# The models
# ----------------------------------------------------------------------------------------------------------------------------
def augment_model(packed, d, S):
    """One image [3][S][S]: crop, IO.resize_bilinear, window, mirror."""
    off, H, W, x1, y1, x2, y2, oh, ow, top, left, flip = (int(v) for v in d)
    src = packed[off:off + 3 * H * W].reshape(H, W, 3)
    crop = np.ascontiguousarray(src[y1:y2, x1:x2].transpose(2, 0, 1))
    r = IO.resize_bilinear(crop, oh, ow)[..., top:top + S, left:left + S]
    return np.ascontiguousarray(r[..., ::-1] if flip else r)


def _sums(a, bounds, taps, axis):
    """sum_t a[first + t] taps[t] along `axis`, exact in int64."""
    a = np.moveaxis(a, axis, 0)
    out = np.zeros((len(bounds),) + a.shape[1:], np.int64)
    for i, (f, n) in enumerate(np.asarray(bounds).tolist()):
        if n > 0:
            out[i] = (a[f:f + n] * taps[i, :n].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))).sum(0)
    return np.moveaxis(out, 0, axis)


def _clip8(ss, bits=22):
    return np.clip((ss + (1 << (bits - 1))) >> bits, 0, 255)


def kernel_model(packed, d, S, variant=""):
    """augment_u8_kernel for one image, and its wrong kernels:
    no_window_origin  the coefficient index is the window's own (top, left left out);   mirror_first  mirror, then window;
    vertical_first    the vertical pass first;        no_rounding   no uint8 between the passes;
    crop_origin       (x1, y1) ignored;               taps_WH       taps from (W, H), not the crop's size;
    pitch_crop        row pitch x2 - x1, not W;       no_offset     the byte offset ignored;
    mirror_rows       the rows mirrored, not the columns;   cols64_dropped  window columns from 64 on not written;
    rows_cut8         the intermediate of a row tile cut at 8 source rows (kAugRows = 8)."""
    off, H, W, x1, y1, x2, y2, oh, ow, top, left, flip = (int(v) for v in d)
    cw, ch = x2 - x1, y2 - y1
    hb, hk = coeffs(W if variant == "taps_WH" else cw, ow)
    vb, vk = coeffs(H if variant == "taps_WH" else ch, oh)
    if variant == "no_window_origin":
        top = left = 0
    if variant == "mirror_first" and flip:
        left = ow - left - S
    hb, hk, vb, vk = hb[left:left + S], hk[left:left + S], vb[top:top + S].copy(), vk[top:top + S]
    cut = 8 if variant == "rows_cut8" else ROWS
    for r0 in range(0, S, TH):                                       # the LDS intermediate holds `cut` source rows of a row tile
        last = min(r0 + TH, S) - 1
        rbase = int(vb[r0, 0])
        nrows = min(int(vb[last, 0] + vb[last, 1]) - rbase, cut)
        for r in range(r0, last + 1):
            vb[r, 1] = max(0, min(int(vb[r, 1]), nrows - (int(vb[r, 0]) - rbase)))
    if variant == "crop_origin":
        x1 = y1 = 0
    if variant == "no_offset":
        off = 0
    pitch = cw if variant == "pitch_crop" else W
    R, Cn = int((vb[:, 0] + vb[:, 1]).max()), int((hb[:, 0] + hb[:, 1]).max())
    idx = off + ((y1 + np.arange(R)[None, :, None]) * pitch + x1 + np.arange(Cn)[None, None, :]) * 3 + np.arange(3)[:, None, None]
    g = packed[np.minimum(idx, packed.size - 1)].astype(np.int64)    # a wrong kernel's reads are clamped into the buffer
    if variant == "vertical_first":
        out = _clip8(_sums(_clip8(_sums(g, vb, vk, 1)), hb, hk, 2))
    elif variant == "no_rounding":
        out = _clip8(_sums(_sums(g, hb, hk, 2), vb, vk, 1), 44)
    else:
        out = _clip8(_sums(_clip8(_sums(g, hb, hk, 2)), vb, vk, 1))
    out = out.astype(np.uint8)
    if flip:
        out = out[:, ::-1] if variant == "mirror_rows" else out[..., ::-1]
    out = np.ascontiguousarray(out)
    if variant == "cols64_dropped":
        out[..., 64:] = FILL
    return out


@functools.lru_cache(maxsize=None)
def expected(name, variant=""):
    """[B][3][S][S] of a row (every image, the skipped one too)."""
    c = next(r[3] for r in rows(AUG_TABLE) if r[3]["name"] == name)
    packed, table = aug_inputs(c)
    out = np.stack([kernel_model(packed, d, c["S"], variant) if variant else augment_model(packed, d, c["S"]) for d in table])
    out.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# Refusals of tgsr_augment_u8: a valid three-image call with one thing wrong
# ----------------------------------------------------------------------------------------------------------------------------
REF_S = 3


def ref_inputs():
    c = next(r[3] for r in rows(AUG_TABLE) if r[3]["name"] == "ragged")
    return aug_inputs(c)


def aug_refusals():
    packed, table = ref_inputs()
    nb = packed.size
    out = [(n + "-null", {n: NULL}) for n in ("packed", "table_host", "table_dev", "ws", "out")]
    out += [("nbytes-0", dict(nbytes=0)), ("nbytes-2^31", dict(nbytes=1 << 31)), ("B-0", dict(B=0)), ("B-65536", dict(B=65536)), ("S-0", dict(S=0)),
            ("S-4097", dict(S=4097)), ("nbytes-one-short", dict(nbytes=nb - 1))]
    # image 1 is 6 x 5 at offset 105: (105, 6, 5, 0, 1, 5, 6, 8, 6, 0, 0, 0), S = 3
    out += [("row-" + n, dict(row=(1, col, v))) for n, col, v in (
        ("off-negative", 0, -1), ("off-past-the-end", 0, nb - 89), ("H-0", 1, 0), ("H-4097", 1, 4097), ("W-0", 2, 0), ("W-4097", 2, 4097),
        ("x1-negative", 3, -1), ("y1-negative", 4, -1), ("x2-above-W", 5, 6), ("x2-is-x1", 5, 0), ("y2-above-H", 6, 7), ("y2-is-y1", 6, 1),
        ("oh-below-S", 7, 2), ("oh-65537", 7, 65537), ("ow-below-S", 8, 2), ("ow-65537", 8, 65537), ("top-negative", 9, -1),
        ("top-above-oh-S", 9, 6), ("left-negative", 10, -1), ("left-above-ow-S", 10, 4), ("flip-2", 11, 2), ("flip-negative", 11, -1))]
    out = [(n, kw, "EINVAL") for n, kw in out]
    out += [("row-ratio-above-16", dict(row17=True), "EINVAL")]
    return out + [(n + "-off-4", dict(off=(n, 2)), "EUNSUPPORTED") for n in ("table_host", "table_dev", "ws")]


def ref_table(kw):
    packed, table = ref_inputs()
    table = table.copy()
    if "row" in kw:
        i, col, v = kw["row"]
        table[i, col] = v
    return table


def aug_refusal_call(L, a, dev, **kw):
    packed, _ = ref_inputs()
    table = ref_table(kw)
    if kw.get("row17"):                                              # a taller image 1 whose crop of 49 rows goes to oh = 3: 49 > 16 * 3
        tall = np.zeros(3 * 49 * 5, np.uint8)
        packed = np.concatenate([packed, tall])
        table[1] = (packed.size - tall.size, 49, 5, 0, 0, 5, 49, 3, 3, 0, 0, 0)
    B, S = kw.get("B", len(table)), kw.get("S", REF_S)
    nbytes = kw.get("nbytes", packed.size)
    host = np.zeros(len(table) * DESC + 1, np.int32)                 # one word to spare: the misaligned host table stays inside it
    host[:table.size] = table.reshape(-1)
    pk = a.place_input_u8(_t(packed), lead=1)
    td = a.place_input(_t(np.concatenate([table.reshape(-1), np.zeros(1, np.int32)])))
    n = L.tgsr_augment_ws_elems(len(table), REF_S)
    assert n == len(table) * 2 * WS_ROW * REF_S
    ws = a.place_output((n + 1,), dtype=torch.int32, written=False)
    out = a.place_output_u8((len(table), 3, REF_S, REF_S), written=False, lead=2)
    addr = {"packed": pk.address, "table_host": host.ctypes.data, "table_dev": td.address, "ws": ws.address, "out": out.address}
    ptr = lambda name: None if kw.get(name) is NULL else ctypes.c_void_p(addr[name] + (kw["off"][1] if kw.get("off", ("",))[0] == name else 0))  # noqa: E731
    call = lambda: L.tgsr_augment_u8(ptr("packed"), nbytes, ptr("table_host"), ptr("table_dev"), B, S, ptr("ws"), ptr("out"), _stream(dev))  # noqa: E731
    call.keep = host
    return call


def run_refusals(dev):
    """Every refusal of the two entry points on `dev`: the code, and not one word of the arena changed."""
    M, L = _lib()
    for name, kw, code in coeff_refusals():
        a = Arena(dev, guard=64)
        call = coeff_refusal_call(L, a, dev, **kw)
        a.buffer()
        assert call() == getattr(M, code), "resize_coeffs-" + name
        v = a.violations()
        assert not v, name + ": " + "; ".join(v)
    for name, kw, code in aug_refusals():
        a = Arena(dev, guard=64)
        call = aug_refusal_call(L, a, dev, **kw)
        a.buffer()
        assert call() == getattr(M, code), "augment_u8-" + name
        v = a.violations()
        assert not v, name + ": " + "; ".join(v)


# ============================================================================================================================
# The host tests
# ============================================================================================================================
TEXT = open(os.path.join(CSRC, "tgsr_augment.hip")).read()


def _const(name):
    m = re.search(r"\b%s = ([^;,]+)[;,]" % name, TEXT)
    assert m, name
    return m.group(1).strip()


def test_the_tables_against_the_source():
    assert _const("kAugDesc") == str(DESC) and _const("kAugMaxSide") == str(MAX_SIDE) and _const("kAugMaxOut") == str(MAX_OUT)
    assert _const("kAugMaxRatio") == str(MAX_RATIO) and _const("kAugMaxTaps") == "2 * kAugMaxRatio + 1" and MAX_TAPS == 2 * MAX_RATIO + 1
    assert _const("kAugWsRow") == "2 + kAugMaxTaps" and WS_ROW == 2 + MAX_TAPS
    assert "constexpr int kAugTH = %d, kAugTW = %d;" % (TH, TW) in TEXT
    assert _const("kAugRows") == "kAugMaxRatio * (kAugTH - 1) + kAugMaxTaps + 3" and ROWS == MAX_RATIO * (TH - 1) + MAX_TAPS + 3
    assert "return (int64_t)B * 2 * kAugWsRow * S;" in TEXT and "if (B < 1 || S < 1) return 0;" in TEXT
    launches = re.findall(r"hipLaunchKernelGGL\(([a-z_0-9]+)", TEXT)
    assert sorted(launches) == ["augment_coeffs_kernel", "augment_u8_kernel", "resize_coeffs_kernel"]
    named = " ".join(r[1] for r in COEFF_TABLE + AUG_TABLE)
    assert all(k in named for k in launches)
    for table, entry in ((COEFF_TABLE, COEFFS), (AUG_TABLE, AUGMENT)):
        assert {r[0] for r in table} == {entry}
        assert [r[1] for r in table if r[3] is None] == ["no instance"] and "refused" in table[-1][2]
        names = [row_id(r) for r in rows(table)]
        assert len(set(names)) == len(names)
    M, L = _lib()
    assert len(M.SIGNATURES[COEFFS][1]) == 6 and len(M.SIGNATURES[AUGMENT][1]) == 9 and len(M.SIGNATURES[WS_ELEMS][1]) == 2
    for B, S in ((1, 1), (3, 5), (2, 70), (65535, 4096)):
        assert L.tgsr_augment_ws_elems(B, S) == B * 2 * WS_ROW * S
    for B, S in ((0, 5), (5, 0), (-1, 5), (5, -1), (0, 0)):
        assert L.tgsr_augment_ws_elems(B, S) == 0
    # what the launchers refuse, as the refusal rows say it
    for snippet in ("!bounds || !taps || in_size < 1 || out_size < 1 || in_size > kAugMaxOut || out_size > kAugMaxOut",
                    "(int64_t)in_size > (int64_t)kAugMaxRatio * out_size || ksize != aug_ksize(in_size, out_size)",
                    "!packed || !table_host || !table_dev || !ws || !out || nbytes < 1 || nbytes > INT32_MAX",
                    "B < 1 || B > 65535 || S < 1 || S > kAugMaxSide", "if (!aug_aligned4(bounds, taps)) return TGSR_EUNSUPPORTED;",
                    "if (!aug_aligned4(table_host, table_dev, ws)) return TGSR_EUNSUPPORTED;",
                    "if (!aug_desc_ok(d, S, nbytes)) return;"):
        assert snippet in TEXT, snippet
    header = open(os.path.join(CSRC, "..", "..", "include", "tgsr_hip.h")).read()
    for words in ("may start at any byte", "what ws holds before a call does not matter", "keep their prior contents",
                  "nothing is launched or written"):
        assert words in header, words


def test_every_refusal_returns_before_any_hip_call():
    """On host memory, without a device: whatever passed a refusal on to a launch would answer TGSR_ELAUNCH or follow a host pointer
    on the device.  The code each gives, and an untouched arena, say none does."""
    run_refusals("cpu")
    names = [n for n, _kw, _c in aug_refusals()]
    assert len(set(names)) == len(names) == 38 and len(coeff_refusals()) == 12
    for want in ["packed-null", "table_host-null", "table_dev-null", "ws-null", "out-null", "nbytes-0", "nbytes-2^31", "B-0", "B-65536", "S-0", "S-4097",
                 "nbytes-one-short", "row-ratio-above-16", "table_host-off-4", "table_dev-off-4", "ws-off-4"]:
        assert want in names, want
    cols = {kw["row"][1] for _n, kw, _c in aug_refusals() if "row" in kw}
    assert cols == set(range(12)), "one bad value for each of the twelve descriptor fields"


def test_the_refusal_calls_are_valid_but_for_the_one_thing():
    packed, table = ref_inputs()
    assert all(desc_ok(d, REF_S, packed.size) for d in table)
    assert not desc_ok(table[2], REF_S, packed.size - 1) and desc_ok(table[1], REF_S, packed.size - 1), "one short cuts the last image only"
    for name, kw, _code in aug_refusals():
        if "row" in kw:
            t = ref_table(kw)
            bad = [i for i, d in enumerate(t) if not desc_ok(d, REF_S, packed.size)]
            assert bad == [1], name
    for name, kw, code in coeff_refusals():
        i, o, k = kw.get("i", 7), kw.get("o", 3), kw.get("k", 7)
        if code == "EUNSUPPORTED" or "bounds" in kw or "taps" in kw:
            assert (i, o, k) == (7, 3, ksize(7, 3))
    assert ksize(7, 3) == 7 and ksize(33, 2) == 35 and ksize(1, 1) == 3 and ksize(16, 1) == 33 and ksize(65536, 4096) == 33


def test_the_cases_are_the_ones_their_rows_describe():
    R = {row_id(r): r[3] for r in rows(AUG_TABLE)}
    for c in R.values():
        packed, table = aug_inputs(c)
        assert all(desc_ok(d, c["S"], packed.size) for d in table), c["name"]
        assert int(table[-1, 0]) + 3 * int(table[-1, 1]) * int(table[-1, 2]) == packed.size, "the last image ends exactly at nbytes"
        dev = dev_table(c, table)
        for i, d in enumerate(dev):                                  # a descriptor the device sees and skips reads nothing outside packed if not skipped
            if not desc_ok(d, c["S"], packed.size):
                good = d.copy()
                good[11] = 0
                assert c["bad"] and i == c["bad"][0] and desc_ok(good, c["S"], packed.size), "only the flip field is wrong"
    assert {c["leads"][0] for c in R.values()} == {0, 1, 2, 3} and {c["leads"][1] for c in R.values()} == {0, 1, 2, 3}
    d = aug_inputs(R["identity"])[1][0]
    assert d[7] == d[6] - d[4] and d[8] == d[5] - d[3] and (coeffs(7, 7)[1][:, :2] == (1 << 22, 0)).all()
    t = aug_inputs(R["remainders"])[1]
    assert R["remainders"]["S"] == 64 + 6 == 8 * 8 + 6 and sorted(t[:, 11].tolist()) == [0, 1]
    assert all(d[3] > 0 and d[4] > 0 and d[5] < d[2] and d[6] < d[1] for d in t), "strictly inside"
    up = lambda d: (d[8] > d[5] - d[3], d[7] > d[6] - d[4])          # noqa: E731
    assert {up(d) for d in t} == {(True, False), (False, True)}
    d = aug_inputs(R["down16"])[1][0]
    assert (d[5] - d[3], d[6] - d[4], d[7], d[8]) == (144, 144, 9, 9) and int(coeffs(144, 9)[0][:, 1].max()) >= 32
    t = aug_inputs(R["up17"])[1]
    assert [(int(d[9]), int(d[10])) for d in t] == [(4, 4), (0, 0)] and (t[:, 7:9] == 68).all() and R["up17"]["S"] == 64
    d = aug_inputs(R["tall"])[1][0]
    assert tuple(d[1:3]) == (4096, 1) and d[7] == 65536 and d[9] + R["tall"]["S"] == 65536 and aug_inputs(R["tall"])[0].size == 12288
    t = aug_inputs(R["ragged"])[1]
    assert t[1, 0] % 2 == 1 and t[2, 0] % 2 == 1 and sorted(t[:, 11].tolist()) == [0, 1, 1]
    assert (expected("ragged")[::-1] == expected("ragged-reversed")).all() and R["ragged-reversed"]["order"] == (2, 1, 0)
    assert (aug_inputs(R["ragged-reversed"])[1][:, 0] != t[::-1, 0]).any(), "other offsets, the same images"
    assert R["skipped"]["bad"] == (1, 11, 2)


@pytest.mark.parametrize("row", rows(AUG_TABLE), ids=row_id)
def test_each_row_catches_what_it_lists(row):
    c, catch = row[3], row[4]
    ref = expected(c["name"])
    assert expected(c["name"], "right").tobytes() == ref.tobytes(), "the kernel's structure, restated, gives the plain model's bytes"
    assert set(catch) <= set(V_AUGMENT)
    for v in catch:
        assert expected(c["name"], v).tobytes() != ref.tobytes(), "%s cannot tell %s from the right kernel" % (c["name"], v)


def test_every_variant_is_caught():
    caught = set().union(*(set(r[4]) for r in rows(AUG_TABLE)))
    assert caught == set(V_AUGMENT), sorted(caught ^ set(V_AUGMENT))


@pytest.mark.parametrize("row", rows(COEFF_TABLE), ids=row_id)
def test_coefficient_rows(row):
    c = row[3]
    b, k = coeffs(c["i"], c["o"])
    assert k.shape == (c["o"], ksize(c["i"], c["o"])) and b.shape == (c["o"], 2) and MAX_RATIO * c["o"] >= c["i"]
    assert all((k[i, n:] == 0).all() for i, (_f, n) in enumerate(b.tolist())), "zero behind the count"
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= c["i"]).all()


def test_the_lds_bound_of_augment_u8_kernel():
    """augment_u8_kernel clips nrows at kAugRows silently and takes rbase from the tile's first row: first[] must never decrease, no
    count may exceed kAugMaxTaps, and the source rows under any kAugTH consecutive output rows must fit kAugRows - over every
    in <= 4096 with out at and just above ceil(in / 16), and at the ratios 15 and 15.5."""
    worst_span, worst_count = 0, 0
    for i in range(1, MAX_SIDE + 1):
        lo = -(-i // MAX_RATIO)
        for o in sorted({lo, lo + 1, max(lo, -(-i // 15)), max(lo, int(np.ceil(i / 15.5)))}):
            b = _bounds(i, o)
            first, count = b[:, 0], b[:, 1]
            assert (np.diff(first) >= 0).all(), (i, o)
            worst_count = max(worst_count, int(count.max()))
            end = first + count
            for t in range(1, TH + 1):                                # every window of up to kAugTH rows, wherever it starts
                if t <= o:
                    worst_span = max(worst_span, int((end[t - 1:] - first[:o - t + 1]).max()))
    print("AUGMENT_ABI lds bound: largest span %d, largest count %d" % (worst_span, worst_count))
    assert worst_count <= MAX_TAPS and worst_span <= ROWS


def _bounds(i, o):
    """IO.resize_coeffs' bounds alone, vectorised (checked against it below)."""
    scale = i / o
    support = max(scale, 1.0)
    center = (np.arange(o) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), i) - xmin
    return np.stack([xmin, xmax], 1)


def test_the_vectorised_bounds_are_the_oracles():
    for i, o in ((160, 10), (4096, 256), (7, 3), (3, 7), (1000, 63), (4095, 265), (31, 2)):
        assert np.array_equal(_bounds(i, o), coeffs(i, o)[0]), (i, o)


@pytest.mark.parametrize("row", rows(AUG_TABLE), ids=row_id)
def test_rows_against_pillow(row):
    Image = pytest.importorskip("PIL.Image")
    c = row[3]
    packed, table = aug_inputs(c)
    for b, d in enumerate(table.tolist()):
        off, H, W, x1, y1, x2, y2, oh, ow, top, left, flip = d
        im = Image.fromarray(packed[off:off + 3 * H * W].reshape(H, W, 3))
        im = im.crop((x1, y1, x2, y2)).resize((ow, oh), Image.BILINEAR).crop((left, top, left + c["S"], top + c["S"]))
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(np.asarray(im).transpose(2, 0, 1), expected(c["name"])[b]), (c["name"], b)
