"""CPU: what tests/test_hip_attnviz_abi.py rests on - its table, its numpy model and its refusals - checked without a GPU.

The GPU file calls tgsr_attn_panels (tgsr_amd/csrc/tgsr_attnviz.hip) through ctypes with every device operand inside one guarded arena
(tests/arena.py) and compares panel, maps, conf and order BIT-EXACT with `panels_model` below.  tests/test_hip_attnviz.py compares the
map bytes with a scipy model to within one, which is right for the shipped operators (their entries are irrational) and lets a kernel
that is one off on a few pixels pass.  Here the comparison is exact because the inputs are chosen so that every fp64 product and sum
is exact in any order:

  * att values are multiples of 2^-8 in (0, 1), some of them exactly 2 / n and 4 / n where those are such multiples;
  * Mh and Mw (`operator`) are written by rule, not by expand_operator: three bands of multiples of 1/16 in [-2/16, 6/16], neither
    the identity nor symmetric.

A tile value is then an integer over 2^16 below 2^37: tile, conf, min and max are exact, and the byte trunc(((t - min) / (max - min)) *
255) is three correctly rounded fp64 operations, which numpy repeats.  test_the_tiles_are_exact proves the claim for every row: the
tile computed in float64 equals the tile computed in integers scaled by 2^16 (2^8 for att, 2^4 for each operator).

TABLE holds one row per case and one refusal row (case None); `catch` names the wrong kernels - V_PANELS, each a change to the model -
whose outputs differ from the right kernel's on that row's input.  Three things the issue's rows cannot do, and what is done instead:
conf is identically 0 for n <= 4 (no x < 1 exceeds 4 / n), so the rect rows with n = 4 order by the tie rule alone - an involution;
the conf order that is not its own inverse is asked of rect-n6-conf.  The LDS-limit row has T = 1, so n = 1 and its map is black: it
checks the extents (a 2 MB tile in ws, 512-byte map rows) and no arithmetic.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from arena import Arena, PATTERN

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgsr_amd", "csrc")
PANELS, WS_ELEMS = "tgsr_attn_panels", "tgsr_attn_panels_ws_elems"
KAR, KPR, KAT, MAX_A, MAX_V = 16, 2, 64, 128, 512
NULL = object()
FILL = 0xA5
V_PANELS = ("thresh_T", "conf_thresh", "ge", "M_swapped", "minmax_block0", "cd_f32", "ties_lower", "inverse_perm", "one_sep",
            "slots_not_black", "map_round", "no_128", "img_trunc", "behind_live", "head_unclipped")


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream(dev):
    if torch.device(dev).type != "cuda":
        return None
    from tgsr_amd import ops
    return ops._stream()


def _t(x):
    return torch.from_numpy(np.array(x, copy=True))


def ws_elems(B, T, h, w, u):
    Vh, Vw = u * h, u * w
    return B * T * (Vh * Vw + 2 * ((Vh + KAR - 1) // KAR))


# ----------------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------------
def _c(name, B, T, h, w, u, K, by_conf, lens, why, catch, img="u8", alpha=180, with_maps=True, dev_lens=None, nan_behind=False, offs=(0, 0),
       tie=None, seed=0):
    """lens: the caption lengths the model uses; dev_lens: what the device sees where that differs (the clamp); offs: bytes of panel
    and maps off a 16-byte boundary; tie = (b, j0, j1): two words of image b with the same map."""
    return dict(name=name, B=B, T=T, h=h, w=w, u=u, K=K, by_conf=by_conf, lens=tuple(lens), img=img, alpha=alpha, with_maps=with_maps,
                dev_lens=tuple(dev_lens or lens), nan_behind=nan_behind, offs=offs, tie=tie, seed=seed), why, tuple(catch)


SEED6 = 1                 # of rect-n6-conf: the first seed whose conf order is not its own inverse
_PASTE = ("one_sep", "map_round", "no_128")
_LIVE = ("conf_thresh", "cd_f32") + _PASTE
CASES = (
    _c("minimal-T1", 1, 1, 2, 2, 1, 1, 0, (1,), "h = w = 2, u = 1, T = n = K = 1: the threshold is 2, the map is black, max == min", ("no_128",)),
    _c("minimal-T3", 1, 3, 2, 2, 1, 3, 1, (3,), "the same map size with T = n = K = 3 and a live map", ("conf_thresh", "M_swapped", "ties_lower") + _PASTE),
    _c("rect-n4-slot", 1, 6, 5, 12, 3, 3, 0, (4,), "h = 5, w = 12, u = 3, T = 6, n = 4, K = 3, slot = word; thresh = 1/2 and an x of exactly 1/2",
       ("thresh_T", "ge", "cd_f32", "behind_live") + _PASTE),
    _c("rect-n4-conf", 1, 6, 5, 12, 3, 3, 1, (4,), "the same by conf: conf is 0 for every word (4 / n = 1), the tie rule alone orders: 3 2 1 0",
       ("thresh_T", "ge", "cd_f32", "ties_lower", "behind_live") + _PASTE),
    _c("rect-n6-conf", 1, 6, 5, 12, 3, 3, 1, (6,), "the same with n = 6: a conf order that is not its own inverse", ("inverse_perm",) + _LIVE, seed=SEED6),
    _c("ragged-tiles", 2, 5, 17, 17, 2, 4, 1, (5, 3), "h = w = 17, u = 2: hp = 20, wp = 32, Vh = Vw = 34: three row blocks, the last of two rows, three "
       "column tiles, the last of two columns; a float32 image", ("thresh_T", "M_swapped", "minmax_block0", "slots_not_black", "img_trunc", "behind_live") + _LIVE,
       img="f32"),
    _c("thin-128x2", 1, 4, 128, 2, 1, 4, 0, (4,), "(h, w) = (128, 2), u = 1: eight row blocks, one column tile of two", ("ge", "minmax_block0", "cd_f32") + _PASTE),
    _c("thin-2x128", 1, 4, 2, 128, 1, 4, 0, (4,), "(h, w) = (2, 128), u = 1: one row block of two rows, eight column tiles", ("ge", "cd_f32") + _PASTE),
    _c("lds-limit", 1, 1, 128, 128, 4, 1, 0, (1,), "h = w = 128, u = 4, T = 1: the 512 limit, 107 584 bytes of LDS; n = 1: a black map - the extents, no "
       "arithmetic", ("no_128",)),
    _c("most-words-K64", 3, 64, 4, 4, 1, 64, 1, (64, 1, 33), "T = 64, B = 3, lens 64, 1, 33; words 10 and 40 of image 0 have the same map: the tie goes "
       "to the higher index; K = 64", ("thresh_T", "ge", "M_swapped", "ties_lower", "inverse_perm", "slots_not_black", "behind_live") + _LIVE, tie=(0, 10, 40)),
    _c("most-words-K1", 3, 64, 4, 4, 1, 1, 1, (64, 1, 33), "the same with K = 1: one slot", ("ties_lower", "inverse_perm", "conf_thresh", "cd_f32", "map_round", "no_128"), tie=(0, 10, 40)),
    _c("behind-the-caption", 2, 5, 4, 6, 2, 4, 1, (2, 4), "the maps of words >= n hold the arena's NaN: conf 0, order -1 and black maps there, nothing non-finite",
       ("thresh_T", "slots_not_black") + _LIVE, nan_behind=True),
    _c("clamp", 2, 6, 4, 4, 2, 6, 1, (1, 6), "device cap_lens of 0 acts as 1, T + 5 = 11 as T = 6 (T <= 59: an unclamped kernel stays inside its LDS "
       "arrays and the arena)", ("M_swapped", "slots_not_black") + _LIVE, dev_lens=(0, 11)),
) + tuple(
    _c("align-3x2-%d" % o, 2, 3, 3, 2, 1, 1, 0, (3, 2), "panel %d and maps %d bytes off 16; h = 3, w = 2, u = 1, K = 1: row groups of 24 and 12 panel bytes, "
       "map rows of 2 bytes" % (o, (o + 5) % 16), ("map_round", "no_128") + (("head_unclipped",) if o in HEAD_O else ()), offs=(o, (o + 5) % 16))
    for HEAD_O in (tuple(o for o in range(16) if o not in (8, 9)),) for o in range(16)
) + tuple(
    _c("align-4x5-%d" % o, 1, 3, 4, 5, 2, 2, 1, (3,), "panel %d and maps %d bytes off 16; Vh = 8, Vw = 10, K = 2: row groups of 144 bytes, of 20 map bytes"
       % (o, (o + 11) % 16), _LIVE, offs=(o, (o + 11) % 16)) for o in range(16)
) + (
    _c("maps-null", 2, 4, 4, 5, 2, 3, 1, (4, 3), "maps_or_null == NULL: the region of maps stays untouched", _LIVE, with_maps=False),
    _c("alpha-0", 2, 4, 4, 5, 2, 3, 1, (4, 3), "alpha = 0: the image alone", ("one_sep", "no_128"), alpha=0),
    _c("alpha-255", 2, 4, 4, 5, 2, 3, 1, (4, 3), "alpha = 255: the map alone", ("cd_f32", "one_sep", "map_round", "no_128"), alpha=255),
    _c("img-f32-ties", 2, 4, 4, 5, 2, 3, 1, (4, 3), "a float32 image with values on .5 ties and outside [-1, 1]", ("img_trunc",) + _LIVE, img="f32"),
    _c("second-trip", 2, 4, 4, 5, 2, 3, 0, (4, 3), "run twice, ws refilled with a finite value in between: the same bits", _PASTE),
)
R_PANELS = ("att, cap_lens, img, Mh, Mw, ws, panel, conf or order NULL; B, T, K < 1; K > T; u < 1; alpha outside [0, 255]: TGSR_EINVAL; h or w outside "
            "[2, 128], u h or u w > 512, T > 64 (ws_elems 0); att, cap_lens, order or a float32 img off 4 bytes; Mh, Mw, ws or conf off 8 bytes: "
            "TGSR_EUNSUPPORTED: refused, nothing launched or written")
TABLE = [(PANELS, "attn_expand_kernel + attn_panel_kernel", why, c, catch) for c, why, catch in CASES] + [(PANELS, "no instance", R_PANELS, None, ())]


def rows():
    return [r for r in TABLE if r[3] is not None]


def row_id(r):
    return r[3]["name"]


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs
# ----------------------------------------------------------------------------------------------------------------------------
def operator(V, a, u, salt):
    """float64 [V][a]: the bands |v // u - k| < 2 of ((5 v + 3 k + salt) mod 9 - 2) / 16."""
    v, k = np.arange(V)[:, None], np.arange(a)[None, :]
    M = np.where(np.abs(v // u - k) < 2, ((5 * v + 3 * k + salt) % 9 - 2) / 16.0, 0.0)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _ties():
    """float32 v with ((v + 1) / 2) * 255 == k + 0.5 exactly, in float32."""
    f = np.float32
    k = np.arange(255, dtype=np.float64)
    v = ((2 * k + 1) / 255.0 - 1.0).astype(f)
    y = ((v + f(1)) / f(2)) * f(255)
    return v[y == (k + 0.5).astype(f)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(att float32 [B][T][h][w], img [B][3][Vh][Vw] uint8 or float32, Mh, Mw)."""
    c = next(r[3] for r in rows() if r[3]["name"] == name)
    B, T, h, w, u = c["B"], c["T"], c["h"], c["w"], c["u"]
    rng = np.random.default_rng([41, B, T, h, w, u, c["seed"]])
    att = (rng.integers(1, 256, (B, T, h, w)) / 256.0).astype(np.float32)
    for b, n in enumerate(c["lens"]):
        flat = att[b].reshape(T, -1)
        for j in range(n):                                           # an x of exactly thresh and one of exactly 2 thresh, where they exist
            if 512 % n == 0 and 2 < n:
                flat[j, (7 * j + 1) % (h * w)] = 2.0 / n
            if 1024 % n == 0 and 4 < n:
                flat[j, (5 * j + 3) % (h * w)] = 4.0 / n
    if c["tie"]:
        b, j0, j1 = c["tie"]
        att[b, j1] = att[b, j0]
    if c["nan_behind"]:
        for b, n in enumerate(c["lens"]):
            att[b, n:].view(np.int32)[...] = PATTERN
    Vh, Vw = u * h, u * w
    if c["img"] == "u8":
        img = rng.integers(0, 256, (B, 3, Vh, Vw), dtype=np.uint8)
    else:
        img = (rng.standard_normal((B, 3, Vh, Vw)) * 0.6).astype(np.float32)
        flat = img.reshape(-1)
        idx = rng.choice(flat.size, size=max(1, flat.size // 5), replace=False)
        flat[idx] = rng.choice(_ties(), size=idx.size)
        idx = rng.choice(flat.size, size=max(3, flat.size // 40), replace=False)
        flat[idx] = rng.choice(np.array([-3.0, 2.5, -1.0, 1.0, 1.0000001, -1.0000001], np.float32), size=idx.size)
    for x in (att, img):
        x.setflags(write=False)
    return att, img, operator(Vh, h, u, 1), operator(Vw, w, u, 4)


# ----------------------------------------------------------------------------------------------------------------------------
# The model
# ----------------------------------------------------------------------------------------------------------------------------
def img_bytes(img, variant=""):
    """utils.py:341-343 in float32: add, divide, multiply, round half to even, clamp.  img_trunc: truncated."""
    if img.dtype == np.uint8:
        return img
    f = np.float32
    v = ((img + f(1)) / f(2)) * f(255)
    assert v.dtype == np.float32
    return np.clip(v if variant == "img_trunc" else np.rint(v), 0, 255).astype(np.uint8)


def tile_of(x, n, Mh, Mw, variant=""):
    """(tile float64 [Vh][Vw], conf) of one word's map x float32 [h][w] under caption length n."""
    x64 = x.astype(np.float64)
    thresh = 2.0 / float(n)
    over = (lambda a, t: a >= t) if variant == "ge" else (lambda a, t: a > t)
    conf = float(x64[over(x64, thresh if variant == "conf_thresh" else 2.0 * thresh)].sum())
    X = np.where(over(x64, thresh), x64, 0.0)
    if variant == "M_swapped":
        Mh, Mw = Mw, Mh
    return Mh @ X @ Mw.T, conf


def _cd_f32(tile):
    """The rows of every block of 16 as a kernel would store them that took the f32 MFMA's C/D map, row = 4 (lane >> 4) + reg, for the
    f64 one's (lane >> 4) + 4 reg: stored row lq + 4 r holds true row 4 lq + r (rows at and behind Vh are zero)."""
    Vh = tile.shape[0]
    pad = np.zeros((-(-Vh // KAR) * KAR,) + tile.shape[1:])
    pad[:Vh] = tile
    out = pad.copy()
    for blk in range(0, len(pad), KAR):
        for lq in range(4):
            for r in range(4):
                out[blk + lq + 4 * r] = pad[blk + 4 * lq + r]
    return out[:Vh]


def stretch(tile, variant=""):
    mn, mx = (tile[:KAR].min(), tile[:KAR].max()) if variant == "minmax_block0" else (tile.min(), tile.max())
    rg = mx - mn
    if not rg > 0.0:
        return np.zeros(tile.shape, np.uint8)
    y = ((tile - mn) / rg) * 255.0
    y = np.rint(y) if variant == "map_round" else np.trunc(y)
    return (y.astype(np.int64) & 255).astype(np.uint8)             # (unsigned)(int) y, then the store of its low byte


def slot_order(conf, n, by_conf, variant=""):
    order = np.full(len(conf), -1, np.int32)
    words = list(range(n))
    if by_conf:
        words.sort(key=lambda j: (-conf[j], j if variant == "ties_lower" else -j))
    if variant == "inverse_perm":
        words = np.argsort(words).tolist()
    order[:n] = words
    return order


def panels_model(c, variant=""):
    """dict(panel [B][Vh][K (Vw + 2)][3], maps [B][T][Vh][Vw], conf float64 [B][T], order int32 [B][T], tails = the 16 bytes behind
    panel and maps as the call leaves them).  The wrong kernels:
    thresh_T 2 / T for 2 / n;  conf_thresh conf over x > thresh;  ge >= for >;  M_swapped Mh and Mw exchanged;  minmax_block0 min / max
    of the first row block only;  cd_f32 the f32 MFMA's C/D rows;  ties_lower ties to the lower index;  inverse_perm the slot of every
    word for the word of every slot;  one_sep one separator column;  slots_not_black slots at and behind min(K, n) blended over a zero
    map;  map_round the map byte rounded;  no_128 the paste without + 128;  img_trunc the image byte truncated;  behind_live the maps
    of words behind the caption computed like the others;  head_unclipped the head of a row group not clipped to the group."""
    att, img, Mh, Mw = inputs(c["name"])
    B, T, u, K, alpha = c["B"], c["T"], c["u"], c["K"], c["alpha"]
    Vh, Vw = u * c["h"], u * c["w"]
    ib = img_bytes(img, variant).astype(np.int64)
    panel = np.zeros((B, Vh, K * (Vw + 2), 3), np.uint8)
    maps = np.zeros((B, T, Vh, Vw), np.uint8)
    conf, order = np.zeros((B, T)), np.zeros((B, T), np.int32)
    cell = Vw + 1 if variant == "one_sep" else Vw + 2
    for b in range(B):
        n = min(max(int(c["dev_lens"][b]), 1), T)
        assert n == c["lens"][b]
        for j in range(T if variant == "behind_live" and not c["nan_behind"] else n):
            tile, cf = tile_of(att[b, j], T if variant == "thresh_T" else n, Mh, Mw, variant)
            if j < n:
                conf[b, j] = cf
            maps[b, j] = stretch(_cd_f32(tile) if variant == "cd_f32" else tile, variant)
        order[b] = slot_order(conf[b], n, c["by_conf"], variant)
        for s in range(K):
            if s < min(K, n):
                m = maps[b, order[b, s]].astype(np.int64)
            elif variant == "slots_not_black":
                m = np.zeros((Vh, Vw), np.int64)
            else:
                continue
            t = m[:, :, None] * alpha + ib[b].transpose(1, 2, 0) * (255 - alpha) + (0 if variant == "no_128" else 128)
            panel[b, :, s * cell:s * cell + Vw] = (((t >> 8) + t) >> 8).astype(np.uint8)
    tails = np.full((2, 16), FILL, np.uint8)
    if variant == "head_unclipped":                                # the last row group of the last image / plane: head bytes from r0 on
        for k, (nbytes, row) in enumerate(((panel.size, K * (Vw + 2) * 3), (maps.size, Vw))):
            group = ((Vh - 1) % KPR + 1) * row
            head = (16 - (c["offs"][k] + nbytes - group) % 16) % 16
            if head > group:
                tails[k, :head - group] = 0
    return dict(panel=panel, maps=maps, conf=conf, order=order, tails=tails)


@functools.lru_cache(maxsize=None)
def expected(name, variant=""):
    c = next(r[3] for r in rows() if r[3]["name"] == name)
    return panels_model(c, variant)


def differ(a, b):
    return any(a[k].tobytes() != b[k].tobytes() for k in ("panel", "maps", "conf", "order", "tails"))


# ----------------------------------------------------------------------------------------------------------------------------
# Refusals: a valid small call with one thing wrong
# ----------------------------------------------------------------------------------------------------------------------------
REF = dict(B=2, T=5, h=4, w=4, u=2, alpha=180, K=3, by_conf=1, f32=1)
POINTERS = ("att", "cap_lens", "img", "Mh", "Mw", "ws", "panel", "conf", "order")


def refusals():
    out = [(n + "-null", {n: NULL}, "EINVAL") for n in POINTERS]
    out += [(n, kw, "EINVAL") for n, kw in (("B-0", dict(B=0)), ("T-0", dict(T=0)), ("K-0", dict(K=0)), ("K-T+1", dict(K=6)), ("u-0", dict(u=0)),
                                            ("alpha-negative", dict(alpha=-1)), ("alpha-256", dict(alpha=256)))]
    out += [(n, kw, "EUNSUPPORTED") for n, kw in (("h-1", dict(h=1)), ("w-129", dict(w=129)), ("uh-513", dict(h=27, u=19)), ("T-65", dict(T=65)))]
    out += [(n + "-off-4", dict(off=(n, 2)), "EUNSUPPORTED") for n in ("att", "cap_lens", "order", "img")]
    out += [(n + "-off-8", dict(off=(n, 4)), "EUNSUPPORTED") for n in ("Mh", "Mw", "ws", "conf")]
    return out


def refusal_call(L, a, dev, **kw):
    B, T, h, w, u = (REF[k] for k in ("B", "T", "h", "w", "u"))
    Vh, Vw = u * h, u * w
    g = np.random.default_rng(9)
    spare = lambda x: np.concatenate([x.reshape(-1), x.reshape(-1)[:2]])      # noqa: E731  two elements to spare for an operand moved up
    regs = dict(att=a.place_input(_t(spare((g.integers(1, 256, (B, T, h, w)) / 256.0).astype(np.float32)))),
                cap_lens=a.place_input(_t(np.array([5, 3, 0, 0], np.int32))),
                img=a.place_input(_t(spare(g.standard_normal((B, 3, Vh, Vw)).astype(np.float32)))),
                Mh=a.place_input(_t(spare(np.array(operator(Vh, h, u, 1))))), Mw=a.place_input(_t(spare(np.array(operator(Vw, w, u, 4))))))
    n = L.tgsr_attn_panels_ws_elems(B, T, h, w, u)
    assert n == ws_elems(B, T, h, w, u)
    regs.update(ws=a.place_output((n + 1,), dtype=torch.float64, written=False), panel=a.place_output_u8((B, Vh, REF["K"] * (Vw + 2), 3), written=False, lead=1),
                maps=a.place_output_u8((B, T, Vh, Vw), written=False, lead=3), conf=a.place_output((B * T + 1,), dtype=torch.float64, written=False),
                order=a.place_output((B * T + 1,), dtype=torch.int32, written=False))
    v = dict(REF, **{k: x for k, x in kw.items() if k in REF})
    if any(k in kw for k in ("h", "w", "u", "T")) and v["u"] >= 1 and v["T"] >= 1:
        assert L.tgsr_attn_panels_ws_elems(v["B"], v["T"], v["h"], v["w"], v["u"]) == 0
    ptr = lambda name: None if kw.get(name) is NULL else ctypes.c_void_p(regs[name].address + (kw["off"][1] if kw.get("off", ("",))[0] == name else 0))  # noqa: E731
    return lambda: L.tgsr_attn_panels(ptr("att"), ptr("cap_lens"), ptr("img"), v["f32"], ptr("Mh"), ptr("Mw"), v["B"], v["T"], v["h"], v["w"], v["u"],
                                      v["alpha"], v["K"], v["by_conf"], ptr("ws"), ptr("panel"), ptr("maps"), ptr("conf"), ptr("order"), _stream(dev))


def run_refusals(dev):
    M, L = _lib()
    for name, kw, code in refusals():
        a = Arena(dev, guard=64)
        call = refusal_call(L, a, dev, **kw)
        a.buffer()
        assert call() == getattr(M, code), name
        v = a.violations()
        assert not v, name + ": " + "; ".join(v)


# ============================================================================================================================
# The host tests
# ============================================================================================================================
TEXT = open(os.path.join(CSRC, "tgsr_attnviz.hip")).read()


def test_the_table_against_the_source():
    for name, v in (("kAR", KAR), ("kAT", KAT), ("kPR", KPR), ("kAMaxA", MAX_A), ("kAMaxV", MAX_V)):
        assert re.search(r"constexpr int %s = %d;" % (name, v), TEXT), name
    launches = re.findall(r"hipLaunchKernelGGL\(([a-z_0-9]+)", TEXT)
    assert sorted(launches) == ["attn_expand_kernel", "attn_panel_kernel"] and all(k in TABLE[0][1] for k in launches)
    for snippet in ("if (!att || !cap_lens || !img || !Mh || !Mw || !ws || !panel || !conf || !order) return TGSR_EINVAL;",
                    "if (B < 1 || T < 1 || K < 1 || K > T || u < 1 || alpha < 0 || alpha > 255) return TGSR_EINVAL;",
                    "if (h < 2 || w < 2 || h > kAMaxA || w > kAMaxA || T > kAT) return false;",
                    "return (int64_t)u * h <= kAMaxV && (int64_t)u * w <= kAMaxV;",
                    "if ((low(att) | low(cap_lens) | low(order) | (img_f32 ? low(img) : 0)) & 3) return TGSR_EUNSUPPORTED;",
                    "if ((low(Mh) | low(Mw) | low(ws) | low(conf)) & 7) return TGSR_EUNSUPPORTED;",
                    "return (int64_t)B * T * ((int64_t)Vh * Vw + 2 * ((Vh + kAR - 1) / kAR));", "if (head > r1 - r0) head = r1 - r0;",
                    "if (head > span) head = span;", "return n < 1 ? 1 : (n > T ? T : n);"):
        assert snippet in TEXT, snippet
    assert [r[1] for r in TABLE if r[3] is None] == ["no instance"] and "refused" in TABLE[-1][2]
    names = [row_id(r) for r in rows()]
    assert len(set(names)) == len(names)
    M, L = _lib()
    assert len(M.SIGNATURES[PANELS][1]) == 20 and len(M.SIGNATURES[WS_ELEMS][1]) == 5
    for r in rows():
        c = r[3]
        assert L.tgsr_attn_panels_ws_elems(c["B"], c["T"], c["h"], c["w"], c["u"]) == ws_elems(c["B"], c["T"], c["h"], c["w"], c["u"]) > 0
    for bad in ((0, 5, 8, 8, 4), (1, 0, 8, 8, 4), (1, 5, 1, 8, 4), (1, 5, 8, 1, 4), (1, 5, 8, 129, 1), (1, 5, 129, 8, 1), (1, 5, 8, 8, 0),
                (1, 5, 27, 8, 19), (1, 5, 8, 27, 19), (1, 65, 8, 8, 4), (-1, 5, 8, 8, 4)):
        assert L.tgsr_attn_panels_ws_elems(*bad) == 0, bad
    header = open(os.path.join(CSRC, "..", "..", "include", "tgsr_hip.h")).read()
    for words in ("panel, maps and a uint8 img may start at any byte", "neither written nor read", "conf and order are written whole",
                  "nothing is launched or written"):
        assert words in header, words


def test_every_refusal_returns_before_any_hip_call():
    """On host memory, without a device: the entry returns from its argument checks, no pointer is followed."""
    run_refusals("cpu")
    names = [n for n, _kw, _c in refusals()]
    assert len(set(names)) == len(names) == 28 and [n for n in names if n.endswith("-null")] == [p + "-null" for p in POINTERS]
    for want in ("B-0", "T-0", "K-0", "K-T+1", "u-0", "alpha-negative", "alpha-256", "h-1", "w-129", "uh-513", "T-65"):
        assert want in names
    assert REF["K"] + 3 == REF["T"] + 1 and 27 * 19 == 513 and 19 * REF["w"] <= 512


def test_a_byte_image_at_any_byte_is_no_refusal():
    """What the alignment rule leaves out: a uint8 img, panel and maps take part in no alignment refusal (the GPU file runs them at
    every byte offset)."""
    assert "(img_f32 ? low(img) : 0)" in TEXT and "low(panel)" not in TEXT and "low(maps" not in TEXT


def _int_tile(x, n, Mh, Mw):
    """tile_of in integers: att scaled by 2^8, each operator by 2^4."""
    xi = np.rint(x.astype(np.float64) * 256).astype(np.int64)
    assert (xi / 256.0 == x).all() and (xi > 0).all() and (xi < 256).all()
    a, b = np.rint(Mh * 16).astype(np.int64), np.rint(Mw * 16).astype(np.int64)
    assert (a / 16.0 == Mh).all() and (b / 16.0 == Mw).all()
    X = np.where(xi * n > 512, xi, 0)                                # x > 2 / n
    t = a @ X @ b.T
    return t, int(xi[xi * n > 1024].sum())


def test_the_tiles_are_exact():
    for r in rows():
        c = r[3]
        att, _img, Mh, Mw = inputs(c["name"])
        for b, n in enumerate(c["lens"]):
            for j in range(n):
                tile, conf = tile_of(att[b, j], n, Mh, Mw)
                ti, ci = _int_tile(att[b, j], n, Mh, Mw)
                assert int(np.abs(ti).max()) < 1 << 53 and (tile * 65536.0 == ti).all() and conf * 256.0 == ci, (c["name"], b, j)
                X = np.where(att[b, j].astype(np.float64) > 2.0 / n, att[b, j], 0).astype(np.float64)
                assert (Mh @ (X @ Mw.T) == tile).all(), "the other association gives the same bits"


def test_the_operators_are_neither_the_identity_nor_symmetric():
    for V, a, u in ((2, 2, 1), (4, 4, 1), (34, 17, 2), (512, 128, 4), (128, 128, 1), (15, 5, 3)):
        M = operator(V, a, u, 1)
        assert M.shape == (V, a) and (M * 16 == np.rint(M * 16)).all() and np.abs(M).max() <= 6 / 16
        if V == a:
            assert (M != np.eye(a)).any() and (M != M.T).any() and (M != operator(V, a, u, 4)).any()
        else:
            from tgsr_amd.attnviz import expand_operator
            assert (M != expand_operator(a, u)).any()


def test_the_cases_are_the_ones_their_rows_describe():
    R = {row_id(r): r[3] for r in rows()}
    for c in R.values():
        assert 1 <= c["K"] <= c["T"] <= KAT and len(c["lens"]) == c["B"] and all(1 <= n <= c["T"] for n in c["lens"])
        assert all(min(max(d, 1), c["T"]) == n for d, n in zip(c["dev_lens"], c["lens"]))
        att = inputs(c["name"])[0]
        live = np.concatenate([att[b, :n].reshape(-1) for b, n in enumerate(c["lens"])])
        assert (live > 0).all() and (live < 1).all() and (live * 256 == np.rint(live * 256)).all()
        e = expected(c["name"])
        assert np.isfinite(e["conf"]).all()
        for b, n in enumerate(c["lens"]):
            assert (e["conf"][b, n:] == 0).all() and (e["order"][b, n:] == -1).all() and (e["maps"][b, n:] == 0).all()
            assert sorted(e["order"][b, :n].tolist()) == list(range(n))
    e = expected("minimal-T1")
    assert (e["maps"] == 0).all() and (e["panel"][:, :, :2] != 0).any() and (expected("minimal-T3")["maps"].max() == 255)
    o = expected("rect-n4-conf")["order"][0].tolist()
    assert o == [3, 2, 1, 0, -1, -1] and (expected("rect-n4-conf")["conf"] == 0).all()
    o = expected("rect-n6-conf")["order"][0]
    assert (np.argsort(o) != o).any(), "word of slot and slot of word differ"
    att = inputs("rect-n4-slot")[0]
    assert (att[0, :4] == np.float32(0.5)).any()
    c = R["ragged-tiles"]
    assert (c["h"] + 3) // 4 * 4 == 20 and (c["w"] + 15) // 16 * 16 == 32 and c["u"] * c["h"] == 34 == 2 * KAR + 2
    assert (R["thin-128x2"]["h"], R["thin-128x2"]["w"], R["thin-2x128"]["h"], R["thin-2x128"]["w"]) == (128, 2, 2, 128)
    c = R["lds-limit"]
    assert c["u"] * c["h"] == MAX_V == c["u"] * c["w"] and c["h"] == MAX_A and c["T"] == 1
    for name, K in (("most-words-K64", 64), ("most-words-K1", 1)):
        c, e = R[name], expected(name)
        assert c["T"] == KAT and c["lens"] == (64, 1, 33) and c["K"] == K and e["conf"][0, 10] == e["conf"][0, 40] > 0
        o = e["order"][0].tolist()
        assert o.index(40) + 1 == o.index(10), "the tie goes to the higher index"
    c = R["behind-the-caption"]
    att = inputs(c["name"])[0]
    assert all(np.isnan(att[b, n:]).all() and (att[b, n:].view(np.int32) == PATTERN).all() for b, n in enumerate(c["lens"]))
    c = R["clamp"]
    assert c["dev_lens"] == (0, c["T"] + 5) and c["lens"] == (1, c["T"]) and c["T"] <= 59
    assert {R["align-3x2-%d" % o]["offs"][0] for o in range(16)} == set(range(16)) == {R["align-3x2-%d" % o]["offs"][1] for o in range(16)}
    assert {R["align-4x5-%d" % o]["offs"][1] for o in range(16)} == set(range(16))
    c = R["align-3x2-5"]
    Wb = c["K"] * (c["w"] + 2) * 3
    assert Wb == 12 and (16 - (5 + (c["B"] * 3 - 1) * Wb) % 16) % 16 == 15, "a last row group of 12 bytes under a 15-byte head"
    assert not R["maps-null"]["with_maps"] and R["alpha-0"]["alpha"] == 0 and R["alpha-255"]["alpha"] == 255
    img = inputs("img-f32-ties")[1]
    assert img.dtype == np.float32 and np.isin(img, _ties()).sum() > img.size // 8 and (np.abs(img) > 1).any() and len(_ties()) >= 8
    assert (expected("alpha-0")["panel"][0, :, :10] == img_bytes(inputs("alpha-0")[1])[0].transpose(1, 2, 0)).all()


@pytest.mark.parametrize("row", rows(), ids=row_id)
def test_each_row_catches_what_it_lists(row):
    c, catch = row[3], row[4]
    ref = expected(c["name"])
    assert set(catch) <= set(V_PANELS)
    for v in catch:
        assert differ(expected(c["name"], v), ref), "%s cannot tell %s from the right kernel" % (c["name"], v)


def test_every_variant_is_caught():
    caught = set().union(*(set(r[4]) for r in rows()))
    assert caught == set(V_PANELS), sorted(caught ^ set(V_PANELS))


def test_the_model_against_the_suites_other_model():
    """panels_model against tests/attnviz_model.py (what test_hip_attnviz.py compares with) given the same operator form: the map
    bytes, conf, the order rule and - where Pillow is importable - Pillow's own paste."""
    import attnviz_model as AM
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    for name in ("minimal-T3", "rect-n4-conf", "rect-n6-conf", "ragged-tiles", "most-words-K64", "clamp", "img-f32-ties", "alpha-0", "alpha-255"):
        c = next(r[3] for r in rows() if r[3]["name"] == name)
        att, img, Mh, Mw = inputs(name)
        e = expected(name)
        ib = AM.image_bytes(np.array(img)) if img.dtype == np.float32 else img
        assert (ib == img_bytes(img)).all()
        for b, n in enumerate(c["lens"]):
            mb, conf = AM.map_bytes(att[b], n, c["u"], expand_fn=lambda X, _u: Mh @ X @ Mw.T)
            assert (mb == e["maps"][b]).all() and (conf == e["conf"][b]).all()
            assert (AM.slot_order(conf, n, bool(c["by_conf"])) == e["order"][b]).all()
            if have_pil:
                assert (AM.panel(mb, ib[b], e["order"][b], n, c["K"], c["alpha"]) == e["panel"][b]).all(), (name, b)
