"""CPU: what tests/test_hip_igemm_abi.py rests on, checked without a GPU.

  * the arena's strided in-out operand (`place_inout(bstride=...)`, the destination of an accumulating call) and its skewed
    workspace on a CPU buffer: offsets, gaps, and that check() trips on a written gap word of such a region;
  * both instance tables against the library's own planners (host functions): every row's case reaches the instance the row names
    under the switches the row names, every workspace, statistics-slot and pack size the GPU test allocates is the planner's, and
    the "one slab", "K split, last slab short", "last 2048-pixel slot short" cases are what they claim;
  * the tables name every instantiated kernel of csrc/tgsr_down.hip and of the convolution half of csrc/tgsr_igemm.hip;
  * tolerance discrimination, once per convolution case: the fp64 reference, built again with one border pixel (last row, last
    column of the last sample - the pixel a ragged-tile bug would drop) of the gathered operand zeroed, must differ from the first by
    MORE than the case's tolerance in at least one element.  A case that fails this is to be shrunk or re-seeded, never its
    tolerance widened.
"""
import pytest
import torch

import test_hip_igemm_abi as T
from arena import GUARD, PATTERN, Arena


# ---- the arena's new parameters ----
def test_arena_strided_inout_and_skewed_workspace():
    a = Arena("cpu")
    base = torch.arange(24, dtype=torch.float32).view(2, 3, 4) + 1
    io = a.place_inout(base, bstride=20)
    ws = a.place_ws(6, skew=1)
    sk = a.place_inout(torch.ones(3), skew=3)
    assert io.span == 20 + 12 and io.slices() == [(io.offset, io.offset + 12), (io.offset + 20, io.offset + 32)]
    assert io.address % 16 == 0 and ws.address % 16 == 4 and sk.address % 16 == 12 and ws.span == 6
    assert ws.offset - (io.offset + io.span) >= GUARD
    buf = a.buffer()
    assert torch.equal(io.read(), base) and bool((buf[io.offset + 12:io.offset + 20] == PATTERN).all())
    a.check()                                                        # an in-out operand is born written: its initial values
    buf.view(torch.float32)[io.offset:io.offset + 12] += 0.5         # the call updates both samples ...
    buf.view(torch.float32)[io.offset + 20:io.offset + 32] += 0.5
    buf.view(torch.float32)[ws.offset:ws.offset + 6] = 0.25
    a.check()
    assert torch.equal(io.read(), base + 0.5)
    for word, what in ((io.offset + 12, "the gap"), (io.offset + 19, "the gap"), (ws.offset + 6, "past the end of ws"),
                       (ws.offset - 1, "before ws"), (io.offset - 1, "before inout")):
        keep = int(buf[word])
        buf[word] = 0
        v = a.violations()
        assert len(v) == 1 and "were written" in v[0] and what in v[0], (word, what, v)
        with pytest.raises(AssertionError):
            a.check()
        buf[word] = keep
        a.check()
    buf.view(torch.float32)[io.offset + 25] = float("nan")
    assert any("non-finite" in v for v in a.violations())
    buf[io.offset + 25] = PATTERN
    assert any("1 of 24 words never written" in v for v in a.violations())
    a.rearm(ws_fill=0.75)
    assert torch.equal(io.read(), base) and ws.read().tolist() == [0.75] * 6
    with pytest.raises(AssertionError):
        Arena("cpu").place_inout(base, bstride=11)                   # samples would overlap


# ---- the instance tables against the library's planners ----
def _L():
    from tgsr_amd import _lib
    return _lib.lib()


@pytest.fixture(autouse=True)
def switches_stay_put():
    L = _L()
    before = (L.tgsr_dconv_set_split(1), L.tgsr_gconv_set_form(1))
    L.tgsr_dconv_set_split(before[0])
    L.tgsr_gconv_set_form(before[1])
    yield
    assert (L.tgsr_dconv_set_split(before[0]), L.tgsr_gconv_set_form(before[1])) == before, "a test left a switch changed"


@pytest.mark.parametrize("row", T._drows(), ids=T.drow_id)
def test_discriminator_rows_reach_their_instance(row):
    entry, instance, cond, c = row
    p = T.d_plan(_L(), c)                                            # (asserts that the workspace is [head | asked slabs])
    assert p["instance"] == instance
    assert entry == T.D_FN[(c["kind"], c["op"])]
    T.check_plan_claims(cond, p)
    assert ("switch 0" in cond) == (c["sw"] == 0) or "skew" in cond or p["image"] or "off" in cond
    if not p["image"]:
        assert p["M"] % p["MB"] != 0 and p["N"] % p["NB"] != 0, "the last M tile and the last N tile are ragged"
    for name in c["skew"]:
        assert name in ("x", "w", "dy", "ws", "out")
    x, w, dy = T.d_inputs(T._dkey(c))
    assert x.numel() * w.shape[0] * w.shape[2] * w.shape[3] <= 2e9, "the fp64 reference stays cheap"


@pytest.mark.parametrize("row", T._grows(), ids=T.grow_id)
def test_trunk_rows_reach_their_instance(row):
    entry, instance, cond, c = row
    L = _L()
    p = T.g_plan(L, c)                                               # (asserts the workspace and the slots against the planners)
    assert p["instance"] == instance
    assert (entry == T.GSTATS) == (c["mode"] == "s") == (c["bn"] is not None)
    T.check_plan_claims(cond, p)
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = c["geom"]
    assert p["M"] * p["K"] == Cout * Cin * kh * kw, "the pack holds exactly the filter's elements"
    if c["mode"] == "s":
        assert p["nslots"] == L.tgsr_gconv_stats_nslots(B, Cout, p["OH"], p["OW"], Cin * kh * kw) >= 1
        assert (p["nslots"] - 1) * p["slot_px"] < p["N"] <= p["nslots"] * p["slot_px"]
    if p["form"] != "image" and not c["raw"]:
        assert p["M"] % (64 if p["wide"] else 128) != 0 and p["N"] % p["NB"] != 0, "the last M tile and the last N tile are ragged"
        assert B >= 2 and c["spad"] % 2 == 1 and c["opad"] % 2 == 1 and c["sextra"] and c["oextra"]
    if c["mode"] == "d":
        assert not c["bias"] and not c["relu"]


def test_the_tables_account_for_every_instance():
    d = " ".join(r[1] for r in T.DTABLE if r[3] is not None)
    for mode, wides in (("kFwd4", ("true", "false")), ("kDgrad4", ("true", "false")), ("kFwd3", ("false",)), ("kDgrad3", ("false",)),
                        ("kWgrad4", ("false",)), ("kWgrad3", ("false",))):
        for wide in wides:
            for name in [T._F32 % (mode, wide)] + [T._S6 % (mode, wide, apre) for apre in (("true", "false") if "4" in mode and "W" not in mode else ("false",))]:
                conds = [r[2] for r in T.DTABLE if r[1] == name and r[3] is not None]
                assert any("one slab" in k for k in conds) and any("last slab short" in k for k in conds), name
    assert len({r[1] for r in T.DTABLE if r[3] is not None and "igemm_kernel" in r[1]}) == 8
    assert len({r[1] for r in T.DTABLE if r[3] is not None and "igemm6_kernel" in r[1]}) == 12
    for cin in (1, 2, 3, 4):
        assert "dconv_dgrad4_image_kernel<%d>" % cin in d
    assert any(r[3] is None and "not instantiated" in r[2] for r in T.DTABLE)
    # act = 1 in the GEMM epilogue (one slab) and in slab_sum_kernel (K split), on both arithmetic forms
    for needle in ("act in the GEMM epilogue", "act in slab_sum_kernel"):
        assert sum(needle in r[2] and r[3]["act"] == 1 for r in T.DTABLE if r[3] is not None) >= 2
    # the fallbacks under switch 1: a partial chunk, pixels % 16 != 0, 4 Cout % 16 != 0, and every operand ig_plan's `align` names
    skewed = {(r[3]["kind"], r[3]["op"], n) for r in T.DTABLE if r[3] is not None and "igemm_kernel" in r[1] for n in r[3]["skew"]}
    for (kind, op), names in T.D_ALIGN.items():
        for n in names:
            assert (kind, op, n) in skewed or (3, op, n) in skewed or (4, op, n) in skewed, (kind, op, n)
    assert {(4, 0, "w"), (4, 0, "ws"), (4, 1, "w"), (4, 1, "ws"), (4, 2, "dy"), (3, 0, "w"), (3, 2, "dy")} <= skewed
    g = [r for r in T.GTABLE if r[3] is not None]
    names = {r[1].split(" + ")[0] for r in g}
    for dg, wide, stats in (("false", "false", "false"), ("false", "true", "false"), ("true", "false", "false"), ("true", "true", "false"),
                            ("false", "false", "true"), ("false", "true", "true")):
        assert T._GF % (dg, wide, stats) in names
        assert T._G6 % ("kDgradG" if dg == "true" else "kFwdG", wide, stats) in names
    for m in (1, 2, 3, 4):
        assert T._IM % m in names
    for fin in (T._FIN, T._FST):
        assert sum(fin in r[1] and "fp32" == T.g_plan(_L(), r[3])["form"] for r in g) and sum(fin in r[1] and "igemm6" in r[1] for r in g)
    taps = {(c["geom"][5], c["geom"][6], c["geom"][7]) for c in (r[3] for r in g)}
    assert {(1, 1, 1), (3, 3, 1), (3, 3, 2), (1, 7, 1), (7, 1, 1), (5, 5, 1)} <= taps
    conds = " | ".join(r[2] for r in g)
    for predicate in ("KH KW = 36 > 25", "K % 16 != 0", "data gradient at stride 2", "A one word off", "mask given with M <= 4",
                      "ops.linear", "ops.conv1x1_wgrad", "tgsr_dconv_set_split(0)"):
        assert predicate in conds, predicate
    assert {c["scale"] for c in (r[3] for r in g) if not c["raw"]} == {0, 1}
    assert {c["bn"] for c in (r[3] for r in g) if c["bn"] is not None} == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- tolerance discrimination ----
def _discriminates(full, dropped, atol, rtol):
    return bool(((full - dropped).abs() > atol + rtol * full.abs()).any())


def _unique(rows, key):
    seen = {}
    for r in rows:
        seen.setdefault(key(r[3]), r)
    return list(seen.values())


@pytest.mark.parametrize("row", _unique(T._drows(), lambda c: (T._dkey(c), c["op"], c["act"])), ids=T.drow_id)
def test_discriminator_tolerance_tells_a_dropped_border_pixel(row):
    c = row[3]
    ops = list(T.d_inputs(T._dkey(c)))
    ref, _ = T.d_refs(T._dkey(c), c["op"], c["act"])
    cut = ops[T.d_gathered(c)].clone()
    cut[-1, :, -1, -1] = 0
    ops[T.d_gathered(c)] = cut
    atol, rtol = T.d_tol(c, ref)
    assert _discriminates(ref, T.d_reference(c["kind"], c["op"], c["act"], *ops, torch.float64), atol, rtol)


@pytest.mark.parametrize("row", _unique(T._grows(), T._gkey), ids=T.grow_id)
def test_trunk_tolerance_tells_a_dropped_border_pixel(row):
    c = row[3]
    ref, _ = T.g_refs(T._gkey(c))
    assert T.rel(T.g_reference(T._gkey(c), torch.float64, cut=True), ref) > T.G_CAP[c["mode"]]
