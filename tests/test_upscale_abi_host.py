"""CPU: what tests/test_hip_upscale_abi.py rests on, checked without a GPU.

  * the table against tgsr_tiles.hip, tgsr_ensemble.hip and tgsr_metrics.hip: every hipLaunchKernelGGL has a row with a case, the
    table names nothing the files lack, every launcher condition (vec_in, vec_out, vec_src, vec_dst, the `which` / `two` grids, the
    four template pairings) stands in a row;
  * every refusal of the GPU file's test_refusals, here on host memory: each is a return in front of the first launch; the calls
    they start from keep every rule but the one;
  * the grid arithmetic restated there against the launchers' text; every case named for a second trip makes one in the loop it
    names and no other case does; the sizes just below (147 x 148, th = tw = 32, 576, C = 32) make none; the arithmetic of
    the unreachable 64-bit item loop;
  * every case is the one its row describes: the vector flags written by hand, origins modulo 4, sides modulo 32, which operand is
    off, the device row that fails the kernels' check and the host row that does not;
  * the models against something independent: gather and stitch against plain slicing loops, the ensemble model against
    tgsr_amd.tiles' index maps and torch.flip / transpose, the tiled metrics model against metrics_model and metrics_model against
    the recorded tests/golden/sr_metrics.npz values;
  * each row tells a right kernel from the wrong ones it lists, and every wrong kernel is caught by some row.
"""
import os
import re

import numpy as np
import pytest
import torch

import ensemble_model as EM
import metrics_model as MM
import test_hip_upscale_abi as A
import tiles_model as TM
from conftest import load_npz

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgsr_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


TEXT = {n: source(n) for n in ("tgsr_tiles.hip", "tgsr_ensemble.hip", "tgsr_metrics.hip")}
CASES = [r for r in A.TABLE if r[3] is not None and not r[3].get("unreachable")]


# ---- the table against the sources ----
def test_the_table_names_every_launch_of_the_sources():
    inst = set()
    for text in TEXT.values():
        inst |= {re.sub(r"\s", "", m) for m in re.findall(r"hipLaunchKernelGGL\(\(?([A-Za-z_0-9]+(?:<[^>]*>)?)", text)}
    want = set(A.K_G.values()) | set(A.K_DG.values()) | set(A.K_M.values()) | {A.K_S, A.K_DM, A.K_FIN, A.K_Y}
    assert inst == want and len(want) == 12
    with_case = " ".join(r[1] for r in CASES)
    for k in inst:
        assert k in with_case, k + " has no row with a case"
    named = set(re.findall(r"[a-z_0-9]+_kernel(?:<[^>]*>)?", " ".join(r[1] for r in A.TABLE)))
    assert named == inst, sorted(named ^ inst)
    entries = (A.GATHER, A.STITCH, A.D8G, A.D8M, A.METRICS, A.RGB2Y)
    assert {r[0] for r in A.TABLE} == set(entries)
    for r in A.TABLE:
        assert len(r) == 5
        if r[3] is None:
            assert r[1] == "no instance" and "refused" in r[2] and r[4] == ()
    assert [r[0] for r in A.TABLE if r[3] is None] == list(entries), "one refusal row per entry point"
    names = [A.row_id(r) for r in CASES]
    assert len(set(names)) == len(names)
    unreachable = [r for r in A.TABLE if r[3] is not None and r[3].get("unreachable")]
    assert len(unreachable) == 1 and unreachable[0][0] == A.STITCH and "unreachable in a test" in unreachable[0][2]
    from tgsr_amd import _lib
    for e, nargs in ((A.GATHER, 13), (A.STITCH, 15), (A.D8G, 16), (A.D8M, 18), (A.METRICS, 11), (A.WS_ELEMS, 4), (A.RGB2Y, 6)):
        assert len(_lib.SIGNATURES[e][1]) == nargs, e


# (what stands in the launcher, what stands in a row's condition; None: the same text)
CONDITIONS = {
    "tgsr_tiles.hip": (
        ("(W % 4 == 0) && aligned_to(img, in_align) && (!img2 || aligned_to(img2, in_align))", "aligned_to(img, in_align)"),
        ("(!img2 || aligned_to(img2, in_align))", None), ("(tw % 4 == 0) && aligned_to(out, 16) && (!out2 || aligned_to(out2, 16))", "tw % 4 == 0"),
        ("(!out2 || aligned_to(out2, 16))", None), ("W % 4 == 0", None), ("vec_in && (x0 & 3) == 0", "vin = vec_in && x0 % 4 == 0"),
        ("img2 ? 2u : 1u", None), ("!tile_desc_ok", None),
        ("((int64_t)s * tw) % 4 == 0 && aligned_to(src[e], 16) && src_stride[e] % 4 == 0",
         "(s tw) % 4 == 0 && aligned_to(src[e], 16) && src_stride[e] % 4 == 0"),
        ("((int64_t)s * W) % 4 == 0 && aligned_to(dst[e], out_u8[e] ? 4 : 16)", "(s W) % 4 == 0 && aligned_to(dst[e], out_u8[e] ? 4 : 16)"),
        ("L.vec_src[e] != 0 && (sx0 & 3) == 0", "vsrc = vec_src && (s x0) % 4 == 0"), ("vdst ? (xa & ~3) : xa", "gx = vdst ? xa & ~3 : xa"),
        ("src_stride[e] < block && Tb > 1", None), ("items <= (int64_t)0x7fffffff - step", None)),
    "tgsr_ensemble.hip": (
        ("(W % 4 == 0) && d8_aligned(img, in_align) && (!img2 || d8_aligned(img2, in_align))", "d8_aligned(img, in_align)"),
        ("(!img2 || d8_aligned(img2, in_align))", None),
        ("(tw % 4 == 0) && (th % 4 == 0) && d8_aligned(out, 16) && (!out2 || d8_aligned(out2, 16))", "d8_aligned(out, 16)"),
        ("(!out2 || d8_aligned(out2, 16))", None), ("th % 4 == 0", None), ("two ? blockIdx.z >> 1 : blockIdx.z", "blockIdx.z = 2 * image + which"),
        ("blockIdx.z / N", "blockIdx.z = entry * N + image"), ("!d8_desc_ok", None),
        ("((int64_t)s * tw) % 4 == 0 && ((int64_t)s * th) % 4 == 0 && d8_aligned(srcA[e], 16) && (!b || d8_aligned(b, 16)) &&",
         "(s tw) % 4 == 0 && (s th) % 4 == 0 && d8_aligned(srcA[e], 16) && (!b || d8_aligned(b, 16)) && src_stride[e] % 4 == 0"),
        ("((int64_t)s * W) % 4 == 0 && d8_aligned(dst[e], out_u8[e] ? 4 : 16)", "d8_aligned(dst[e], out_u8[e] ? 4 : 16)"),
        ("(b != nullptr) != (nk == 4)", None), ("N * (two + 1) > 65535", None), ("n * N > 65535", None)),
    "tgsr_metrics.hip": (
        ("if (sr_f32 && hr_f32)", "sr_f32 && hr_f32"), ("else if (sr_f32)", "else sr_f32"), ("else if (hr_f32)", "else hr_f32"),
        ("grid(tiles_x * tiles_y, B)", None), ("g > 16384 ? 16384 : g", None)),
}


def test_every_launcher_condition_stands_in_a_row():
    conds = " ".join(r[2] for r in A.TABLE)
    for name, pairs in CONDITIONS.items():
        for in_source, in_row in pairs:
            assert in_source.replace("n * N > 65535", "(int64_t)n * N > 65535").replace("N * (two + 1) > 65535", "(int64_t)N * (two + 1) > 65535") in TEXT[
                name], in_source + " is no longer in " + name
            assert (in_row or in_source) in conds, (in_row or in_source) + " stands in no row"
    # what the launchers refuse, as the refusal rows and the refusal list say it
    for name, snippet in (("tgsr_tiles.hip", "!img || !out || (img2 != nullptr) != (out2 != nullptr)"),
                          ("tgsr_tiles.hip", "!table_host || !table_dev || Tb < 1 || Tb > 65535"),
                          ("tgsr_tiles.hip", "n < 1 || n > TGSR_STITCH_MAX || !src || !src_stride || !dst || !C || !scale || !out_u8"),
                          ("tgsr_tiles.hip", "!src[e] || !dst[e] || C[e] < 1 || C[e] > 65535 || s < 1 || s > 64"),
                          ("tgsr_ensemble.hip", "Tb < 1 || Tb > 65535 || N < 1 || N > kD8MaxN"), ("tgsr_ensemble.hip", "if (src_stride[e] < block) return TGSR_EINVAL;"),
                          ("tgsr_ensemble.hip", "if (nk == 8) return k0 == 0 && th == tw;"), ("tgsr_ensemble.hip", "return nk == 4 && (k0 == 0 || k0 == 4);"),
                          ("tgsr_ensemble.hip", "(nk == 4 && !srcB)"), ("tgsr_metrics.hip", "!sr || !hr || !ws || !out || !metrics_shape_ok(B, H, W, shave)"),
                          ("tgsr_metrics.hip", "B >= 1 && B <= 65535 && H >= 1 && W >= 1 && shave >= 0"),
                          ("tgsr_metrics.hip", "!rgb || !y || B < 1 || H < 1 || W < 1")):
        assert snippet in TEXT[name], snippet
    for name in ("tgsr_tiles.hip", "tgsr_ensemble.hip"):
        assert "H > kTileMaxSide || W > kTileMaxSide || th < 1 || tw < 1 || th > H || tw > W ||" in TEXT[name]
        assert "constexpr int kTileMaxSide = 1 << 20;" in TEXT[name] and "constexpr int kTileMaxTile = 4096;" in TEXT[name]
    assert "constexpr int kD8MaxN = 4096;" in TEXT["tgsr_ensemble.hip"] and "#define TGSR_STITCH_MAX 12" in open(
        os.path.join(CSRC, "..", "..", "include", "tgsr_hip.h")).read()
    assert A.STITCH_MAX * 4096 < 65535 and 2 * 4096 < 65535, "the two count refusals behind N <= 4096 stay unreachable"
    names = [n for n, *_ in A.refusals()]
    assert len(set(names)) == len(names)
    table_rules = [n for n, _ in A._table_refusals()]
    assert len(table_rules) == 27 and sum(n.startswith("row-") for n in table_rules) == 12
    for e in (A.GATHER, A.STITCH, A.D8G, A.D8M):
        for n in table_rules:
            assert e[5:] + "-" + n in names
    for wanted in ["tile_gather-img-null", "tile_gather-img2-null", "tile_gather-out2-null", "d8_gather-out-null", "d8_gather-N-4097", "d8_gather-k0-1",
                   "d8_gather-nk-8-th-not-tw", "tile_stitch-n-0", "tile_stitch-n-13", "tile_stitch-src-entry-null", "tile_stitch-dst-entry-null",
                   "tile_stitch-C-0", "tile_stitch-C-65536", "tile_stitch-s-0", "tile_stitch-s-65", "tile_stitch-stride-below-block",
                   "d8_merge-stride-below-block", "d8_merge-stride-0-Tb-1", "d8_merge-nk-8-with-srcB", "d8_merge-nk-4-srcB-null",
                   "d8_merge-nk-4-srcB-entry-null", "d8_merge-N-0", "d8_merge-N-4097", "sr_metrics-B-0", "sr_metrics-B-65536", "sr_metrics-shave-negative",
                   "sr_metrics-crop-10-high", "sr_metrics-crop-10-wide", "sr_metrics-ws-null", "rgb_to_y_u8-B-0", "rgb_to_y_u8-H-0", "rgb_to_y_u8-W-0"] + [
                       e + "-" + n + "-null" for e in ("tile_stitch", "d8_merge") for n in ("src", "src_stride", "dst", "C", "scale", "out_u8")]:
        assert wanted in names, wanted


def test_every_refusal_returns_in_front_of_the_first_launch(monkeypatch):
    """The refusals of test_hip_upscale_abi.test_refusals on host memory: whatever passed one of them on to a launch would hand a
    kernel a host pointer - or, without a device, answer TGSR_ELAUNCH.  The code each gives, and an untouched arena, say none does."""
    monkeypatch.setattr(A, "DEV", "cpu")
    monkeypatch.setattr(A, "_stream", lambda: None)
    A.test_refusals()


def test_the_refusal_calls_are_valid_but_for_the_one_thing():
    R = A.REF
    for row in A.REF_TABLE:
        assert A.desc_ok(row, R["H"], R["W"], R["th"], R["tw"])
        assert A.desc_ok(row, R["H"], R["W"], 2, R["tw"]), "th = 2 (nk-8-th-not-tw) breaks no table rule"
    assert R["th"] == R["tw"] and R["th"] <= R["H"] and R["tw"] <= R["W"] and 1 <= R["N"] <= 4096 and 1 <= R["n"] <= 12
    assert 1 <= R["C"] <= 65535 and 1 <= R["s"] <= 64
    assert R["MH"] - 2 * R["shave"] == 11 and R["MW"] - 2 * R["shave"] == 12, "the smallest crop the entry accepts, one column to spare"
    for name, kw in A._table_refusals():
        if "row" in kw:                                            # each changed row fails, and only because of that number
            t = A.REF_TABLE.copy()
            i, col, v = kw["row"]
            t[i, col] = v
            assert not A.desc_ok(t[i], R["H"], R["W"], R["th"], R["tw"]), name
            assert A.desc_ok(t[1 - i], R["H"], R["W"], R["th"], R["tw"])


# ---- the launch arithmetic ----
def test_the_grid_caps_are_the_launchers():
    t, e, m = TEXT["tgsr_tiles.hip"], TEXT["tgsr_ensemble.hip"], TEXT["tgsr_metrics.hip"]
    for text, snippet in ((t, "const int items = 3 * th * ((tw + 3) / 4);"), (t, "(items + 255) / 256 < 64 ? (items + 255) / 256 : 64"),
                          (t, "const int64_t items = (int64_t)C[e] * s * th * ((s * tw + 3) / 4 + 1);"), (t, "gx < 256 ? gx : 256"),
                          (t, "const int ng = (xb - gx + 3) >> 2, rows = yb - ya;"), (t, "const uint32_t step = gridDim.x * 256u"),
                          (e, "const int blocks = 3 * ((th + kBlk - 1) / kBlk) * ((tw + kBlk - 1) / kBlk);"), (e, "blocks < 1024 ? blocks : 1024"),
                          (e, "(int64_t)C[e] * ((s * th + kBlk - 1) / kBlk) * ((s * tw + 3 + kBlk - 1) / kBlk)"), (e, "most < 4096 ? most : 4096"),
                          (e, "blk < C * nby * nbx; blk += gridDim.x"), (e, "constexpr int kBlk = 32;"),
                          (e, "const int nbx = (xb - gx + kBlk - 1) / kBlk, nby = (yb - ya + kBlk - 1) / kBlk;"),
                          (m, "const int64_t g = (total + 255) / 256;"), (m, "static inline int metrics_tiles(int n) { return (n + kMT - 1) / kMT; }"),
                          (m, "constexpr int kMT = 32;")):
        assert snippet in text, snippet


def _g(th, tw):
    return dict(th=th, tw=tw)


def test_second_trips_are_where_the_rows_say():
    named = lambda r: "second-trip" in r[3]["name"]                # noqa: E731
    for r in CASES:
        c = r[3]
        if r[0] == A.GATHER:
            trips = A.gather_plan(c)["trips"]
        elif r[0] == A.STITCH:
            blocks = A.stitch_plan(c)["blocks"]
            walked = max(A.stitch_items(c, e, row) for e in c["entries"] for row in c["table"])
            assert walked <= A.stitch_plan(c)["most"], "the launcher's bound covers what the kernel walks"
            trips = -(-walked // (blocks * 256))
        elif r[0] == A.D8G:
            trips = A.d8g_plan(c)["trips"]
        elif r[0] == A.D8M:
            p = A.d8m_plan(c)
            assert p["walked"] <= p["most"]
            trips = p["trips"]
        elif r[0] == A.RGB2Y:
            trips = A.y_plan(c)["trips"]
        else:
            continue
        assert trips == (2 if named(r) else 1), (A.row_id(r), trips)
        assert named(r) == ("second trip" in r[2]), A.row_id(r)
    count = {e: sum(named(r) for r in CASES if r[0] == e) for e in (A.GATHER, A.STITCH, A.D8G, A.D8M, A.RGB2Y, A.METRICS)}
    assert count == {A.GATHER: 4, A.STITCH: 1, A.D8G: 2, A.D8M: 1, A.RGB2Y: 1, A.METRICS: 0}
    # the neighbours: one trip each
    assert A.gather_plan(_g(148, 148))["items"] == 16428 and A.gather_plan(_g(147, 148))["items"] == 16317 <= 64 * 256
    assert A.gather_plan(_g(4096, 5))["items"] == 24576 and A.gather_plan(_g(147, 148))["trips"] == 1
    trip = next(r[3] for r in CASES if r[3]["name"] == "second-trip-37x40-37x37")
    assert A.stitch_plan(trip)["most"] == 66600 and A.stitch_plan(dict(trip, th=32, tw=32))["most"] == 49920 <= 256 * 256
    assert A.stitch_items(trip, trip["entries"][0], trip["table"][0]) == 65712 > 256 * 256
    assert A.d8g_plan(_g(577, 577))["blocks"] == 1083 and A.d8g_plan(_g(576, 576))["blocks"] == 972 and A.d8g_plan(_g(4096, 65))["blocks"] == 1152
    assert 4 * 3 * 4096 * 65 * 4 < 4 * 3 * 577 * 577 * 4, "4096 x 65 is the cheaper output"
    trip = next(r[3] for r in CASES if r[3]["name"] == "second-trip-nk4-4096x1")
    assert A.d8m_plan(trip) == dict(most=4224, grid=4096, walked=4224, trips=2)
    assert A.d8m_plan(dict(trip, entries=(A._e(32, 1),)))["trips"] == 1
    assert A.y_plan(dict(B=3, H=1183, W=1183))["total"] == 4198467 > 16384 * 256 > 2 * 1183 * 1183, "the second trip starts inside the last image"


def test_the_64_bit_item_loop_is_out_of_reach():
    """items = C rows ng > 2^31 - step, step <= 65 536.  A destination row has at least 4 (ng - 1) elements and there are C rows of
    them (per owned row): more than 4 (items - C rows) elements.  With C rows <= 65535 * 2^18 the smallest such destination lies
    where ng is largest, (2^18 + 3) / 4 + 1 groups: C rows >= (2^31 - 65536) / 65537, and 4 (ng - 1) C rows >= 2^32 elements."""
    ng_max = (64 * 4096 + 3) // 4 + 1
    need = (1 << 31) - 65536
    c_rows = -(-need // ng_max)
    elements = c_rows * 4 * (ng_max - 1)
    assert ng_max == 65537 and elements >= (1 << 32) - (1 << 20)
    assert elements * 1 > 4 * (1 << 30) - (1 << 20) and elements * 4 > 15 * (1 << 30), "about 4 GiB of uint8 / 16 GiB of float32, and 16 GiB of source"
    assert "items <= (int64_t)0x7fffffff - step" in TEXT["tgsr_tiles.hip"]


# ---- the cases are the ones their rows describe ----
def test_the_cases_are_the_ones_their_rows_describe():
    for r in CASES:
        c = r[3]
        if r[0] in (A.GATHER, A.D8G):
            d8 = r[0] == A.D8G
            assert A.gather_flags(c, d8) == c["want"], A.row_id(r)
            assert all(A.desc_ok(row, c["H"], c["W"], c["th"], c["tw"]) for row in c["table"]), A.row_id(r)
            assert set(c["mis"]) <= {"img", "img2", "out", "out2"} and (c["two"] or not {"img2", "out2"} & set(c["mis"]))
            assert ("vec_in = 0" in r[2]) <= (c["want"][0] == 0) and ("vec_out = 0" in r[2]) <= (c["want"][1] == 0), A.row_id(r)
            if "fails alone" in r[2]:                              # exactly one term of exactly one flag
                terms_in = [c["W"] % 4 == 0, "img" not in c["mis"], "img2" not in c["mis"]]
                terms_out = [c["tw"] % 4 == 0, (not d8) or c["th"] % 4 == 0, "out" not in c["mis"], "out2" not in c["mis"]]
                assert (terms_in + terms_out).count(False) == 1, A.row_id(r)
            if d8:
                assert (c["k0"], c["nk"]) in ((0, 8), (0, 4), (4, 4)) and (c["nk"] == 4 or c["th"] == c["tw"]) and 1 <= c["N"] <= 4096
        if r[0] in (A.STITCH, A.D8M):
            assert all(A.desc_ok(row, c["H"], c["W"], c["th"], c["tw"]) for row in c["table"]), A.row_id(r)
            assert 1 <= len(c["entries"]) <= A.STITCH_MAX and all(1 <= e["C"] <= 65535 and 1 <= e["s"] <= 64 for e in c["entries"])
            flags = [(A.merge_flags if r[0] == A.D8M else A.stitch_flags)(c, e) for e in c["entries"]]
            if "vec_src = 0" in r[2]:
                assert all(f[0] == 0 for f in flags), A.row_id(r)
            if "vec_dst = 0" in r[2]:
                assert all(f[1] == 0 for f in flags), A.row_id(r)
            if "fails alone" in r[2] and "vec_src = 0" in r[2]:
                assert all(f[1] == 1 or (e["s"] * c["W"]) % 4 for f, e in zip(flags, c["entries"])), A.row_id(r)
            if r[0] == A.D8M:
                assert c["nk"] in (4, 8) and (c["nk"] == 4 or c["th"] == c["tw"]) and 1 <= c["N"] <= 4096
        if c.get("bad"):
            i, how = c["bad"]
            dev = A.dev_table(c)
            assert 0 < i < len(dev) - 1, "a middle row"
            assert not A.desc_ok(dev[i], c["H"], c["W"], c["th"], c["tw"]) and A.desc_ok(c["table"][i], c["H"], c["W"], c["th"], c["tw"])
            assert (np.delete(dev, i, 0) == np.delete(c["table"], i, 0)).all() and "table_dev row %d" % i in r[2]
            assert dev[i, 1] == c["W"] - c["tw"] + 1 if how == "x0" else dev[i, 3] == dev[i, 2]
    R = {A.row_id(r): r[3] for r in CASES}
    x0s = lambda c: sorted({int(x) for x in c["table"][:, 1]})     # noqa: E731
    for dt in ("u8", "f32"):
        assert x0s(R["tile_gather-%s-vec-9x16-5x8" % dt]) == [0, 1, 3, 4, 6, 8]
        c = R["tile_gather-%s-repeat-unordered-9x16-5x8" % dt]
        rows = [tuple(row) for row in c["table"].tolist()]
        assert len(set(rows)) < len(rows) and rows != sorted(rows)
        assert R["tile_gather-%s-no-img2-9x16-5x8" % dt]["two"] is False
        c = R["tile_gather-%s-1x1" % dt]
        assert (c["H"], c["W"], c["th"], c["tw"]) == (1, 1, 1, 1)
        for r in A._rows(A.D8G):
            if r[3]["dt"] == dt and not r[3]["name"].endswith("4096x65"):
                assert {int(x) % 4 for x in r[3]["table"][:, 1]} == {0, 1, 2, 3}, A.row_id(r)
        sides = {(r[3]["th"] % 32 if r[3]["th"] > 32 else r[3]["th"], r[3]["tw"] % 32 if r[3]["tw"] > 32 else r[3]["tw"], r[3]["k0"], r[3]["nk"])
                 for r in A._rows(A.D8G) if r[3]["dt"] == dt}
        for want in ((8, 8, 0, 8), (32, 32, 0, 8), (1, 1, 0, 8), (31, 31, 0, 8), (8, 8, 0, 4), (8, 8, 4, 4)) + tuple(
                (a, b, k0, 4) for k0 in (0, 4) for a, b in ((1, 32), (31, 32), (32, 1), (32, 31))):
            assert want in sides, want
        assert {(r[3]["N"], r[3]["two"]) for r in A._rows(A.D8G)} >= {(1, True), (1, False), (3, True)}
    main = R["tile_stitch-n12-7x16-4x8"]
    assert len(main["entries"]) == 12 == A.STITCH_MAX and {e["C"] for e in main["entries"]} == {1, 3, 18}
    assert {e["s"] for e in main["entries"]} == {1, 2, 3, 8, 64} and {e["u8"] for e in main["entries"]} == {0, 1}
    assert sorted({int(v) for v in main["table"][:, 4]}) == [0, 7, 13] and sorted({int(v) for v in main["table"][:, 5]}) == [7, 13, 16]
    assert all(A.stitch_flags(main, e) == (1, 1) for e in main["entries"])
    assert sorted(e["doff"] for e in R["tile_stitch-dst-off-7x16-4x8"]["entries"] if e["u8"]) == [1, 2, 3]
    c = R["tile_stitch-Tb1-stride0-5x8"]
    assert len(c["table"]) == 1 and c["zero_stride"]
    c = R["tile_stitch-padded-7x16-4x8"]
    assert (c["table"][-1] == c["table"][-2]).all() and len(c["table"]) == 10
    for name in ("d8_merge-nk4-N3-padded-7x16-4x8", "d8_merge-nk8-padded-7x7-4x4"):
        assert (R[name]["table"][-1] == R[name]["table"][-2]).all()
    for name in ("tile_stitch-hole-7x16-4x8", "d8_merge-nk8-N3-hole-7x8-4x4", "d8_merge-nk4-hole-7x16-4x8"):
        c = R[name]
        own = A.owned_mask(c["table"], 1, (c["H"], c["W"]))
        assert 0 < int((~own).sum()) < own.size, "a hole, and not the whole image"
    for name, nk in (("d8_merge-nk8-n12-3x3-2x2", 8), ("d8_merge-nk4-n12-3x8-2x4", 4)):
        c = R[name]
        assert c["nk"] == nk and len(c["entries"]) == 12 and {e["s"] for e in c["entries"]} == {1, 2, 3, 8, 64}
        assert any(e["extra"] for e in c["entries"]) and A.owned_mask(c["table"], 1, (c["H"], c["W"])).all()
    c = R["d8_merge-nk4-n12-3x8-2x4"]
    x_lo = {(e["s"] * int(row[4]) & ~3) - e["s"] * int(row[4]) for e in c["entries"] for row in c["table"] if A.merge_flags(c, e)[1]}
    assert x_lo >= {0, -1, -2, -3}, "first columns 1, 2 and 3 modulo 4 under vdst"
    assert {r[3]["N"] for r in A._rows(A.D8M)} == {1, 3}
    crops = {(c["hc"], c["wc"]) for c in R.values() if "hc" in c}
    assert crops == {(11, 11), (33, 43), (37, 70), (43, 43)} and {c["shave"] for c in R.values() if "hc" in c} == {0, 3, 4}
    assert {c["B"] for c in R.values() if "hc" in c} == {1, 3}
    assert A.metrics_tiles(dict(hc=37, wc=70)) == (2, 3) and A.metrics_tiles(dict(hc=33, wc=43)) == (2, 2) and 37 - 32 == 5 and 33 - 32 == 1
    assert len([cy for cy in range(32, 43) if 5 <= cy < 43 - 5]) == 6
    y = R["rgb_to_y_u8-B3-5x7"]
    assert (y["H"] * y["W"]) % 4 != 0 and y["leads"]


def test_the_inputs_carry_what_the_rows_promise():
    c = next(r[3] for r in CASES if r[3]["name"] == "nk4-n12-3x8-2x4")
    src_a, src_b, _ = A._merge_inputs(c["name"])[3]
    win = np.stack([A.d8_back((src_a if k < 4 else src_b).reshape((1, 6, 4) + (src_a if k < 4 else src_b).shape[1:])[0, :, k % 4], k) for k in range(8)])
    asc, desc = EM.mean8(list(win)), EM.mean8(list(win[::-1]))
    assert (asc.view(np.int32) != desc.view(np.int32)).any(), "the order of the eight additions shows"
    ties = A._ties()
    assert ties.size >= 8 and np.isin(asc, ties).sum() >= asc.size // 8, "means that sit on a rounding tie of tgsr_to_uint8"
    f32 = np.float32
    a = list(A.ORDER_A)
    s = f32(0)
    for v in a:
        s = f32(s + v)
    assert s == f32(1) and f32(f32(f32(a[0] + a[1]) + f32(a[2] + a[3])) + f32(0)) == f32(1 + 2.0 ** -23)
    sr_f, hr_f, sr_u, hr_u = A._metrics_inputs(A.M_CASES[0][0]["name"])
    assert np.isin(sr_f, ties).sum() > sr_f.size // 10 and (np.abs(hr_f) > 1).any() and (sr_u != hr_u).any()
    img = A._image("f32", (3, 9, 16), 1)
    assert np.signbit(img[img == 0]).any() and (np.abs(img[img != 0]) < 1e-38).any()


# ---- the models against something independent ----
def _slices_gather(img, table, th, tw):
    out = np.empty((len(table), 3, th, tw), np.float32)
    for t, row in enumerate(table):
        for ch in range(3):
            for y in range(th):
                for x in range(tw):
                    v = img[ch, row[0] + y, row[1] + x]
                    out[t, ch, y, x] = (np.float32(v) / np.float32(255) - np.float32(0.5)) / np.float32(0.5) if img.dtype == np.uint8 else v
    return out


def test_gather_and_stitch_models_against_plain_loops():
    for r in A._rows(A.GATHER):
        c = r[3]
        if c["th"] * c["tw"] > 64:
            continue
        img, img2 = A.gather_inputs(c)
        loops = _slices_gather(img, c["table"], c["th"], c["tw"])
        assert loops.tobytes() == TM.gather(img, c["table"], c["th"], c["tw"]).tobytes()
        assert loops.tobytes() == A.gather_model(img, img2, c["table"], c["th"], c["tw"])[0].tobytes()
    c = next(r[3] for r in A._rows(A.STITCH) if r[3]["name"] == "hole-7x16-4x8")
    for e, (tiles, prior) in zip(c["entries"], A._stitch_inputs(c["name"])):
        s, out = e["s"], prior.copy()
        for t, (y0, x0, oy0, oy1, ox0, ox1) in enumerate(c["table"].tolist()):
            for y in range(s * oy0, s * oy1):
                for x in range(s * ox0, s * ox1):
                    v = tiles[t, :, y - s * y0, x - s * x0]
                    out[:, y, x] = np.round(np.clip((v + np.float32(1)) * np.float32(127.5), 0, 255)).astype(np.uint8) if e["u8"] else v
        assert out.tobytes() == TM.stitch(tiles, c["table"], c["th"], prior.copy()).tobytes()


def _flat(rows, stride):
    """[R][block] as it lies in memory with `stride` between the rows (0: one row)."""
    R, block = rows.shape[0], rows[0].size
    flat = np.full((R - 1) * stride + block, A.FILL, np.float32)
    for t in range(R):
        flat[t * stride:t * stride + block] = rows[t].reshape(-1)
    return flat


def stitch_outputs(c, variant=""):
    out = []
    for e, (tiles, prior) in zip(c["entries"], A._stitch_inputs(c["name"])):
        stride = 0 if c["zero_stride"] else tiles[0].size + e["extra"]
        out.append(A.stitch_model(_flat(tiles, stride), stride, e["C"], e["s"], c["table"], c["th"], c["tw"], prior.copy(), A.stitch_flags(c, e)[1],
                                  variant, rows=A.good_rows(c)))
    return out


def merge_outputs(c, variant=""):
    return [A.merge_model(src_a, src_b, c["table"], c["th"], c["tw"], prior.copy(), variant, rows=A.good_rows(c))
            for src_a, src_b, prior in A._merge_inputs(c["name"])]


def gather_outputs(c, d8, variant=""):
    img, img2 = A.gather_inputs(c)
    if d8:
        outs = [A.d8_gather_model(x, c["table"], c["th"], c["tw"], c["k0"], c["nk"], variant) for x in (img, img2) if x is not None]
    else:
        outs = [o for o in A.gather_model(img, img2, c["table"], c["th"], c["tw"], variant) if o is not None]
    if c["bad"]:                                                   # the skipped window shows nothing
        for o in outs:
            (o[:, c["bad"][0]] if d8 else o[c["bad"][0]])[...] = 0
    return outs


def metrics_output(c, variant=""):
    _sr_f, _hr_f, sr_u, hr_u = A._metrics_inputs(c["name"])
    return A.metrics_tiled_model(sr_u, hr_u, c["shave"], variant)


def outputs(row, variant=""):
    entry, c = row[0], row[3]
    if entry in (A.GATHER, A.D8G):
        return gather_outputs(c, entry == A.D8G, variant)
    if entry == A.STITCH:
        return stitch_outputs(c, variant)
    if entry == A.D8M:
        return merge_outputs(c, variant)
    if entry == A.METRICS:
        return [metrics_output(c, variant)]
    return [A.rgb2y_model(A._y_input(c["B"], c["H"], c["W"]), variant)]


def differ(row, got, ref):
    """Would the GPU test's comparison tell `got` from `ref`?"""
    if row[0] != A.METRICS:
        return any(g.tobytes() != r.tobytes() for g, r in zip(got, ref))
    windows = (row[3]["hc"] - 10) * (row[3]["wc"] - 10)
    g, r = got[0], ref[0]
    return bool((g[:, :2] != r[:, :2]).any() or (np.abs(g[:, 2] - r[:, 2]) / windows > 2 * A.SSIM_TOL).any())


@pytest.mark.parametrize("row", CASES, ids=A.row_id)
def test_models_and_variants(row):
    """The variant-free model below the wrong kernels IS the model the GPU test compares with; each wrong kernel the row lists gives
    other bits on the row's input."""
    entry, c, catch = row[0], row[3], row[4]
    ref = outputs(row)
    if entry == A.GATHER:
        img, img2 = A.gather_inputs(c)
        want = [TM.gather(x, c["table"], c["th"], c["tw"]) for x in (img, img2) if x is not None]
    elif entry == A.D8G:
        img, img2 = A.gather_inputs(c)
        want = [EM.gather(x, c["table"], c["th"], c["tw"], c["k0"], c["nk"]) for x in (img, img2) if x is not None]
    elif entry == A.STITCH:
        good = A.good_rows(c)
        want = [TM.stitch(tiles[good], c["table"][good], c["th"], prior.copy()) for tiles, prior in A._stitch_inputs(c["name"])]
    elif entry == A.D8M:
        want = [A.merge_expected(c, e, *x) for e, x in zip(c["entries"], A._merge_inputs(c["name"]))]
    elif entry == A.METRICS:
        _sr_f, _hr_f, sr_u, hr_u = A._metrics_inputs(c["name"])
        assert MM.check_rows(ref[0], sr_u, hr_u, c["shave"], A.SSIM_TOL) <= A.SSIM_TOL
        s_rgb, s_y, ss, (pixels, windows) = MM.rows(sr_u, hr_u, c["shave"])
        assert pixels == c["hc"] * c["wc"] and windows == (c["hc"] - 10) * (c["wc"] - 10)
        if c["same"]:
            assert s_rgb == [0] * c["B"] == s_y and np.allclose(ss, windows, rtol=0, atol=1e-9 * windows)
        want = None
    else:
        want = [MM.rgb2y(A._y_input(c["B"], c["H"], c["W"]))]
    if want is not None:
        if c.get("bad") and entry in (A.GATHER, A.D8G):
            for o in want:
                (o[:, c["bad"][0]] if entry == A.D8G else o[c["bad"][0]])[...] = 0
        assert len(want) == len(ref) and all(w.tobytes() == r.tobytes() and w.dtype == r.dtype for w, r in zip(want, ref)), "the model below the variants"
    allowed = {A.GATHER: A.V_GATHER, A.STITCH: A.V_STITCH, A.D8G: A.V_D8G, A.D8M: A.V_D8M, A.METRICS: A.V_METRICS, A.RGB2Y: A.V_Y}[entry]
    assert set(catch) <= set(allowed)
    for variant in catch:
        assert differ(row, outputs(row, variant), ref), "%s cannot tell %s from the right kernel" % (A.row_id(row), variant)


def test_every_variant_is_caught_by_some_row():
    for entry, variants in ((A.GATHER, A.V_GATHER), (A.STITCH, A.V_STITCH), (A.D8G, A.V_D8G), (A.D8M, A.V_D8M), (A.METRICS, A.V_METRICS),
                            (A.RGB2Y, A.V_Y)):
        caught = set().union(*(set(r[4]) for r in A._rows(entry)))
        assert caught == set(variants), (entry, sorted(caught ^ set(variants)))
    for dt in ("u8", "f32"):                                       # per kernel instance too
        for entry, variants in ((A.GATHER, A.V_GATHER), (A.D8G, A.V_D8G)):
            assert set().union(*(set(r[4]) for r in A._rows(entry) if r[3]["dt"] == dt)) == set(variants)
    for nk in (4, 8):
        caught = set().union(*(set(r[4]) for r in A._rows(A.D8M) if r[3]["nk"] == nk))
        assert caught >= {"mirror_first", "b0b1_swapped", "desc_sum", "pairwise_sum", "u8_trunc"}


def test_the_ensemble_model_against_the_index_maps_and_torch():
    from tgsr_amd import tiles
    win = np.arange(2 * 5 * 7, dtype=np.float32).reshape(2, 5, 7)
    for k in range(8):
        v = EM.variant(win, k)
        assert v.shape[-2:] == tiles.d8_shape(k, 5, 7) and np.array_equal(v, tiles.d8_apply(win, k))
        t = torch.from_numpy(win)
        t = t.transpose(1, 2) if k & 4 else t
        t = torch.flip(t, [1]) if k & 2 else t
        t = torch.flip(t, [2]) if k & 1 else t
        assert np.array_equal(v, t.contiguous().numpy())
        assert np.array_equal(EM.back(v, k), win) and np.array_equal(tiles.d8_invert(v, k), win)
        assert np.array_equal(A.d8_variant(win, k), v) and np.array_equal(A.d8_back(v, k), win)
        for variant in ("mirror_first", "b0b1_swapped"):           # the wrong transforms are transforms: they invert themselves
            assert np.array_equal(A.d8_back(A.d8_variant(win, k, variant), k, variant), win)


def test_metrics_model_against_the_recorded_values():
    """metrics_model's SSE and Y against tests/golden/sr_metrics.npz (the reference's own rgb2y / psnr on the fixture images), and
    the tiled restatement against metrics_model on them."""
    from tgsr_amd.metrics import psnr_from_sse
    golden, io = load_npz("sr_metrics.npz"), load_npz("io_pyramid.npz")
    for k in (1, 2, 3):
        a, b = io["ret%d_u8" % k], io["bic%d_u8" % k]
        assert np.array_equal(MM.rgb2y(a), golden["ret%d_y" % k]) and np.array_equal(A.rgb2y_model(b), golden["bic%d_y" % k])
        tiled = A.metrics_tiled_model(a[None], b[None], 0)
        MM.check_rows(tiled, a[None], b[None], 0, A.SSIM_TOL)
        for sse, n, want in ((tiled[0, 0], a.size, golden["pair%d_rgb" % k]), (tiled[0, 1], a.size // 3, golden["pair%d_y" % k])):
            got = psnr_from_sse(int(sse), n)
            assert np.float64(got[0]).tobytes() == want[0].tobytes() and np.float64(got[1]).tobytes() == want[1].tobytes()
    import test_hip_metrics
    assert A.SSIM_TOL == test_hip_metrics.SSIM_TOL == 1e-9
