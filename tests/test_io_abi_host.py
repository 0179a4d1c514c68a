"""CPU: what tests/test_hip_io_abi.py rests on, checked without a GPU.

  * the table against tgsr_amd/csrc/tgsr_io.hip: every hipLaunchKernelGGL and the hipMemcpyAsync branch has a row with a case, the
    table names nothing the file lacks, every condition of the three launchers stands in a row;
  * the launch arithmetic restated there: io_grid, the outputs of each launch, which of the 2 * passes blur launches writes `out`;
    every case named "second trip" makes one in the pass it names, and no other case makes any; tmp's byte count;
  * every refusal of the GPU file's test_refusals, here on host memory: each is a return in front of the first launch;
  * every case's input through the oracle AND through Pillow itself wherever Pillow can say the case - all but the hand-written
    tables and passes = 2 - and through the numpy models the variants are built on: the three agree byte for byte;
  * the product's host tables are the oracle's at every case's sizes, 1 x 300 -> 1 x 7 (ksize 87) included;
  * each row tells a right kernel from the wrong ones it lists: the model rebuilt with one change a kernel bug would make gives
    at least one other output byte (or bit) on that row's input, and every variant is caught by some row;
  * the hand-written tables make both arms of the clip fire; gaussian_box_params meets the entry's weight condition.
"""
import os
import re

import numpy as np
import pytest
import torch

import test_hip_io_abi as A
from oracle import tgsr_oracle_io as IO

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgsr_amd", "csrc", "tgsr_io.hip")


def source():
    return open(SOURCE).read()


# ---- the table against the source ----
def test_the_table_names_every_launch_of_the_source():
    text = source()
    inst = {re.sub(r"\s", "", m) for m in re.findall(r"hipLaunchKernelGGL\(\(?([A-Za-z_0-9]+(?:<[^>]*>)?)", text)}
    assert inst == {A.K_H, A.K_V, A.K_BH, A.K_BV, A.K_NORM}
    assert len(re.findall(r"hipMemcpyAsync\(", text)) == 1
    inst.add(A.K_COPY)
    with_case = " ".join(r[1] for r in A.TABLE if r[3] is not None)
    for k in inst:
        assert k in with_case, k + " has no row with a case"
    named = set(re.findall(r"[a-z_0-9]+_kernel(?:<[0-9]>)?|hipMemcpyAsync", " ".join(r[1] for r in A.TABLE)))
    assert named == inst, "the table names an instance the source does not launch: %s" % sorted(named ^ inst)
    assert {r[0] for r in A.TABLE} == {A.RESIZE, A.BLUR, A.NORM} == set(A.SPEC) == set(A.NULLS) == set(A.SIZES)
    for r in A.TABLE:
        assert len(r) == 5
        if r[3] is None:
            assert r[1] == "no instance" and "refused" in r[2] and r[4] == ()
    names = [r[3]["name"] for r in A.TABLE if r[3] is not None]
    assert len(set(names)) == len(names)
    from tgsr_amd import _lib
    for e, spec in A.SPEC.items():
        assert len(spec) + 1 == len(_lib.SIGNATURES[e][1]), e


def test_every_launcher_condition_stands_in_a_row():
    text, conds = source(), " ".join(r[2] for r in A.TABLE)
    for snippet in ("Wout != Win", "Hout != Hin", "doh && dov", "!doh && !dov", "k < passes", "((launches - 1 - k) & 1) ? tmp : out"):
        assert snippet in text, snippet + " is no longer in the launcher"
        assert snippet in conds, snippet + " stands in no row"
    # what the launchers refuse, as the refusal rows and the refusal list say it
    for snippet in ("!in || !out || N < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1", "doh && (!hbounds || !hcoef || hk < 1)",
                    "dov && (!vbounds || !vcoef || vk < 1)", "doh && dov && !tmp",
                    "!in || !tmp || !out || N < 1 || H < 1 || W < 1 || radius < 0 || passes < 1", "!in || !out || n < 1",
                    "(2 * (uint64_t)radius + 1) * (uint64_t)ww + 2 * (uint64_t)fw > (1ull << 24)", "io_overlap("):
        assert snippet in text, snippet
    names = [n for n, *_ in A.refusals()]
    assert len(set(names)) == len(names)
    for e in A.SPEC:
        for n in A.NULLS[e]:
            assert "%s-%s-null" % (e[5:], n) in names
        for n in A.SIZES[e]:
            assert "%s-%s-0" % (e[5:], n) in names and "%s-%s--1" % (e[5:], n) in names
    for wanted in ("resize_bilinear_u8-hk-0", "resize_bilinear_u8-vk-0", "resize_bilinear_u8-tmp-null", "resize_bilinear_u8-out-is-in",
                   "resize_bilinear_u8-tmp-is-in", "resize_bilinear_u8-tmp-is-out", "gaussian_blur_u8-radius-negative", "gaussian_blur_u8-passes-0",
                   "gaussian_blur_u8-weights-2^24+2", "gaussian_blur_u8-3ww-wraps-32-bits-to-5", "gaussian_blur_u8-out-is-in",
                   "gaussian_blur_u8-tmp-is-in", "gaussian_blur_u8-tmp-is-out"):
        assert wanted in names, wanted


def test_every_refusal_returns_in_front_of_the_first_launch(monkeypatch):
    """The refusals of test_hip_io_abi.test_refusals on host memory: whatever passed one of them on to a launch would hand a kernel
    a host pointer - or, without a device, answer TGSR_ELAUNCH.  The code each gives, and an untouched arena, say none does."""
    monkeypatch.setattr(A, "DEV", "cpu")
    monkeypatch.setattr(A, "_stream", lambda: None)
    A.test_refusals()


def test_the_refusal_calls_are_valid_but_for_the_one_thing():
    """The call the refusals start from: its tables stay inside the image, its operands have the sizes the header states, its
    weights are radius 2's, which the entry accepts (their sum is 2^24 exactly: the bound itself)."""
    from tgsr_amd.datasets import _resize_tables
    c = A.REF_RS
    for size, out in ((c["Win"], c["Wout"]), (c["Hin"], c["Hout"])):
        b, k, ks = _resize_tables(size, out)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= size).all() and (b[:, 1] <= ks).all() and k.shape == (out, ks)
    spec = {n: arg[0] for kind, n, *arg in A.SPEC[A.RESIZE] if kind == "img"}
    assert spec["in"] == c["N"] * c["Hin"] * c["Win"] and spec["tmp"] == c["N"] * c["Hin"] * c["Wout"]
    assert spec["out"] >= max(c["N"] * h * w for h in (c["Hout"], c["Hin"]) for w in (c["Wout"], c["Win"]))
    b = A.REF_BL
    assert (b["radius"], b["ww"], b["fw"]) == A.G2 and (2 * b["radius"] + 1) * b["ww"] + 2 * b["fw"] == 1 << 24
    assert all(arg[0] == b["N"] * b["H"] * b["W"] for kind, n, *arg in A.SPEC[A.BLUR] if kind == "img")
    assert (2 ** 32 + 5) == 3 * 1431655767 and (2 * (1 << 31)) % 2 ** 32 == 0          # the two sums that wrap 32 bits to a small one


# ---- the launch arithmetic ----
def test_io_grid_restated():
    m = re.search(r"static inline int io_grid\(int64_t n\) \{\s*const int64_t g = \(n \+ 255\) / 256;\s*return \(int\)\(g < 1 \? 1 : "
                  r"\(g > 8192 \? 8192 : g\)\);", source())
    assert m, "io_grid changed: restate it in test_hip_io_abi.io_plan"
    assert source().count("dim3(256)") == 5
    P = A.io_plan
    assert P(1) == dict(blocks=1, trips=1) and P(256)["blocks"] == 1 and P(257)["blocks"] == 2
    assert P(8192 * 256) == dict(blocks=8192, trips=1) and P(8192 * 256 + 1) == dict(blocks=8192, trips=2)


def test_second_trips_are_where_the_rows_say():
    for r in A._rows(A.RESIZE):
        c = r[3]
        launches = A.resize_launches(c)
        assert " + ".join(k for k, _, _ in launches) == r[1]
        assert [d for _, d, _ in launches] == (["tmp", "out"] if len(launches) == 2 else ["out"])
        trips = {k: A.io_plan(n)["trips"] for k, _, n in launches if k != A.K_COPY}
        if "second-trip-v" in c["name"]:
            assert trips == {A.K_H: 1, A.K_V: 2} and "second trip" in r[2]
        elif "second-trip-h" in c["name"]:
            assert trips == {A.K_H: 2} and "second trip" in r[2]
        else:
            assert all(t == 1 for t in trips.values()) and "second trip" not in r[2], c["name"]
        assert A.resize_tmp_bytes(c) == (c["N"] * c["hin"] * c["wout"] if r[1] == A.K_BOTH else 0)
    for r in A._rows(A.BLUR):
        c = r[3]
        trips = A.io_plan(c["N"] * c["H"] * c["W"])["trips"]
        assert (trips == 2) == ("second-trip" in c["name"]) == ("second trip" in r[2]) and trips <= 2
    for r in A._rows(A.NORM):
        trips = A.io_plan(r[3]["n"])["trips"]
        assert (trips == 2) == ("second-trip" in r[3]["name"]) == ("second trip" in r[2])
    assert sum("second-trip" in r[3]["name"] for r in A.TABLE if r[3] is not None) == 4


def test_the_last_blur_launch_writes_out():
    for passes in (1, 2, 3, 4):
        seq = A.blur_launches(dict(passes=passes))
        assert len(seq) == 2 * passes and seq[-1][1] == "out"
        assert [k for k, _ in seq] == [A.K_BH] * passes + [A.K_BV] * passes
        assert all(a[1] != b[1] for a, b in zip(seq, seq[1:])), "no launch reads what it writes"
        assert seq[0][1] == "tmp", "an even number of launches: the first one writes tmp, so `in` is only read"
    assert {r[3]["passes"] for r in A._rows(A.BLUR)} == {1, 2, 3}


def test_the_cases_are_the_ones_their_rows_describe():
    R = {r[3]["name"]: r[3] for r in A.TABLE if r[3] is not None}
    shape = lambda c: (c["N"], c["hin"], c["win"], c["hout"], c["wout"])  # noqa: E731
    assert shape(A.RS_DOWN) == (8, 37, 53, 16, 16) and shape(A.RS_UP) == (6, 5, 3, 13, 17) and shape(A.RS_H) == (6, 7, 53, 7, 20)
    assert shape(A.RS_V) == (6, 37, 9, 12, 9) and shape(A.RS_COPY) == (6, 5, 7, 5, 7) and shape(A.RS_1_UP) == (6, 1, 1, 4, 3)
    assert shape(A.RS_TO_1) == (6, 4, 3, 1, 1) and shape(A.RS_1_1) == (6, 1, 1, 1, 1) and shape(A.RS_17) == (1, 1, 300, 1, 7)
    assert shape(A.RS_HAND) == (6, 9, 11, 6, 8) and shape(A.RS_TRIP_V) == (3, 40, 40, 840, 840) and shape(A.RS_TRIP_H) == (3, 700, 10, 700, 1000)
    x = A.resize_input(A.RS_DOWN)
    assert (x[-2] == 0).all() and (x[-1] == 255).all() and len(np.unique(x[:-2])) == 256
    h, v = A.resize_tables(A.RS_TO_1)
    assert (h[2], v[2]) == (7, 9)
    h, v = A.resize_tables(A.RS_1_UP)
    assert (h[0][:, 1] == 1).all() and (v[0][:, 1] == 1).all()
    h, v = A.resize_tables(A.RS_17)
    assert v is None and h[2] == 87 and h[1].shape == (7, 87) and int(h[0][:, 1].max()) > 33
    assert A.G2 == (1, 4473924, 1677722) and A.G05 == (0, 15379114, 699051) and A.G5 == (4, 1694668, 762602)
    assert A.B1375 == (1, 4473924, 1677722) and A.B37 == (3, 1997287, 1398103) and A.G25_2 == (2, 2816175, 1348170)
    blur = [(c["N"], c["H"], c["W"]) for c in [A.BL_MAIN] + A.BL_SMALL]
    assert blur == [(6, 37, 53), (3, 1, 1), (3, 1, 2), (3, 2, 1), (3, 3, 3), (3, 1, 64), (3, 64, 1)]
    assert all(r[3]["leads"] for r in (A.TABLE[0],)) and sum(bool(c["leads"]) for c in R.values()) == 3
    assert {e for e in (A.RESIZE, A.BLUR, A.NORM) if any(r[3]["leads"] for r in A._rows(e))} == {A.RESIZE, A.BLUR, A.NORM}
    assert sorted(A.LEADS) == [(0, 0), (1, 3), (2, 2), (3, 1)]
    assert [A._tmp_lead(*l) for l in A.LEADS] == [0, 3, 0, 1]
    assert [int(v) for v in A.norm_input(A.NM_256)] == list(range(256)) and A.norm_input(A.NM_TRIP).size == 2097156


# ---- the references ----
def _pil_resize(a, hout, wout):
    Image = pytest.importorskip("PIL.Image")
    return np.stack([np.asarray(Image.fromarray(p).resize((wout, hout), Image.BILINEAR)) for p in a])


def _pil_blur(a, how):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    f = ImageFilter.GaussianBlur(how[1]) if how[0] == "gauss" else ImageFilter.BoxBlur(how[1])
    return np.stack([np.asarray(Image.fromarray(p).filter(f)) for p in a])


@pytest.mark.parametrize("row", A._rows(A.RESIZE), ids=A.row_id)
def test_resize_references_and_variants(row):
    _entry, _inst, _cond, c, catch = row
    x, ref = A.resize_input(c), A.resize_reference(c)
    htab, vtab = A.resize_tables(c)
    stats = {}
    assert np.array_equal(A.resize_model(x, htab, vtab, stats=stats), ref), "the model differs from the oracle"
    if c["tables"] == "hand":
        n = ref.size
        assert stats["low"] > n // 20 and stats["high"] > n // 20, stats           # both arms of the clip, each on a real share of the outputs
        print("IO_CLIP %s: ss < 0 on %d, ss > 255 on %d of %d outputs (both passes together)" % (c["name"], stats["low"], stats["high"], n))
    else:
        assert stats.get("low", 0) == 0 and stats.get("high", 0) == 0, "Pillow's tables never reach the clip"
        assert np.array_equal(_pil_resize(x, c["hout"], c["wout"]), ref), "the oracle differs from Pillow"
        for own, (size, out) in zip((htab, vtab), ((c["win"], c["wout"]), (c["hin"], c["hout"]))):   # the product's tables are the oracle's
            if own is not None:
                b, k = IO.resize_coeffs(size, out)
                assert np.array_equal(own[0], b) and np.array_equal(own[1], k) and own[2] == k.shape[1]
    for t, size in ((htab, c["win"]), (vtab, c["hin"])):                             # no row of a table reads outside the image
        if t is not None:
            assert (t[0][:, 0] >= 0).all() and (t[0][:, 1] >= 0).all() and (t[0][:, 0] + t[0][:, 1] <= size).all() and (t[0][:, 1] <= t[2]).all()
    assert set(catch) <= set(A.V_RESIZE)
    for variant in catch:
        assert not np.array_equal(A.resize_model(x, htab, vtab, variant), ref), "%s cannot tell %s from the right kernel" % (c["name"], variant)


@pytest.mark.parametrize("row", A._rows(A.BLUR), ids=A.row_id)
def test_blur_references_and_variants(row):
    _entry, _inst, _cond, c, catch = row
    x, ref = A.blur_input(c), A.blur_reference(c)
    r, ww, fw = c["params"]
    assert (2 * r + 1) * ww + 2 * fw <= 1 << 24
    assert np.array_equal(A.blur_model(x, r, ww, fw, c["passes"]), ref), "the model differs from the oracle"
    if c["pil"] is not None:
        how, radius = c["pil"]
        assert c["params"] == (IO.gaussian_box_params(radius, 3) if how == "gauss" else IO.box_blur_params(radius))
        assert c["passes"] == (3 if how == "gauss" else 1)
        assert np.array_equal(_pil_blur(x, c["pil"]), ref), "the oracle differs from Pillow"
    else:
        assert c["passes"] == 2
    assert set(catch) <= set(A.V_BLUR)
    for variant in catch:
        assert not np.array_equal(A.blur_model(x, r, ww, fw, c["passes"], variant), ref), "%s cannot tell %s from the right kernel" % (
            c["name"], variant)


@pytest.mark.parametrize("row", A._rows(A.NORM), ids=A.row_id)
def test_normalize_references_and_variants(row):
    _entry, _inst, _cond, c, catch = row
    x = A.norm_input(c)
    ref = IO.normalize(x)
    assert ref.dtype == np.float32 and np.array_equal(A.bits(A.norm_model(x)), A.bits(ref))
    exact = (x.astype(np.float64) / 255.0 - 0.5) / 0.5
    assert float(np.abs(ref.astype(np.float64) - exact).max()) <= 2.0 ** -23          # three roundings of values below 1
    assert np.array_equal(A.bits(torch.from_numpy(x.copy()).float().div(255.0).sub(0.5).div(0.5).numpy()), A.bits(ref))   # torch's fp32 too
    for variant in catch:
        assert not np.array_equal(A.bits(A.norm_model(x, variant)), A.bits(ref)), "%s cannot tell %s" % (c["name"], variant)


def test_every_variant_is_caught_by_some_row():
    for entry, variants in ((A.RESIZE, A.V_RESIZE), (A.BLUR, A.V_BLUR), (A.NORM, A.V_NORM)):
        caught = set().union(*(set(r[4]) for r in A._rows(entry)))
        assert caught == set(variants), sorted(caught ^ set(variants))
    only_hand = [r[3]["name"] for r in A._rows(A.RESIZE) if "no_clip" in r[4]]
    assert only_hand == [A.RS_HAND["name"]]


def test_normalize_model_round_trip_and_ends():
    x = A.norm_input(A.NM_256)
    f = IO.normalize(x)
    assert A.bits(f[0]) == A.bits(np.float32(-1.0)) and A.bits(f[255]) == A.bits(np.float32(1.0)) and (np.diff(f.astype(np.float64)) > 0).all()
    back = np.round(np.maximum(0, np.minimum(255, (f + np.float32(1.0)) * np.float32(127.5)))).astype(np.uint8)
    assert np.array_equal(back, x)


def test_gaussian_box_params_meet_the_weight_condition():
    """tgsr_gaussian_blur_u8 refuses (2 radius + 1) ww + 2 fw > 2^24.  Every caller in tgsr_amd/ passes gaussian_box_params(radius,
    3): fw = (2^24 - (2 r + 1) ww) // 2 makes the sum 2^24 or 2^24 - 1 whenever fw >= 0, over every radius a caller could mean."""
    from tgsr_amd.datasets import gaussian_box_params
    for passes in (1, 2, 3):
        for radius in np.arange(0.0, 64.0, 0.0625):
            r, ww, fw = gaussian_box_params(float(radius), passes)
            assert (r, ww, fw) == IO.gaussian_box_params(float(radius), passes)
            assert r >= 0 and ww >= 1 and fw >= 0 and (1 << 24) - 1 <= (2 * r + 1) * ww + 2 * fw <= 1 << 24, (radius, passes)
    for radius in (0.0, 0.3, 1.0, 1.375, 2.0, 3.7, 9.0):
        r, ww, fw = IO.box_blur_params(radius)
        assert fw >= 0 and (1 << 24) - 1 <= (2 * r + 1) * ww + 2 * fw <= 1 << 24
