"""CPU: what tests/test_hip_lp_abi.py rests on, checked without a GPU.

  * every refusal of the GPU file, here on host memory: each is a return in front of the first launch (whatever passed one of them
    on to a launch would hand a kernel a host pointer - or, without a device, answer TGSR_ELAUNCH);
  * the instance table against the kernel launches in tgsr_lp_conv.hip, tgsr_lp_misc.hip and tgsr_text_tail.hip: the set of
    instances the sources launch (template parameters expanded from the instantiations in the same files) equals the set the
    table names, every instance but lp_resblocks_kernel has a case, and each row's instance is the one the launcher's dispatch -
    restated here, with the rows of the 3x3 convolution asked of the library's own tgsr_lp_conv3x3_plan - takes for its case;
  * the inputs: every lp operand exactly representable in bf16 and in f16, every reference finite with a positive tolerance, every
    mask row with a word left, and the repository's CPU model of the path (oracle/tgsr_oracle_lp.py; fp32 arithmetic restated where
    it has no function) inside every case's tolerance of the fp64 reference - a tolerance the plain fp32 arithmetic misses says
    nothing about a kernel;
  * discrimination, once per case: the fp64 reference rebuilt with one change a kernel bug would make - a tap dropped, the halo row of
    the second tile row taken from the wrong tile, value and gate halves swapped, the residual read at offset 0, a sub-pixel phase
    swapped, one word's mask bit flipped, mask mode 1 for mode 0, one of the four head partials left out, alpha where the map applies,
    tanh dropped - leaves the tolerance in at least one element.  A case that cannot tell gets another shape, never a wider tolerance.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import test_hip_lp_abi as A
from oracle import tgsr_oracle_lp as OL

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgsr_amd", "csrc")
TYPES = [("bf16", torch.bfloat16, 2.0 ** -8), ("f16", torch.float16, 2.0 ** -11)]


def _L():
    from tgsr_amd import _lib
    return _lib.lib()


# ---- refusals on host memory ----
@pytest.mark.parametrize("name", [n for n, _run, _code in A.refusals()])
def test_every_refusal_returns_in_front_of_the_first_launch(name, monkeypatch):
    monkeypatch.setattr(A, "DEV", "cpu")
    monkeypatch.setattr(A, "_stream", lambda: None)
    A.test_refusal(name)


def test_the_refusals_cover_every_launcher():
    names = [n for n, _run, _code in A.refusals()]
    assert len(set(names)) == len(names)
    entries = {r[0] for r in A.TABLE}
    assert entries == set(A.REFUSALS), "an entry of the table without refusals, or refusals of an entry the table does not hold"
    for fn in (A.CONV, A.UP, A.UPHEAD, A.UPATT, A.STEM, A.STEMATT):
        assert any(t == "out_coff_negative" for t, _c, _o in A.REFUSALS[fn])
    for fn in (A.UPATT, A.STEMATT, A.ATTN):
        tags = {t for t, _c, _o in A.REFUSALS[fn]}
        assert {"c_coff_negative", "mask_mode_2", "c_code_over_h"} <= tags
    assert {"res_coff_negative", "res_2gib"} <= {t for t, _c, _o in A.REFUSALS[A.CONV]}


# ---- the table against the sources ----
def _text(name):
    return open(os.path.join(CSRC, name)).read()


def launched_instances():
    """Every kernel instance the three files launch, storage type as `T`, template parameters expanded from the instantiations of the
    launch helpers in the same files."""
    conv, misc = _text("tgsr_lp_conv.hip"), _text("tgsr_lp_misc.hip")
    raw = set()
    for text in (conv, misc, _text("tgsr_text_tail.hip")):
        raw |= {re.sub(r"\s", "", m) for m in re.findall(r"hipLaunchKernelGGL\(\(?([A-Za-z_0-9]+(?:<[^>]*>)?)", text)}
    out = set()
    pairs = sorted(set(re.findall(r"launch_lp_conv_epi<T, (\d+), (\d+)>", conv)))
    assert pairs == [("32", "32"), ("32", "64"), ("64", "128"), ("64", "64")]
    up_heads = sorted(set(re.findall(r"launch_lp_upconv<(?:BF16|F16), (\d)>", conv)))
    att_heads = sorted(set(re.findall(r"launch_lp_upconv_att<(?:BF16|F16), (\d)>", conv)))
    to3_k = sorted(set(re.findall(r"launch_to3_k<T, (\d)>", misc)))
    assert (up_heads, att_heads, to3_k) == (["0", "3", "5"], ["0", "3"], ["3", "5"])
    for k in raw:
        if k.startswith("lp_conv3x3_kernel<"):
            rows = k[-2]
            for cin, cout in pairs:                                   # launch_lp_conv_epi: GLU (with and without UP) from Cout = 64 on
                forms = [("kEpiRes", "false"), ("kEpiAffine", "false")] + ([("kEpiGlu", "true"), ("kEpiGlu", "false")] if int(cout) >= 64 else [])
                out |= {"lp_conv3x3_kernel<T,%s,%s,%s,%s,%s>" % (cin, cout, e, u, rows) for e, u in forms}
        elif k.startswith("lp_upconv_glu_kernel<"):
            att = k.endswith(",true>")
            cin = re.match(r"lp_upconv_glu_kernel<T,(\d+),HK", k).group(1)
            out |= {"lp_upconv_glu_kernel<T,%s,%s%s>" % (cin, h, ",true" if att else "") for h in (att_heads if att else up_heads)}
        elif k.startswith("lp_to3_kernel<"):
            out |= {k.replace("<T,K,", "<T,%s," % kk) for kk in to3_k}
        elif k.startswith("lp_convert_kernel<"):
            out.add(k)
        else:
            out.add(re.sub(r"<(BF16|F16)([,>])", r"<T\2", k))
    return out


def test_the_table_names_every_instance_the_sources_launch():
    inst = launched_instances()
    assert len(inst) == 28 + 8 + 10 + 5 + 2 + 2 + 6 + 1 + 1, sorted(inst)      # conv, upBlock, heads, combine, stem, convert, converters + packs + attention, chain, tail
    named = {r[1] for r in A.TABLE}
    assert named == inst, (sorted(named - inst), sorted(inst - named))
    with_case = {r[1] for r in A.TABLE if r[3] is not None}
    assert inst - with_case == {"lp_resblocks_kernel<T,4>"}
    none = [r for r in A.TABLE if r[3] is None]
    assert len(none) == 1 and none[0][0] == A.RESBLOCKS and "refusals only" in none[0][2] and "flag buffer" in none[0][2]
    assert 2 * 28 == 56                                                # the 56 lp_conv3x3_kernel instances: 28 here, each for two types
    ids = [A.row_id(r) for r in A._rows()]
    assert len(set(ids)) == len(ids)


def instance_of(c):
    """The launchers' dispatch, restated: the instance a case reaches."""
    k = c["kind"]
    if k == "conv":
        return A.conv_instance(c, _L().tgsr_lp_conv3x3_plan(c["B"], c["H"], c["W"]))
    if k == "up":
        return "lp_upconv_glu_kernel<T,%d,%d%s>" % (c["Cin"], c["hk"], ",true" if c["att"] else "")
    if k == "stem":
        return "lp_stem_kernel<T,%s>" % ("true" if c["att"] else "false")
    if k == "to3":
        return "lp_to3_kernel<T,%d,%s%s>" % (c["K"], A._ACT[c["act"]], ",true" if c["amap"] else "")
    if k == "combine":
        if not c["via_map"]:
            return "lp_head_combine_kernel"
        return "lp_head_combine_map_kernel<%s,%s>" % ("true" if c["high_tanh"] else "false", "true" if c["maps"] and any(c["maps"]) else "false")
    if k == "convert":
        return "lp_convert_kernel<%s>" % ("F16,BF16" if c["src"] == "f16" else "BF16,F16")
    return {"attn": "lp_word_attention_kernel<T>", "tail": "text_tail_kernel", "from": "lp_from_nchw_kernel<T>", "to": "lp_to_nchw_kernel<T>",
            A.PACK3: "lp_pack_conv3x3_kernel<T>", A.PACKUP: "lp_pack_upconv_kernel<T>", A.PACKTO3: "lp_pack_to3_kernel<T>"}[c.get("fn", k)]


@pytest.mark.parametrize("row", A._rows(), ids=A.row_id)
def test_each_row_reaches_the_instance_it_names(row):
    entry, instance, _cond, c = row
    assert instance_of(c) == instance
    fn = {"conv": A.CONV, "up": A.UPATT if c.get("att") else A.UPHEAD if c.get("hk") else A.UP, "stem": A.STEMATT if c.get("att") else A.STEM,
          "to3": A.TO3MAP if (c.get("amap") or c.get("act") == A.ACT_IDENT) else A.TO3, "attn": A.ATTN,
          "combine": A.COMBINEMAP if c.get("via_map") else A.COMBINE, "tail": A.TAIL, "from": A.FROM, "to": A.TO, "convert": A.CONVERT,
          "pack": c.get("fn")}[c["kind"]]
    assert fn == entry
    if c["kind"] == "conv":
        assert c["W"] % 32 == 0 and c["H"] % 4 == 0 and c["xcp"] >= c["Cin"] and (c["epi"] != "glu" or c["Cout"] >= 64)
        tiles8 = c["B"] * (c["H"] // 8) * (c["W"] // 32)
        assert instance.endswith(",8>") == (tiles8 >= 512 and c["H"] % 8 == 0)
    if c["kind"] == "up":
        assert c["H"] % 4 == 0 and c["W"] % 32 == 0 and (not c["att"] or (c["Cin"] == 64 and c["hk"] in (0, 3) and c["out"]))
    if c["kind"] in ("up", "stem", "attn") and c.get("att"):
        assert 1 <= c["att"]["T"] <= 32


def test_the_cases_cover_what_the_issue_lists():
    conv = [r[3] for r in A._rows(A.CONV)]
    combos = {(c["Cin"], c["Cout"], c["epi"], c["up"]) for c in conv}
    assert len(combos) == 14
    big = [c for c in conv if (c["B"], c["H"], c["W"]) == (64, 32, 64)]
    assert {(c["Cin"], c["Cout"], c["epi"], c["up"]) for c in big} == combos and len(big) == 14
    assert any(c["B"] * (c["H"] // 8) * (c["W"] // 32) == 511 for c in conv)
    small = [c for c in conv if c not in big]
    assert any((c["H"], c["W"]) == (4, 32) for c in small) and any((c["H"], c["W"]) == (8, 64) for c in small) and any(c["B"] == 3 for c in small)
    assert any(c["oco"] == 32 and c["ocp"] == 72 for c in small) and any(c["xcp"] == 72 and c["Cin"] == 64 for c in small)
    assert any(c["xcp"] == 64 and c["Cin"] == 32 for c in small) and any(c["epi"] == "res" and c["rco"] == 8 for c in small)
    assert any(not c["aff"] for c in small)
    stems = [r[3] for r in A._rows(A.STEM)]
    assert {c["C"] for c in stems} == {8, 24, 32, 64} and all(c["H"] == 5 and c["W"] == 40 for c in stems)
    for entry in (A.ATTN, A.STEMATT, A.UPATT):
        atts = [(r[3]["B"], r[3]["att"]) for r in A._rows(entry)]
        assert {1, 7, 32} <= {a["T"] for _b, a in atts} and {"none", "m0", "m1"} <= {a["mask"] for _b, a in atts}
        assert any(b == 3 and a["mask"] == "m0" for b, a in atts) and any(not a["attn"] for _b, a in atts)
    assert any(r[3]["second"] for r in A._rows(A.ATTN)) and any(r[3]["B"] == 257 and r[3]["att"]["mask"] == "m0" for r in A._rows(A.ATTN))
    to3 = [r[3] for r in A._rows(A.TO3, A.TO3MAP)]
    assert {(c["K"], c["act"], c["amap"]) for c in to3} == {(k, a, m) for k in (3, 5) for a, m in ((0, False), (1, False), (1, True), (2, False), (2, True))}
    assert any(c["act"] == 1 and not c["addend"] for c in to3)
    heads = [r[3] for r in A._rows(A.UPHEAD)]
    assert {c["hk"] for c in heads} == {3, 5} and any(not c["out"] for c in heads) and any((c["H"], c["W"]) == (8, 64) for c in heads)
    comb = [r[3] for r in A._rows(A.COMBINE, A.COMBINEMAP)]
    assert {len(c["sizes"]) for c in comb} >= {1, 4} and any(not all(c["low"]) for c in comb) and any(not all(c["high"]) for c in comb)
    assert any(c["low_tanh"] for c in comb) and any(not c["high_tanh"] for c in comb) and any(c["maps"] and not all(c["maps"]) for c in comb)
    tails = [r[3] for r in A._rows(A.TAIL)]
    assert {c["T"] for c in tails} == {1, 32} and any(c["B"] == 17 for c in tails) and {c["nsets"] for c in tails} == {1, 4}
    assert all(c["width"] > c["T"] for c in tails)


# ---- the inputs, the references, the CPU model ----
def _representable(t):
    return torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)


def _model_inside(model, r, e, u, what):
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(e).all()), what
    assert bool(((u * (r.abs() + e) + e > 0) | (r == 0)).all()), what + ": no room where the reference is not an exact zero (a masked word's weight is)"
    q = A.worst(model, r, e, u)
    assert q <= 1.0, "%s: the CPU model is %.3f x the tolerance from the fp64 reference" % (what, q)
    return q


def _moved(other, r, e, u):
    return A.worst(other, r, e, u) > 1.0


def _attention_checks(c, att, h, src, mask, td, u, what):
    """The CPU model of the attention inside the tolerance; the mask variants outside it."""
    T, mode = att["T"], int(att["mask"] == "m1")
    assert _representable(src) and float(src[..., T:].abs().sum()) == 0
    if mask is not None:
        assert mask.shape == (c["B"], T) and bool((~mask).any(1).all()), "a mask row with every word masked is outside the contract"
    cr, ec, Pr, eP = A.attention_ref(h, src, mask, mode, T, u)
    eye = torch.eye(32).reshape(32, 32, 1, 1)
    cm, pm = OL.word_attention(h, src[:, :, :T], eye, mask, td, correct_mask=bool(mode))
    _model_inside(cm, cr, ec, u, what + " c_code")
    _model_inside(pm.reshape(Pr.shape), Pr, eP, 0.0, what + " attn")
    if mask is not None and T > 1:
        flipped = mask.clone()
        flipped[0, 0] = ~flipped[0, 0]                                   # sample 0 keeps every word: word 0 becomes masked
        c2, _e, P2, _e2 = A.attention_ref(h, src, flipped, mode, T, u)
        assert _moved(c2, cr, ec, u) and _moved(P2, Pr, eP, 0.0), what + ": a flipped mask bit stays inside the tolerance"
    if att["mask"] == "m0":
        c2, _e, P2, _e2 = A.attention_ref(h, src, mask, 1, T, u)
        assert _moved(c2, cr, ec, u) and _moved(P2, Pr, eP, 0.0), what + ": mask mode 1 for mode 0 stays inside the tolerance"


@pytest.mark.parametrize("row", A._rows(A.CONV), ids=A.row_id)
def test_conv3x3_case(row):
    c = row[3]
    rows = int(row[1][-2])
    x, w, scale, shift, res = A.conv_inputs(A.ckey(c))
    assert _representable(x) and _representable(w) and (res is None or _representable(res))
    glu, up = c["epi"] == "glu", bool(c["up"])
    r, e = A.conv_refs(A.ckey(c))
    for _name, td, u in TYPES:
        _model_inside(OL.conv_block(x, w, scale, shift, td, glu=glu, upsample=up, residual=res), r, e, u, "conv")
    u = TYPES[1][2]                                                      # the tighter of the two tolerances: f16's
    variants = ["tap"] + (["swap"] if glu else []) + (["phase"] if up else []) + (["halo"] if c["H"] >= rows + 2 else [])
    for v in variants:
        other, _ = A.conv3x3_ref(x, w, scale, shift, res, glu, up, variant=v, rows=rows)
        assert _moved(other, r, e, 2.0 ** -8), "%s stays inside the bf16 tolerance" % v
    if res is not None:
        assert c["rco"] == 8
        at0 = torch.cat([torch.zeros_like(res[:, :8]), res[:, :-8]], 1)    # what offset 0 of the residual's image holds for these channels
        other, _ = A.conv3x3_ref(x, w, scale, shift, at0, glu, up)
        assert _moved(other, r, e, 2.0 ** -8), "the residual read at offset 0 stays inside the tolerance"
    assert u < 2.0 ** -8


@pytest.mark.parametrize("row", A._rows(A.UP, A.UPHEAD, A.UPATT), ids=A.row_id)
def test_upblock_case(row):
    c = row[3]
    x, w, scale, shift, hw = A.up_inputs(c["B"], c["Cin"], c["H"], c["W"], c["hk"], c["aff"])
    assert _representable(x) and (hw is None or _representable(hw))
    assert all(_representable(t) for t in (w, w[:, :, 1] + w[:, :, 2], w[:, :, :, 0] + w[:, :, :, 1], w[:, :, :2, :2].sum((2, 3)), w[:, :, 1:, 1:].sum((2, 3))))
    r, e = A.conv3x3_ref(x, w, scale, shift, None, True, True)
    for _name, td, u in TYPES:
        model = OL.conv_block(x, w, scale, shift, td, glu=True, upsample=True, subpixel=True)
        _model_inside(model, r, e, u, "upBlock")
        if c["hk"]:
            pr, pe = A.tile_partials_ref(model, hw)
            pm = F.conv2d(model.reshape(c["B"], 32, c["H"] // 4, 8, c["W"] // 32, 64).permute(0, 2, 4, 1, 3, 5).reshape(-1, 32, 8, 64), hw, None, 1,
                          2 * (c["hk"] // 2))
            _model_inside(pm.reshape(pr.shape), pr, pe, 0.0, "head_partial")
            hw2 = hw.clone()
            hw2[:, :, 0, c["hk"] - 1] = 0
            assert _moved(A.tile_partials_ref(model, hw2)[0], pr, pe, 0.0), "a dropped tap of the head stays inside the tolerance"
        if c["att"]:
            src, mask = A.attention_inputs(c["B"], c["att"]["T"], c["att"]["mask"], 1)
            _attention_checks(c, c["att"], model, src[1], mask, td, u, "fused attention")
    for v in ("tap", "swap", "phase"):
        assert _moved(A.conv3x3_ref(x, w, scale, shift, None, True, True, variant=v)[0], r, e, 2.0 ** -8), v


@pytest.mark.parametrize("row", A._rows(A.STEM, A.STEMATT), ids=A.row_id)
def test_stem_case(row):
    c = row[3]
    x, w, scale, shift = A.stem_inputs(c["B"], c["C"], c["H"], c["W"])
    r, e = A.stem_ref(x, w, scale, shift)
    for _name, td, u in TYPES:
        model = OL.conv_block(x, w, scale, shift, td, glu=True, round_w=False)
        _model_inside(model, r, e, u, "stem")
        if c["att"]:
            src, mask = A.attention_inputs(c["B"], c["att"]["T"], c["att"]["mask"], 2)
            _attention_checks(c, c["att"], model, src[1], mask, td, u, "fused attention")
    for v in ("tap", "swap"):
        assert _moved(A.stem_ref(x, w, scale, shift, variant=v)[0], r, e, 2.0 ** -8), v


@pytest.mark.parametrize("row", A._rows(A.ATTN), ids=A.row_id)
def test_attention_case(row):
    c = row[3]
    h = A.both(torch.randn(c["B"], 32, c["H"], c["W"], generator=A._gen(c["B"], c["H"], c["W"], 19)))
    src, mask = A.attention_inputs(c["B"], c["att"]["T"], c["att"]["mask"], 3)
    assert _representable(h)
    for _name, td, u in TYPES:
        _attention_checks(c, c["att"], h, src[1], mask, td, u, "attention")
    if c["B"] > 256:
        assert bool((mask[256] != mask[0]).any()), "the row read from global memory must not look like a row the LDS copy holds"


@pytest.mark.parametrize("row", A._rows(A.TO3, A.TO3MAP), ids=A.row_id)
def test_conv_to3_case(row):
    c = row[3]
    x, w, add, m = A.to3_inputs(*A.to3_key(c))
    assert _representable(x) and _representable(w)
    r, e = A.to3_ref(x, w, c["act"], add, A.ALPHA, m)
    y = F.conv2d(x, w, None, 1, c["K"] // 2)                            # the model's head (oracle/tgsr_oracle_lp.py: head()) in fp32
    if c["act"] == A.ACT_TANH:
        y = torch.tanh(y)
    if c["act"] != A.ACT_NONE and add is not None:
        y = y + (m[None, None] if m is not None else A.ALPHA) * add
    _model_inside(y, r, e, 0.0, "conv_to3")
    variants = ["tap"] + (["notanh"] if c["act"] == A.ACT_TANH else []) + (["alpha"] if c["amap"] else [])
    for v in variants:
        assert _moved(A.to3_ref(x, w, c["act"], add, A.ALPHA, m, variant=v)[0], r, e, 0.0), v


@pytest.mark.parametrize("row", A._rows(A.COMBINE, A.COMBINEMAP), ids=A.row_id)
def test_combine_case(row):
    c = row[3]
    ref = A.combine_ref(c)
    inputs = A.combine_inputs(c)
    for k, ((pl, ph, low_in, m), (low, e_low, high, e_high)) in enumerate(zip(inputs, ref)):
        H, W = c["sizes"][k]
        lo = A.fold_partials(pl.float(), H, W).float() if pl is not None else low_in
        if pl is not None and c["low_tanh"]:
            lo = torch.tanh(lo)
        if pl is not None:
            _model_inside(lo, low, e_low, 0.0, "low")
        if ph is not None:
            hi = A.fold_partials(ph.float(), H, W).float()
            hi = torch.tanh(hi) if c["high_tanh"] else hi
            hi = hi + (m[None, None] if m is not None else A.ALPHA) * lo
            _model_inside(hi, high, e_high, 0.0, "high")
    multi = any(H > 8 or W > 64 for H, W in c["sizes"])
    variants = (["partial"] if multi else []) + (["alpha"] if c["maps"] else []) + (["notanh"] if c["high_tanh"] and any(c["high"]) else [])
    for v in variants:
        other = A.combine_ref(c, variant=v)
        moved = False
        for (low, e_low, high, e_high), (l2, _e, h2, _e2) in zip(ref, other):
            moved |= _moved(l2, low, e_low, 0.0) or (high is not None and _moved(h2, high, e_high, 0.0))
        assert moved, v
    assert multi or len(c["sizes"]) == 1


def test_some_combine_case_tells_a_missing_partial():
    assert sum(any(H > 8 or W > 64 for H, W in r[3]["sizes"]) for r in A._rows(A.COMBINE, A.COMBINEMAP)) >= 3


@pytest.mark.parametrize("row", A._rows(A.TAIL), ids=A.row_id)
def test_text_tail_case(row):
    c = row[3]
    _words, _ws, _sent, _caw, _cab, cap = A.tail_inputs(c)
    mask = cap[:, :c["T"]] == 0
    assert bool((~mask).any(1).all()) and bool((cap[:, c["T"]:] != 0).all()) and bool(mask.any()) == (c["T"] > 1)
    if c["T"] == 32:
        assert bool(mask[:, 31].any()), "bit 31 of mbits is in use"
    src = torch.randn(c["nsets"], c["B"], 32, 32)
    for _name, td, _u in TYPES:
        pack = A.att_pack_expected(src, mask, c["T"], td)
        assert pack.numel() * 2 == c["nsets"] * c["B"] * 4096 + 4 * c["B"]
        ii, tt = A.att_frag_index()
        assert int(ii.min()) == 0 and int(ii.max()) == 31 and int(tt.min()) == 0 and int(tt.max()) == 31
        f01 = torch.stack([ii[:2].reshape(-1), tt[:2].reshape(-1)], 1)
        assert len({tuple(v) for v in f01.tolist()}) == 32 * 32, "fragments 0, 1 hold every (channel, word) once"


def test_pack_layouts_hold_every_element_once():
    """The expected packs, built from the header's index formulas, are permutations of the filter (plus the stated zeros)."""
    w = torch.arange(96 * 48 * 9, dtype=torch.float32).reshape(96, 48, 3, 3) + 1
    assert sorted(A.conv3x3_pack_expected(w).tolist()) == sorted(w.reshape(-1).tolist())
    w5 = torch.arange(3 * 32 * 25, dtype=torch.float32).reshape(3, 32, 5, 5) + 1
    p = A.to3_pack_expected(w5)
    assert p.numel() == 5 * 512 and sorted(p[p != 0].tolist()) == sorted(w5.reshape(-1).tolist()) and int((p == 0).sum()) == 5 * 512 - 3 * 32 * 25
    # the sub-pixel pack against the CPU model's own pre-summed taps (oracle/tgsr_oracle_lp.py: subpixel_upconv), phase by phase
    g = torch.Generator().manual_seed(0)
    wu = torch.randn(64, 32, 3, 3, generator=g)
    pk = A.upconv_pack_expected(wu).reshape(2, 2, 8, 2, 64, 8)
    x = torch.randn(1, 32, 4, 4, generator=g)
    want = OL.subpixel_upconv(x, wu, torch.float32)
    taps = torch.zeros(2, 2, 2, 2, 64, 32)                              # [a][b][dys][dxs] -> [co][ci]
    for k16 in range(2):
        for grp in range(2):
            for combo in range(8):
                a, b, dys = combo >> 2, (combo >> 1) & 1, combo & 1
                dxs = (b if grp == 0 else 1 - b)                         # group 0 = the outer column of phase b, 1 = the centre column
                for cb in range(2):
                    for l in range(64):
                        taps[a, b, dys, dxs, cb * 32 + (l & 31), k16 * 16 + 8 * (l >> 5):k16 * 16 + 8 * (l >> 5) + 8] = pk[k16, grp, combo, cb, l]
    got = torch.empty_like(want)
    for a in (0, 1):
        for b in (0, 1):
            k = taps[a, b].permute(2, 3, 0, 1)                           # [co][ci][dys][dxs]
            got[:, :, a::2, b::2] = F.conv2d(F.pad(x, (1 - b, b, 1 - a, a)), k)
    assert torch.equal(got, want)
