"""CPU: what tests/test_hip_attention_abi.py rests on, checked without a GPU.

  * the instance table against the host-callable planners (tgsr_word_attention_bwd_chunks, tgsr_damsm_words_bwd_ws_elems) and
    against the launch arithmetic restated in that file: the forward's grid cap and which tile a wave reaches on which trip, the
    backward's blocks_per_wave and which waves are empty;
  * the inputs: every caption length >= 1, the mask rows from 256 on unlike every cached row, and the CPU's own fp32 run of the
    oracle within every elementwise cap (a cap the reference's arithmetic misses at a longer reduction says nothing about a kernel:
    such a case gets a smaller input scale, never a wider cap);
  * tolerance discrimination, once per case: the fp64 reference built again with one change a kernel bug would make - the last pixel
    of the last tile dropped from h / dc, one mask bit of one row flipped, the quirk-mode row index replaced by b (mode-0 cases), one
    caption length off by one (where Tw = 1 leaves no other length: the last region of the last image dropped) - must differ from the
    first by MORE than the case's tolerance in at least one element, or, where the bound is a ratio of mean distances, by more than
    that bound allows.  A case that fails this gets a different shape, never a wider tolerance.
"""
import pytest
import torch

import test_hip_attention_abi as A


def _L():
    from tgsr_amd import _lib
    return _lib.lib()


def _moved(ref, other, tol):
    atol, rtol = tol
    return bool(((ref - other).abs() > atol + rtol * ref.abs()).any())


def _mean_moved(ref64, ref32, other, bound):
    """`other` is further from fp64 than `bound` x the CPU fp32 run is: the ratio assertion would trip on it."""
    return float((other - ref64).abs().mean()) > bound * float((ref32.double() - ref64).abs().mean())


# ---- the table against the planners and the restated launch arithmetic ----
def test_the_table_accounts_for_every_instance_and_path():
    inst = lambda *e: " ".join(r[1] for r in A._rows(*e))               # noqa: E731
    cond = lambda *e: " ".join(r[2] for r in A._rows(*e))               # noqa: E731
    for ni in (1, 2, 4):
        assert A._A % ni in inst(A.WAF, A.PROJ)
    for ni in (1, 2):
        assert A._B % ni in inst(A.WAB)
    for k in ("scalar tail", "float4", "> 64 KB", "not 16-byte aligned", "word_project_mfma_kernel", "capped grid"):
        assert k in inst(A.WAF, A.PROJ)
    assert "GRID" in inst(A.DF) and "PAIRED" in inst(A.FA) and "damsm_pair_bwd_kernel" in inst(A.DB)
    none = [r for r in A.TABLE if r[3] is None]
    assert {r[0] for r in none} == {A.WAF, A.WAB, A.DB} and all("refused" in r[2] for r in none)
    wa = [r[3] for r in A._rows(A.WAF, A.PROJ)]
    assert any(c["hextra"] for c in wa) and any(c["cextra"] for c in wa) and any(not c["attn"] for c in wa)
    assert any(not c["mask"] for c in wa) and {c["mode"] for c in wa if c["mask"]} == {0, 1}
    assert any(c["T"] == 32 for c in wa) and any(c["T"] == 1 for c in wa) and any(c["Q"] < 32 for c in wa)
    assert any(c["cdf"] == A.CDF_MAX for c in wa) and any(c["cdf"] % 4 for c in wa) and any(c["wskew"] for c in wa)
    assert sorted(c["nsets"] for c in wa if c["nsets"]) == [1, 4] and {c["cdf"] for c in wa if c["nsets"]} == {37, 100}
    assert sum(c["B"] > 256 for c in wa) == 2
    wb = [r[3] for r in A._rows(A.WAB)]
    assert any(c["hextra"] for c in wb) and any(c["B"] > 256 for c in wb) and any(not c["mask"] for c in wb)
    assert any(c["T"] == 32 for c in wb) and any(c["T"] == 1 and c["Q"] < 32 for c in wb)
    df = [r[3] for r in A._rows(A.DF)]
    assert {c["ndf"] for c in df} == {32, 96, 256, 512} and any(c["lens"] is None for c in df) and any(not c["att"] for c in df)
    assert any(c["Tw"] == 1 for c in df) and any(c["S"] == 1 for c in df) and any(c["S"] % 32 == 1 for c in df)
    assert any((c["ndf"], c["Tw"], c["S"]) == (512, 32, 320) for c in df)
    assert [(c["B"], c["ndf"], c["Tw"], c["S"]) for c in (r[3] for r in A._rows(A.FA))] == [(2, 32, 1, 1), (3, 160, 9, 65), (1, 512, 32, 320)]
    db = [r[3] for r in A._rows(A.DB)]
    assert [c["ndf"] for c in db] == [32, 96, 160, 256] and [c for c in db if c["ndf"] == 160][0]["lens"] is None
    assert "idle" in cond(A.DB) and "`dok` cuts a wave" in cond(A.DB)


@pytest.mark.parametrize("row", A._rows(A.WAF, A.PROJ), ids=A.row_id)
def test_word_attention_fwd_rows_reach_their_path(row):
    _entry, instance, cond, c = row
    p = A.fwd_plan(c)
    assert p["instance"] in instance and c["idf"] in (32, 64, 128)
    assert c["T"] <= 32 and (c["nsets"] or c["cdf"] <= A.CDF_MAX)
    if "capped grid" in instance:                                       # cap = 4, gx capped from 5, 17 tiles, stride 16
        assert (p["cap"], p["want"], p["gx"], p["ntiles"], p["stride"], p["trips"]) == (4, 5, 4, 17, 16, 2)
        assert p["ragged_on_second_trip"] and c["B"] > 256
    else:
        assert p["gx"] == p["want"] <= p["cap"] and p["trips"] == 1
    if "waves 2 and 3 exit early" in cond:
        assert (p["ntiles"], p["gx"], p["idle"], p["ragged"]) == (2, 1, [2, 3], True)
    if "Q < 32" in cond:
        assert p["ntiles"] == 1 and p["idle"] == [1, 2, 3]
    if "> 64 KB" in instance:
        assert c["cdf"] * 128 > 64 * 1024
    if "scalar tail" in instance:
        assert c["cdf"] % 4 != 0
    if "float4" in instance or "not 16-byte aligned" in instance:
        assert c["cdf"] % 4 == 0 and bool(c["wskew"]) == ("not 16-byte aligned" in instance)
    assert ((c["idf"] + c["hextra"]) * c["Q"] > c["idf"] * c["Q"]) == bool(c["hextra"])


@pytest.mark.parametrize("row", A._rows(A.WAB), ids=A.row_id)
def test_word_attention_bwd_rows_reach_their_path(row):
    _entry, instance, cond, c = row
    nch = _L().tgsr_word_attention_bwd_chunks(c["Q"])
    assert nch == max(1, min(64, -(-c["Q"] // 128)))
    p = A.bwd_plan(c, nch)
    assert p["instance"] == instance and c["idf"] in (32, 64)
    assert 4 * nch * p["bpw"] >= p["nblk"], "every pixel block has a wave"
    if "two chunks" in cond:
        assert (nch, p["bpw"], p["empty"]) == (2, 1, [5, 6, 7])
    if "blocks_per_wave == 2" in cond:                                  # wave 128 holds the ragged block 256 alone, 129 .. 255 are empty
        assert (nch, p["bpw"], p["nblk"]) == (64, 2, 257) and c["Q"] % 32 != 0 and p["empty"] == list(range(129, 256))
    else:
        assert p["bpw"] == 1
    if "Q < 32" in cond:
        assert (nch, p["nblk"], p["empty"]) == (1, 1, [1, 2, 3])


@pytest.mark.parametrize("row", A._rows(A.DF, A.FA, A.DB), ids=A.row_id)
def test_damsm_rows_fit_the_launchers(row):
    entry, _instance, cond, c = row
    B, ndf, Tw, S = c["B"], c["ndf"], c["Tw"], c["S"]
    assert ndf % 32 == 0 and 32 <= ndf <= (256 if entry == A.DB else 512) and 1 <= Tw <= 32 and 1 <= S <= 320
    lds = 4 * (ndf * 32 + 32 * 321 + 4 * 32 * 65 + 96 + 4 * 96)         # damsm_launch
    assert lds <= 160 * 1024 and (("140 KB" in cond) <= (lds > 138 * 1024))
    if entry == A.DB:
        assert _L().tgsr_damsm_words_bwd_ws_elems(B, ndf, S) == A.damsm_ws_elems(c)
        csz = max(2 * ndf * 33, 32 * S)
        assert 4 * (2 * ndf * 32 + csz + 128 + 8 * 128 + 2 * 32 * 32) <= 160 * 1024
        if "`dok` cuts a wave" in cond:
            assert ndf % 64 != 0
    if "three waves without" in cond:
        assert ndf // 32 < 4
    if "one region" in cond:
        assert S % 32 == 1


# ---- the inputs: lengths, mask rows, and the CPU's own fp32 run within every elementwise cap ----
@pytest.mark.parametrize("row", A._rows(A.WAF, A.PROJ), ids=A.row_id)
def test_word_attention_fwd_inputs_and_cpu_fp32_within_the_caps(row):
    c = row[3]
    h, words, ws, mask = A.wa_inputs(c)
    if mask is not None:
        assert bool((~mask).any(1).all())
        if c["B"] > 256:
            assert all(bool((mask[r] != mask[:256]).any(1).all()) for r in range(256, c["B"]))
    ref_c, ref_a, ref_src = A.wa_refs(c)
    c32, a32, s32 = A.wa_reference(c, h, words, ws[-1], mask, torch.float32)
    A.close(c32, ref_c, A.TOL_CCODE, "c_code")
    A.close(a32, ref_a, A.TOL_ATTN, "attn")
    A.close(s32, ref_src, A.TOL_SRC, "src")


@pytest.mark.parametrize("row", A._rows(A.WAB), ids=A.row_id)
def test_word_attention_bwd_cpu_fp32_within_the_cap(row):
    (dh64, _), (dh32, _) = A.wb_refs(row[3])
    A.close(dh32, dh64, A.TOL_DH, "dh")


@pytest.mark.parametrize("row", A._rows(A.DF, A.DB), ids=A.row_id)
def test_damsm_cpu_fp32_within_the_caps(row):
    (sim64, att64, gw64, gc64), (sim32, att32, gw32, gc32) = A.d_refs(row[3])
    A.close(sim32, sim64, A.TOL_SIM, "sim")
    A.close(att32, att64, A.TOL_ATT_DIAG, "att_diag")
    if row[0] == A.DB:
        A.close(gw32, gw64, A.damsm_grad_tol(gw64), "grad_words")
        A.close(gc32, gc64, A.damsm_grad_tol(gc64), "grad_ctx")


@pytest.mark.parametrize("row", A._rows(A.FA), ids=A.row_id)
def test_func_attention_cpu_fp32_within_the_caps(row):
    c = row[3]
    query, ctx, _ = A.d_inputs(c)
    wc64, at64 = A.fa_reference(c, query, ctx)
    wc32, at32 = A.fa_reference(c, query, ctx, torch.float32)
    A.close(wc32, wc64, A.TOL_FA_WC, "weighted_context")
    A.close(at32, at64, A.TOL_FA_ATTN, "attn")


# ---- tolerance discrimination ----
def _flip_one_mask_bit(mask, T):
    m = mask.clone()
    m[-1, T - 1] = ~m[-1, T - 1]                # the last row: with B > 256 one a workgroup reads from global memory
    assert bool((~m).any(1).all())
    return m


@pytest.mark.parametrize("row", A._rows(A.WAF, A.PROJ), ids=A.row_id)
def test_word_attention_fwd_tolerance_discriminates(row):
    c = row[3]
    h, words, ws, mask = A.wa_inputs(c)
    ref_c, ref_a, _ = A.wa_refs(c)
    cut = h.clone()
    cut[-1, :, -1] = 0                           # the last pixel of the last tile
    got_c, got_a, _ = A.wa_reference(c, cut, words, ws[-1], mask)
    if c["T"] > 1:                               # with one word the map is 1 and c_code = src whatever h holds: T = 1 tells nothing here
        assert _moved(ref_c, got_c, A.TOL_CCODE) and _moved(ref_a, got_a, A.TOL_ATTN)
    else:                                        # ... there a wrong word projection is what shows: one weight column dropped
        w = ws[-1].clone()
        w[:, -1] = 0
        assert _moved(ref_c, A.wa_reference(c, h, words, w, mask)[0], A.TOL_CCODE)
    if mask is not None:
        got_c, got_a, _ = A.wa_reference(c, h, words, ws[-1], _flip_one_mask_bit(mask, c["T"]))
        assert _moved(ref_c, got_c, A.TOL_CCODE) and _moved(ref_a, got_a, A.TOL_ATTN)
        if c["mode"] == 0:
            got_c, got_a, _ = A.wa_reference(dict(c, mode=1), h, words, ws[-1], mask)
            assert _moved(ref_c, got_c, A.TOL_CCODE) and _moved(ref_a, got_a, A.TOL_ATTN)


@pytest.mark.parametrize("row", A._rows(A.WAB), ids=A.row_id)
def test_word_attention_bwd_tolerance_discriminates(row):
    c = row[3]
    h, src, dc, mask = A.wb_inputs(c)
    (dh64, ds64), (_dh32, ds32) = A.wb_refs(c)
    cut = dc.clone()
    cut[-1, :, -1] = 0
    dh, ds = A.wb_reference(c, h, src, cut, mask)
    assert _mean_moved(ds64, ds32, ds, A.R_DSRC)
    if c["T"] > 1:                               # T = 1: dh is exactly zero whatever dc holds, and the test asserts exactly that
        assert _moved(dh64, dh, A.TOL_DH)
    else:
        assert float(dh64.abs().max()) == 0.0
    if mask is not None:
        dh, ds = A.wb_reference(c, h, src, dc, _flip_one_mask_bit(mask, c["T"]))
        assert _moved(dh64, dh, A.TOL_DH) and _mean_moved(ds64, ds32, ds, A.R_DSRC)
        if c["mode"] == 0:
            dh, ds = A.wb_reference(dict(c, mode=1), h, src, dc, mask)
            assert _moved(dh64, dh, A.TOL_DH) and _mean_moved(ds64, ds32, ds, A.R_DSRC)


def _other_lens(c):
    lens = A.d_lens(c)
    lens[-1] += 1 if lens[-1] < c["Tw"] else -1
    return lens


@pytest.mark.parametrize("row", A._rows(A.DF, A.DB), ids=A.row_id)
def test_damsm_tolerance_discriminates(row):
    c = row[3]
    words, ctx, gsim = A.d_inputs(c)
    (sim64, att64, gw64, gc64), (_s, _a, gw32, gc32) = A.d_refs(c)
    if c["Tw"] > 1:
        sim, att, gw, gc = A.damsm_reference(c, words, ctx, gsim, lens=_other_lens(c))
    else:
        cut = ctx.clone()
        cut[-1, :, -1] = 0                       # the last region of the last image
        sim, att, gw, gc = A.damsm_reference(c, words, cut, gsim)
    assert _moved(sim64, sim, A.TOL_SIM)
    if row[0] == A.DF and c["att"] and c["Tw"] > 1:         # Tw = 1: softmax over one word is 1, the map 1 / S whatever the inputs hold
        assert _moved(att64, att, A.TOL_ATT_DIAG)
    if row[0] == A.DB:
        assert _moved(gw64, gw, A.damsm_grad_tol(gw64)) and _moved(gc64, gc, A.damsm_grad_tol(gc64))
        assert _mean_moved(gw64, gw32, gw, A.R_GWORDS) and _mean_moved(gc64, gc32, gc, A.R_GCTX)


@pytest.mark.parametrize("row", A._rows(A.FA), ids=A.row_id)
def test_func_attention_tolerance_discriminates(row):
    c = row[3]
    query, ctx, _ = A.d_inputs(c)
    wc64, at64 = A.fa_reference(c, query, ctx)
    cut = ctx.clone()
    cut[-1, :, -1] = 0
    wc, at = A.fa_reference(c, query, cut)
    assert _moved(wc64, wc, A.TOL_FA_WC)
    assert c["S"] == 1 or _moved(at64, at, A.TOL_FA_ATTN)
