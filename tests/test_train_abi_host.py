"""CPU: what tests/test_hip_train_abi.py rests on, checked without a GPU.

  * the arena's own arithmetic (tests/arena.py on a CPU buffer): offsets, alignment, gaps, and that check() trips on a written
    guard word, a written gap word, a written input and an unwritten output word;
  * the instance table against the library's own planners (*_ws_elems, tgsr_conv3x3_wgrad_plan, tgsr_conv_to3_bwd_plan and
    tgsr_bn_train_nsplit are host functions): every row's case reaches the instance the row names, the exported plan equals the
    restated one, and the `multi` cases have 1 < nslots < units;
  * tolerance discrimination, once per case: the fp64 reference gradient, built again with one border pixel (last row, last
    column - the pixel a ragged-tile bug would drop) of one sample's grad_out zeroed, must differ from the first by MORE than the
    test's tolerance in at least one element.  A tolerance that cannot tell a dropped pixel from rounding hides failures; a case
    that fails this is to be shrunk, never its tolerance widened.
"""
import pytest
import torch

import test_hip_train_abi as T
from arena import GUARD, PATTERN, Arena


# ---- the arena ----
def _arena():
    a = Arena("cpu")
    x = a.place_input(torch.arange(24, dtype=torch.float32).view(2, 3, 4), bstride=20)
    y = a.place_input(torch.ones(5), skew=1)
    ws = a.place_ws(7)
    out = a.place_output((2, 6), bstride=10)
    run = a.place_inout(torch.tensor([1.0, 2.0]))
    nbt = a.place_inout(torch.tensor([41], dtype=torch.int64), align=8)
    gone = a.place_output((3,), written=False)
    return a, x, y, ws, out, run, nbt, gone


def _write_outputs(a, out, run, nbt):
    buf = a.buffer().view(torch.float32)
    for lo, hi in out.slices() + run.slices():
        buf[lo:hi] = 0.5
    a.buffer()[nbt.offset] = 42


def test_arena_offsets_alignment_and_gaps():
    a, x, y, ws, out, run, nbt, gone = _arena()
    regs = [x, y, ws, out, run, nbt, gone]
    assert x.offset >= GUARD and x.span == 20 + 12 and x.slices() == [(x.offset, x.offset + 12), (x.offset + 20, x.offset + 32)]
    for r, nxt in zip(regs, regs[1:]):
        assert nxt.offset - (r.offset + r.span) >= GUARD            # a guard band between any two operands ...
    assert a.buffer().numel() - (gone.offset + gone.span) >= GUARD  # ... and behind the last
    for r in (x, ws, out, run, gone):
        assert r.address % 16 == 0
    assert y.address % 16 == 4 and nbt.address % 8 == 0
    assert ws.span == 7 and out.span == 16
    buf = a.buffer()
    assert torch.equal(x.read(), torch.arange(24, dtype=torch.float32).view(2, 3, 4))
    assert bool((buf[x.offset + 12:x.offset + 20] == PATTERN).all())                  # the gap between the samples
    assert bool((buf[x.offset - GUARD:x.offset] == PATTERN).all()) and bool((buf[:GUARD] == PATTERN).all())
    assert bool((out.words() == PATTERN).all()) and bool((ws.words() == PATTERN).all())
    assert torch.isnan(buf.view(torch.float32)[0]) and PATTERN != 0x7FC00000
    assert int(nbt.read()) == 41 and run.read().tolist() == [1.0, 2.0]


def test_arena_check_passes_a_clean_call_and_trips_on_every_violation():
    a, x, y, ws, out, run, nbt, gone = _arena()
    assert any("never written" in v for v in a.violations())        # nothing written yet: the outputs are unwritten
    _write_outputs(a, out, run, nbt)
    a.check()
    assert int(nbt.read()) == 42
    a.buffer()[ws.offset:ws.offset + 7] = 0                          # a workspace may be written ...
    a.check()
    for word, what in ((ws.offset + 7, "past the end of ws"), (ws.offset - 1, "before ws"), (out.offset + 6, "the gap"),
                       (x.offset + 3, "input"), (x.offset + 13, "the gap"), (gone.offset + 1, "absent"), (5, "before input")):
        keep = int(a.buffer()[word])
        a.buffer()[word] = 0
        v = a.violations()
        assert len(v) == 1 and "were written" in v[0] and what in v[0], (word, what, v)
        with pytest.raises(AssertionError):
            a.check()
        a.buffer()[word] = keep
        a.check()
    a.buffer()[out.offset + 10 + 5] = PATTERN                        # the last word of the second sample left unwritten
    assert any("1 of 12 words never written" in v for v in a.violations())
    a.buffer().view(torch.float32)[out.offset + 10 + 5] = float("inf")
    assert any("non-finite" in v for v in a.violations())
    a.rearm(ws_fill=0.75)                                            # back to the state before the call, the workspace finite
    assert bool((out.words() == PATTERN).all()) and ws.read().tolist() == [0.75] * 7 and int(nbt.read()) == 41
    assert bool((a.buffer()[ws.offset + 7:ws.offset + 7 + GUARD] == PATTERN).all())


def test_arena_byte_operands_are_padded_to_whole_words_with_the_pattern():
    """A uint8 input (a mask): dense bytes, padded to whole words with PATTERN's bytes, read back as bytes; a write into the
    operand or into its padding trips check()."""
    pat = torch.tensor([PATTERN], dtype=torch.int32).view(torch.uint8).tolist()
    for shape in ((3, 7), (2, 4), (1, 1), (257, 3)):
        n = shape[0] * shape[1]
        m = (torch.arange(n) % 3 == 0).to(torch.uint8).view(shape)
        a = Arena("cpu")
        x = a.place_input(torch.ones(5))
        r = a.place_input(m)
        s = a.place_input(m, skew=1)
        out = a.place_output((3,))
        assert r.per == r.span == (n + 3) // 4 and r.shape == shape and r.address % 16 == 0 and s.address % 16 == 4
        assert r.offset - (x.offset + x.span) >= GUARD and out.offset - (s.offset + s.span) >= GUARD
        assert torch.equal(r.read(), m) and r.read().dtype == torch.uint8 and torch.equal(s.read(), m)
        raw = a.buffer()[r.offset:r.offset + r.per].view(torch.uint8)
        assert raw[:n].tolist() == m.view(-1).tolist()
        assert raw[n:].tolist() == pat[n % 4:] if n % 4 else raw.numel() == n      # the padding bytes hold the pattern's
        assert bool((a.buffer()[r.offset - GUARD:r.offset] == PATTERN).all())
        a.buffer().view(torch.float32)[out.offset:out.offset + 3] = 0.5
        a.check()
        for byte in sorted({0, n - 1, 4 * r.per - 1}):                            # first, last and (where there is one) a padding byte
            view = a.buffer()[r.offset:r.offset + r.per].view(torch.uint8)
            keep = int(view[byte])
            view[byte] = keep ^ 1
            v = a.violations()
            assert len(v) == 1 and "were written" in v[0] and "input" in v[0], (shape, byte, v)
            view[byte] = keep
            a.check()
    with pytest.raises(AssertionError):
        Arena("cpu").place_input(torch.zeros(2, 3, dtype=torch.uint8), bstride=8)


# ---- the instance table against the library's planners ----
def _L():
    from tgsr_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("row", T._rows(T.DIRECT, T.WINO, T.UPWINO), ids=T.row_id)
def test_weight_gradient_rows_reach_their_instance(row):
    entry, instance, _cond, c = row
    xbs = (c["Cin"] + c["xextra"]) * c["H"] * c["W"] + c["xpad"]
    plan = T.plan_of(entry, c, 0, 0, xbs)                            # the arena places both operands 16-byte aligned
    assert plan["instance"] == instance
    n = T.ws_elems(_L(), entry, c)
    assert n == plan["nslots"] * plan["slab"]
    if c["multi"]:
        assert 1 < n // plan["slab"] < plan["units"]
    x, dy = T.wgrad_inputs(T._wkey(c))
    assert x.shape[1] * dy.numel() * 9 <= 2e9, "the fp64 reference of a case stays within about 2e9 multiply-adds"


@pytest.mark.parametrize("row", T._rows(T.DIRECT, T.WINO, T.UPWINO), ids=T.row_id)
def test_the_exported_planner_names_what_the_restated_plan_names(row):
    """tgsr_conv3x3_wgrad_plan - the function the launcher plans with - against plan_of: instance, units, units per workgroup, nslots
    and slab; the Winograd rows at operand addresses 0, 4 and 8 bytes off 16-byte alignment, both sides of the DMA predicate."""
    entry, instance, _cond, c = row
    xbs = (c["Cin"] + c["xextra"]) * c["H"] * c["W"] + c["xpad"]
    assert T.exported_plan(entry, c, 4096, 4096, xbs) == T.plan_of(entry, c, 4096, 4096, xbs)
    assert T.exported_plan(entry, c, 4096, 4096, xbs)["instance"] == instance
    if entry == T.WINO:
        seen = set()
        for g_off in (0, 4, 8):
            for x_off in (0, 4, 8):
                got = T.exported_plan(entry, c, 4096 + g_off, 4096 + x_off, xbs)
                assert got == T.plan_of(entry, c, 4096 + g_off, 4096 + x_off, xbs), (g_off, x_off)
                assert ("dma" not in got["instance"]) or (g_off, x_off) == (0, 0)
                seen.add(got["instance"])
        if "dma" in instance:
            assert len(seen) == 2 and T.exported_plan(entry, c, 4096, 4096, xbs + 2)["instance"] in seen - {instance}


def test_the_table_accounts_for_every_instance():
    inst = " ".join(r[1] for r in T.TABLE if r[3] is not None)
    for ncob in (4, 2, 1):
        for ncib in (2, 1):
            for up in ("false", "true"):
                assert "conv3x3_wgrad_kernel<%d,%d,%s>" % (ncob, ncib, up) in inst
    for k in ("wino_wgrad_kernel<1,1>", "wino_wgrad_kernel<1,2>", "wino_wgrad_kernel<2,1>", "wino_wgrad_kernel<2,2>",
              "wino_wgrad_dma_kernel<1>", "wino_wgrad_dma_kernel<2>", "upwino_wgrad_kernel<1>", "upwino_wgrad_kernel<2>"):
        assert k in inst
    for K in (3, 5):
        for th in ("false", "true"):
            assert "conv_to3_dgrad_kernel<%d,%s>" % (K, th) in inst and "conv_to3_wgrad_kernel<%d,%s>" % (K, th) in inst
            for ncg in (1, 2, 3, 4):
                assert "conv_to3_wgrad_mfma_kernel<%d,%s,%d>" % (K, th, ncg) in inst
    knobs = " ".join(r[2] for r in T.TABLE if r[3] is None)
    for knob in ("TGSR_WGRAD_TILE", "TGSR_WGRAD_DMA", "TGSR_WGRAD_SPLIT_PCT", "TGSR_BN_FUSE_SMALL"):
        assert knob in knobs and "not covered" in knobs
    # every stride parameter takes a non-dense value somewhere; B = 1, Cin = 20 and a `multi` case per weight-gradient entry point
    for entry in (T.DIRECT, T.WINO, T.UPWINO):
        cs = [r[3] for r in T._rows(entry)]
        assert any(c["xextra"] for c in cs) and any(c["B"] == 1 for c in cs) and any(c["multi"] for c in cs)
        assert any(c["H"] % 2 == 1 and c["W"] % 8 != 0 for c in cs)
    assert any(c["Cin"] == 20 for c in (r[3] for r in T._rows(T.DIRECT)))
    to3 = [r[3] for r in T._rows(T.TO3)]
    assert any(c["xextra"] for c in to3) and any(not c["dx"] for c in to3) and any(not c["dw"] for c in to3)
    bn = [r[3] for r in T._rows(T.BNF)] + [c for _, c in T.FROM_STATS]
    assert any(c["oextra"] for c in bn) and any(c["rextra"] and c["res"] for c in bn)
    assert {c["act"] for c in bn} == {0, 1, 2} and {c["run"] for c in bn} == {True, False} == {c["nbt"] for c in bn}
    assert [n for n, _ in T.FROM_STATS] == [1, 3, 96]


@pytest.mark.parametrize("row", T._rows(T.TO3), ids=T.row_id)
def test_conv_to3_rows_reach_their_instance(row):
    _entry, instance, _cond, c = row
    inst, slabs = T.to3_plan(c)
    assert inst == instance
    assert _L().tgsr_conv_to3_bwd_ws_elems(c["B"], c["Cin"], c["H"], c["W"], c["K"]) == slabs * 3 * c["Cin"] * c["K"] ** 2
    assert T.exported_to3_plan(c) == (inst, slabs)                   # tgsr_conv_to3_bwd_plan: the function the launcher plans with


@pytest.mark.parametrize("row", T._rows(T.BNF), ids=T.row_id)
def test_batchnorm_rows_take_the_form_they_name(row):
    _entry, _instance, cond, c = row
    nsplit = _L().tgsr_bn_train_nsplit(c["B"], c["C"], c["H"] * c["W"])
    assert ("nsplit == %d" % nsplit) in cond
    assert (c["H"] * c["W"]) % 4 == 0


# ---- tolerance discrimination ----
def _discriminates(full, dropped, atol, rtol):
    return bool(((full - dropped).abs() > atol + rtol * full.abs()).any())


@pytest.mark.parametrize("row", T._rows(T.DIRECT, T.WINO, T.UPWINO), ids=T.row_id)
def test_weight_gradient_tolerance_tells_a_dropped_border_pixel(row):
    c = row[3]
    x, dy = T.wgrad_inputs(T._wkey(c))
    ref, _ = T.wgrad_refs(T._wkey(c))
    cut = dy.clone()
    cut[-1, :, -1, -1] = 0
    atol, rtol = T.wgrad_tol(dy)
    assert _discriminates(ref, T.wgrad_reference(x, cut, c["up"], torch.float64), atol, rtol)


@pytest.mark.parametrize("row", [r for r in T._rows(T.TO3) if r[3]["dw"]], ids=T.row_id)
def test_conv_to3_tolerance_tells_a_dropped_border_pixel(row):
    c = row[3]
    x, w, add, dy = T.to3_inputs(T._tkey(c))
    _out, _dx, ref = T.to3_refs(T._tkey(c))
    cut = dy.clone()
    cut[-1, :, -1, -1] = 0
    atol, rtol = T.to3_tol(c)
    assert _discriminates(ref, T.to3_reference(x, w, add, cut, c["act"])[2], atol, rtol)


@pytest.mark.parametrize("row", T._rows(T.BNF), ids=T.row_id)
def test_batchnorm_tolerance_tells_a_dropped_border_pixel(row):
    c = row[3]
    i, ref = T.bn_inputs(T._bkey(c)), T.bn_refs(T._bkey(c))
    cut = i["dout"].clone()
    cut[-1, :, -1, -1] = 0
    got = T.bn_reference(i, c["act"], dout=cut)
    atol, rtol = T.bn_affine_tol(i["dout"])
    assert _discriminates(ref["dgamma"], got["dgamma"], atol, rtol) or _discriminates(ref["dbeta"], got["dbeta"], atol, rtol)
    assert _discriminates(ref["draw"], got["draw"], T.OUT_ATOL, 1e-4)
