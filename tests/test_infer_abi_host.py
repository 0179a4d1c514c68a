"""CPU: what tests/test_hip_infer_abi.py rests on, checked without a GPU.

  * the two host planners (tgsr_conv3x3_fwd_plan, tgsr_conv_to3_plan - plain arithmetic, the functions the launchers call) against
    a restatement of the launchers' comments, over a sweep of shapes, with the codes they return for what the calls refuse;
  * the instance table against those planners and the exported *_stats_nslots: every row's case reaches the instance the row
    names, a ragged case has a short last tile in both directions and, where the row says so, two tile rows and columns; all 22
    instances of conv3x3_mfma_kernel are there, and so is every instance of the other kernels;
  * tolerance discrimination, once per case: the fp64 reference built again with one border input value zeroed (last sample, last
    channel, last row, last column - the value a ragged-tile or stride bug would drop) must differ from the first by MORE than the
    case's tolerance in at least one output element.  A case that fails this is reshaped, never its tolerance widened.
"""
import ctypes

import pytest
import torch

import test_hip_infer_abi as T


def _L():
    from tgsr_amd import _lib
    return _lib.lib()


# ---- the planners against their restatement ----
def direct_plan(B, H, W, Cout, glu, up):
    """tgsr_conv3x3_fwd's tile choice restated: (nob, rows, groups, which pass decided)."""
    unit = 64 if glu else 32
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    cands = []
    for nob in ((2, 1) if Cout % (2 * unit) == 0 else (1,)):
        cands += [(nob, rows) for rows in (16, 8, 4) if rows < 16 or nob * (2 if glu else 1) <= 2]
    tiles = [B * -(-Ho // rows) * -(-Wo // 32) * (Cout // (unit * nob)) for nob, rows in cands]
    pick, how = len(cands) - 1, "neither pass"
    for number, floor in (("first pass", 512), ("second pass", 256)):
        if pick != len(cands) - 1:
            break                                    # (a first pass that lands on the LAST candidate is looked at again by the second)
        hit = [i for i, t in enumerate(tiles) if t >= floor]
        if hit:
            pick, how = hit[0], number
    nob, rows = cands[pick]
    return nob, rows, Cout // (unit * nob), how


def _plan(L, B, H, W, Cout, epi, up):
    nob, rpw, groups = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = L.tgsr_conv3x3_fwd_plan(B, H, W, Cout, epi, up, ctypes.byref(nob), ctypes.byref(rpw), ctypes.byref(groups))
    return rc, nob.value, rpw.value, groups.value


def test_conv3x3_plan_is_the_restated_tile_choice_and_reaches_all_22_instances():
    L = _L()
    seen = set()
    for B in (1, 2, 3, 16):
        for glu in (0, 1):
            for Cout in (64, 128, 192) if glu else (32, 96, 128, 192):
                for up in (0, 1):
                    for H in (1, 3, 4, 5, 9, 16, 17, 61, 128):
                        for W in (4, 17, 33, 64, 449, 481, 1009, 2051):
                            rc, nob, rpw, groups = _plan(L, B, H, W, Cout, glu, up)
                            assert rc == 0 and (nob, 4 * rpw, groups) == direct_plan(B, H, W, Cout, glu, up)[:3], (B, H, W, Cout, glu, up)
                            seen.add((nob, glu, up, rpw))
    want = {(nob, glu, up, r) for nob in (1, 2) for glu in (0, 1) for up in (0, 1) for r in (4, 2, 1)} - {(2, 1, 0, 4), (2, 1, 1, 4)}
    assert seen == want and len(want) == 22


def test_conv3x3_plan_returns_the_code_of_the_call_and_leaves_its_outputs_alone():
    L = _L()
    for args, code in (((0, 4, 4, 64, 0, 0), -1), ((1, 0, 4, 64, 0, 0), -1), ((1, 4, 0, 64, 0, 0), -1), ((1, 4, 4, 0, 0, 0), -1),
                       ((1, 4, 4, 64, 2, 0), -1), ((1, 4, 4, 64, -1, 0), -1), ((1, 4, 4, 48, 0, 0), -2), ((1, 4, 4, 96, 1, 0), -2),
                       ((1, 1 << 14, 1 << 14, 64, 0, 0), -2)):
        assert _plan(L, *args) == (code, -7, -7, -7), args
    assert L.tgsr_conv3x3_fwd_plan(1, 4, 4, 64, 0, 0, None, None, None) == 0          # any output may be NULL


def to3_form(x_addr, xbs, B, Cin, H, W, K, add_addr, out_addr, pipe=True):
    """tgsr_conv_to3_fwd's form choice restated: (form, tile rows); None for an absent addend."""
    def tiles(th):
        return B * -(-W // 64) * -(-H // th)
    if K == 5 and Cin % 16 == 0 and W % 64 == 0 and H % 8 == 0 and tiles(8) >= 512 and xbs % 4 == 0 and x_addr % 16 == 0:
        return 0, 8
    th = 16 if tiles(16) >= 512 else 8 if tiles(8) >= 512 else 4
    vec4 = W % 4 == 0 and xbs % 4 == 0 and x_addr % 16 == 0 and out_addr % 16 == 0 and (add_addr is None or add_addr % 16 == 0)
    if vec4 and Cin * ((3 * K * K + 3) & ~3) * 4 <= 16384 and pipe:
        return 1, th
    return (2 if vec4 else 3), th


def _to3(L, x_addr, xbs, B, Cin, H, W, K, add_addr, out_addr):
    form, th = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = L.tgsr_conv_to3_plan(ctypes.c_void_p(x_addr), xbs, B, Cin, H, W, K, None if add_addr is None else ctypes.c_void_p(add_addr),
                              ctypes.c_void_p(out_addr) if out_addr else None, ctypes.byref(form), ctypes.byref(th))
    return rc, form.value, th.value


def test_conv_to3_plan_is_the_restated_form_choice():
    L = _L()
    base = 1 << 20
    seen = set()
    was = L.tgsr_conv_to3_set_pipe(1)
    try:
        for pipe in (1, 0):
            L.tgsr_conv_to3_set_pipe(pipe)
            for B, Cin, H, W in ((1, 9, 12, 64), (2, 3, 5, 8), (1, 5, 9, 70), (4, 6, 128, 512), (8, 6, 128, 512), (2, 16, 128, 1024),
                                 (2, 16, 124, 1024), (2, 20, 128, 1024), (2, 5, 241, 1021), (1, 160, 4, 8), (3, 16, 128, 704)):
                for K in (3, 5):
                    for sx, so, sa, pad in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, None, 0), (0, 0, 0, 2), (0, 0, 0, 4)):
                        xbs = Cin * H * W + pad
                        add = None if sa is None else base + 4 * sa
                        got = _to3(L, base + 4 * sx, xbs, B, Cin, H, W, K, add, base + 4 * so)
                        assert got == (0,) + to3_form(base + 4 * sx, xbs, B, Cin, H, W, K, add, base + 4 * so, bool(pipe)), (B, Cin, H, W, K)
                        seen.add(got[1:])
    finally:
        L.tgsr_conv_to3_set_pipe(was)
    assert {f for f, _ in seen} == {0, 1, 2, 3} and {t for _, t in seen} == {16, 8, 4}
    for args, code in (((0, 64, 1, 4, 4, 4, 3, None, base), -1), ((base, 64, 0, 4, 4, 4, 3, None, base), -1),
                       ((base, 64, 1, 4, 4, 4, 3, None, 0), -1), ((base, 64, 1, 4, 4, 4, 4, None, base), -2),
                       ((base, 64, 1, 4, 4, 4, 7, None, base), -2), ((base, 1 << 30, 1, 4, 1 << 14, 1 << 14, 3, None, base), -2)):
        assert _to3(L, *args) == (code, -7, -7), args


# ---- the instance table against the planners ----
@pytest.mark.parametrize("row", T._rows(*T.CONVS), ids=T.row_id)
def test_convolution_rows_reach_their_instance(row):
    entry, instance, cond, c = row
    L = _L()
    reached, rows, cols = T.conv_plan(L, entry, c)
    assert reached == instance
    assert T.ragged(c, rows, cols) or not c["multi"]
    co, Ho, Wo = T.conv_dims(c)
    if not c["multi"]:
        assert Ho <= rows or Wo <= cols                       # the row says why: one tile row (or column) is all the threshold leaves
    xbs, obs, rbs = T.conv_strides(c)
    assert xbs > c["Cin"] * c["H"] * c["W"] and obs > co * Ho * Wo and rbs > co * Ho * Wo      # slices of wider buffers
    assert c["B"] in (1, 2, 3) and c["B"] * co * Ho * Wo <= 16e6
    assert 2 * Wo + cols < max(T.GUARD, 4 * Wo + 4096)        # an output row pair plus a tile stays inside the guard band
    if entry == T.DIRECT:
        assert direct_plan(c["B"], c["H"], c["W"], c["Cout"], c["glu"], c["up"])[3] in cond
        assert c["Cin"] in (3, 20) and c["Cout"] in (96, 128, 192)
    elif entry == T.UPCONV:
        assert c["Cin"] in (3, 20)
    else:
        assert c["W"] % 4 == 0 and xbs % 4 == 0 and obs % (4 if T.GROUP[entry] == "f44" else 2) == 0
        assert c["Cin"] % (8 if entry in (T.WIDE, T.UPWINO4) else 4) == 0
    if c["stats"]:
        assert not (c["aff"] or c["res"] or c["glu"]) and T.nslots_of(L, entry, c) > 1
    assert c["Cin"] * c["B"] * c["Cout"] * Ho * Wo * 9 <= 1.2e9, "the fp64 reference of a case stays within about 1e9 multiply-adds"


@pytest.mark.parametrize("row", T._rows(T.TO3), ids=T.row_id)
def test_conv_to3_rows_reach_their_instance(row):
    _entry, instance, _cond, c = row
    L = _L()
    base = 1 << 20                                            # the arena places every operand 16-byte aligned, plus its skew
    sk = c["skew"]
    name, th = T.to3_plan(L, c, base + 4 * sk.get("x", 0), base + 4 * sk.get("addend", 0), base + 4 * sk.get("out", 0))
    assert name == instance
    assert T.ragged(c, th, 64) or not c["multi"]
    if "false" in instance:                                   # the scalar form: why it is not the 16-byte copy form
        assert c["W"] % 4 != 0 or T.to3_xbs(c) % 4 != 0 or any(sk.values())
    assert T.to3_xbs(c) > c["Cin"] * c["H"] * c["W"]


def test_the_table_accounts_for_every_instance():
    inst = [r[1] for r in T.TABLE if r[3] is not None]
    direct = {(nob, glu, up, r): T._D % ("%d,%s,%s,%d" % (nob, T._b(glu), T._b(up), r))
              for nob in (1, 2) for glu in (0, 1) for up in (0, 1) for r in (4, 2, 1)}
    named = [k for k, v in direct.items() if v in inst]
    assert len(named) == 22 and set(direct) - set(named) == {(2, 1, 0, 4), (2, 1, 1, 4)}
    assert any(r[3] is None and "conv3x3_mfma_kernel<2,true,*,4,4>" in r[1] and "not instantiated" in r[2] for r in T.TABLE)
    want = ["upconv_glu_mfma_kernel"]
    want += ["%s<%s>" % (k, g) for k in ("upwino_kernel", "upwino4_kernel") for g in ("true", "false")]
    want += ["wino_conv3x3_kernel<%s>" % k for k in ("true,2,false", "false,2,false", "false,2,true", "true,1,false", "false,1,false",
                                                     "false,1,true")]
    want += ["wino4_conv3x3_kernel<%s>" % k for k in ("false,false", "true,false", "false,true")]
    want += ["wino4w_conv3x3_kernel<%s>" % k for k in ("false,8,false", "true,8,false", "false,8,true", "false,4,false", "true,4,false",
                                                       "false,4,true")]
    want += [T._S % ("%d,%d,false,%d,%d" % (K, act, th, ks)) for K in (3, 5) for act in (0, 1) for th, ks in ((16, 1), (8, 2), (4, 4))]
    want += ["conv_to3_mfma_kernel<5,%d,8,8>" % act for act in (0, 1)]
    assert len(want) == 1 + 2 + 2 + 6 + 3 + 6 + 12 + 2
    for k in want:
        assert k in inst, k
    # both affine settings, a residual, one / two / three samples and several stage counts per group
    for entries in ((T.DIRECT, T.UPCONV), (T.WINO, T.UPWINO), (T.WINO4, T.WIDE, T.UPWINO4)):
        cs = [r[3] for r in T._rows(*entries)]
        assert {c["aff"] for c in cs} == {True, False} and {c["B"] for c in cs} == {1, 2, 3} and any(c["res"] for c in cs)
        assert {c["Cout"] for c in cs} >= {128, 192} and any(c["xpad"] for c in cs) and any(c["opad"] for c in cs)
    assert {c["Cin"] for c in (r[3] for r in T._rows(T.WINO, T.WINO4, T.WIDE, T.UPWINO, T.UPWINO4))} >= {4, 8, 12, 16, 24}
    assert any(c["xpad"] % 2 and c["opad"] % 2 for c in (r[3] for r in T._rows(T.DIRECT)))
    # every refusal list names its entry point's function, and every function of the table has one
    fns = {T.fn_of(r[0], r[3]) for r in T._rows(*T.CONVS)}
    assert fns == set(T.REFUSALS) and all(T.fn_of(T.ENTRY_OF[fn], base) == fn for fn, (base, _) in T.REFUSALS.items())
    assert set(T.PACK_OF.values()) | {n for n in T.PACKS if "dgrad" in n} == set(T.PACKS)


# ---- tolerance discrimination ----
def _corner(t, n):
    """The last sample's last `n` rows and columns (everything an input's last value reaches, with a pixel to spare)."""
    return t[-1:, :, -n:, -n:]


@pytest.mark.parametrize("row", T._rows(*T.CONVS), ids=T.row_id)
def test_convolution_tolerance_tells_a_dropped_border_value(row):
    entry, _instance, _cond, c = row
    x, w, scale, shift, res = T.conv_inputs(T._ckey(c))
    n = min(4, c["H"], c["W"])
    s = 2 if c["up"] else 1
    xc = _corner(x, n).clone()
    rc = _corner(res, s * n) if res is not None else None
    full = T.conv_reference(xc, w, scale, shift, rc, c["glu"], c["up"], torch.float64)
    xc[-1, -1, -1, -1] = 0
    cut = T.conv_reference(xc, w, scale, shift, rc, c["glu"], c["up"], torch.float64)
    keep = s * min(2, n)                                      # outputs whose whole window lies inside the corner
    atol, rtol = T.conv_tol(entry)
    d = (full - cut).abs()[..., -keep:, -keep:]
    assert bool((d > atol + rtol * full.abs()[..., -keep:, -keep:]).any())


@pytest.mark.parametrize("row", T._rows(T.TO3), ids=T.row_id)
def test_conv_to3_tolerance_tells_a_dropped_border_value(row):
    c = row[3]
    x, w, add = T.to3_inputs(T._tkey(c))
    n = min(8, c["H"], c["W"])
    xc = _corner(x, n).clone()
    ac = _corner(add, n) if add is not None else None
    full = T.to3_reference(xc, w, ac, c["act"])
    xc[-1, -1, -1, -1] = 0
    cut = T.to3_reference(xc, w, ac, c["act"])
    keep = min(3, n)
    assert bool(((full - cut).abs() > T.TO3_TOL + T.TO3_TOL * full.abs())[..., -keep:, -keep:].any())
