"""CPU: what tests/test_hip_infer_abi.py rests on, checked without a GPU.

  * the host planners (plain arithmetic, the functions the launchers call) against a restatement of the launchers as they stood
    before their arithmetic was gathered, over a sweep of shapes, with the codes they return for what the calls refuse:
    tgsr_conv3x3_form_plan - csrc/tgsr_conv_plan.h, the one place the fp32 forward launches are planned - with tgsr_conv3x3_fwd_plan and
    the *_stats_nslots that answer from it, and tgsr_conv_to3_plan; every refusal row of tests/test_hip_infer_abi.py on made-up
    addresses; the answers of the older exports pinned to a fixture (tests/golden/conv_plan.json); and the Python routing
    (ops.FORMS, ops.wino4_wanted, ops.upwino4_wanted, ops.conv3x3_form) tied to the plan it does not call;
  * the instance table against those planners: every row's case reaches the instance the row names, a ragged case has a short last tile in both directions and, where the row says so, two tile rows and columns; all 22
    instances of conv3x3_mfma_kernel are there, and so is every instance of the other kernels;
  * tolerance discrimination, once per case: the fp64 reference built again with one border input value zeroed (last sample, last
    channel, last row, last column - the value a ragged-tile or stride bug would drop) must differ from the first by MORE than the
    case's tolerance in at least one output element.  A case that fails this is reshaped, never its tolerance widened.
"""
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import test_hip_infer_abi as T  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_plan.json")


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
    seen, names = set(), set()
    for B in (1, 2, 3, 16):
        for glu in (0, 1):
            for Cout in (64, 128, 192) if glu else (32, 96, 128, 192):
                for up in (0, 1):
                    for H in (1, 3, 4, 5, 9, 16, 17, 61, 128):
                        for W in (4, 17, 33, 64, 449, 481, 1009, 2051):
                            rc, nob, rpw, groups = _plan(L, B, H, W, Cout, glu, up)
                            assert rc == 0 and (nob, 4 * rpw, groups) == direct_plan(B, H, W, Cout, glu, up)[:3], (B, H, W, Cout, glu, up)
                            seen.add((nob, glu, up, rpw))
                            kw = T.fake_conv(_case("direct", B, 20, H, W, Cout, glu, up=up))       # the same answer in full
                            got = T.form_plan(L, "direct", kw)
                            assert got == restated_plan("direct", kw, 0) and got[1][1:5] == [nob, glu, up, rpw], (B, H, W, Cout, glu, up)
                            names.add(T.instance_of(got[1]))
    want = {(nob, glu, up, r) for nob in (1, 2) for glu in (0, 1) for up in (0, 1) for r in (4, 2, 1)} - {(2, 1, 0, 4), (2, 1, 1, 4)}
    assert seen == want and len(want) == 22
    assert names == {r[1] for r in T._rows(T.DIRECT)} and len(names) == 22


def test_conv3x3_plan_returns_the_code_of_the_call_and_leaves_its_outputs_alone():
    L = _L()
    for args, code in (((0, 4, 4, 64, 0, 0), -1), ((1, 0, 4, 64, 0, 0), -1), ((1, 4, 0, 64, 0, 0), -1), ((1, 4, 4, 0, 0, 0), -1),
                       ((1, 4, 4, 64, 2, 0), -1), ((1, 4, 4, 64, -1, 0), -1), ((1, 4, 4, 48, 0, 0), -2), ((1, 4, 4, 96, 1, 0), -2),
                       ((1, 1 << 14, 1 << 14, 64, 0, 0), -2)):
        assert _plan(L, *args) == (code, -7, -7, -7), args
    assert L.tgsr_conv3x3_fwd_plan(1, 4, 4, 64, 0, 0, None, None, None) == 0          # any output may be NULL


# What the seven launchers checked and computed, restated from their code as it stood before csrc/tgsr_conv_plan.h:
#   Cout % (GLU), Cin %, alignment in bytes of x / out and residual / the pack, log2 of the H W limit, GLU only, takes a residual, has
#   the statistics epilogue, block size
RULES = {"direct": (32, 64, 1, 0, 0, 0, 28, False, True, False), "upconv": (64, 64, 1, 0, 8, 0, 28, True, False, False),
         "upwino": (64, 64, 4, 16, 8, 0, 26, False, False, False), "upwino4": (64, 64, 8, 16, 16, 16, 26, False, False, False),
         "wino": (32, 32, 4, 16, 8, 0, 28, False, True, True), "wino4": (64, 64, 4, 16, 16, 0, 28, False, True, True),
         "wino4w": (64, 64, 8, 16, 16, 16, 28, False, True, True)}
E, U = -1, -2


def _cdiv(a, b):
    return -(-a // b)


def restated_plan(form, kw, stats):
    """(status, the fields of tgsr_conv3x3_form_plan or None) of a call."""
    cout_mod, cout_glu, cin_mod, xa, ioa, pa, bits, gate_only, has_res, has_stats = RULES[form]
    B, Cin, H, W, Cout, epi = (kw[k] for k in ("B", "Cin", "H", "W", "Cout", "epilogue"))
    glu = epi == 1
    if not kw["x"] or not kw["pack"] or not kw["out"] or Cin < 1 or (kw["scale"] is None) != (kw["shift"] is None):
        return E, None
    if kw["res"] and (glu or not has_res):
        return E, None
    if min(B, H, W, Cout) < 1 or epi not in (0, 1) or (gate_only and not glu) or (stats and not has_stats):
        return E, None
    if Cout % (cout_glu if glu else cout_mod) or H * W >= 1 << bits or Cin % cin_mod or Cin * H * W >= 1 << 32:
        return U, None

    def off(addr, stride, n):
        return n and (addr % n or stride % (n // 4))
    if (xa and W % 4) or off(kw["x"], kw["xbs"], xa) or off(kw["out"], kw["obs"], ioa) or off(kw["pack"], 0, pa) or \
            (kw["res"] and off(kw["res"], kw["rbs"], ioa)):
        return U, None
    st = int(bool(stats) and not glu)
    slots = 0
    if form == "direct":
        up = int(kw["upsample"] != 0)
        nob, rows, groups, _how = direct_plan(B, H, W, Cout, glu, up)
        t, th, tw, tx, ty, block = (nob, int(glu), up, rows // 4), rows, 32, _cdiv(W << up, 32), _cdiv(H << up, rows), 256
    elif form == "upconv":
        t, th, tw, tx, ty, groups, block = (), 8, 64, _cdiv(W, 32), _cdiv(H, 4), Cout // 64, 256
    elif form == "upwino":
        t, th, tw, tx, ty, groups, block = (int(glu),), 4, 32, _cdiv(W, 16), _cdiv(H, 2), Cout // 64, 256
    elif form == "upwino4":
        t, th, tw, tx, ty, groups, block = (int(glu),), 4, 64, _cdiv(2 * W, 64), _cdiv(2 * H, 4), Cout // 64, 256
    elif form == "wino":
        nh = 2 if Cout % 64 == 0 else 1
        th = 4 if nh == 2 else 8
        t, tw, tx, ty, groups, block, slots = (int(glu), nh, st), 32, _cdiv(W, 32), _cdiv(H, th), Cout // (32 * nh), 256, th // 2
    elif form == "wino4":
        t, th, tw, tx, ty, groups, block, slots = (int(glu), st), 8, 64, _cdiv(W, 64), _cdiv(H, 8), Cout // 64, 512, 2
    else:
        nb = 8 if Cout % 128 == 0 else 4
        t, th, tw, tx, ty, groups, block, slots = (int(glu), nb, st), 4, 64, _cdiv(W, 64), _cdiv(H, 4), Cout // (16 * nb), 64 * nb, 1
    gx, gy = (B * tx * ty, groups) if form in ("direct", "upconv") else (B * tx * ty * groups, 1)   # the MFMA forms: groups in grid.y
    t = tuple(t) + (0,) * (4 - len(t))
    return 0, [M().CONV_FORMS.index(form), *t, gx, gy, block, tx, ty, th, tw, _cdiv(Cin, 4), groups, B * tx * ty * slots]


def M():
    from tgsr_amd import _lib
    return _lib


def _case(form, B, Cin, H, W, Cout, glu, res=False, aff=True, stats=False, up=0, xpad=0, opad=0):
    up = 1 if form.startswith("up") else up
    return dict(T._c(B, Cin, Cout, H, W, glu=glu, up=up, aff=aff, res=res, stats=stats, xextra=0, oextra=0, rextra=0, xpad=xpad, opad=opad))


SWEEP_HW = ((1, 4), (3, 20), (5, 36), (8, 64), (9, 68), (16, 128), (61, 40), (64, 64))           # ragged and whole tiles of every form
SWEEP_COUT = (32, 48, 64, 96, 128, 192)
SWEEP_CIN = (1, 3, 4, 6, 8, 12, 16)


def sweep():
    """(form, the named arguments of a call, stats) over sizes, channel counts on both sides of every modulus, every epilogue a
    form's entries can ask for, and operands 0, 4 and 8 bytes off their alignment."""
    for form in RULES:
        has_res, has_stats = RULES[form][8], RULES[form][9]
        for B in (1, 2, 3, 5, 16):
            for H, W in SWEEP_HW:
                for Cout in SWEEP_COUT:
                    for Cin in SWEEP_CIN:
                        for glu in (0, 1):
                            for up in ((0, 1) if form == "direct" else (0,)):
                                for stats in ((0, 1) if has_stats and not glu else (0,)):
                                    c = _case(form, B, Cin, H, W, Cout, glu, res=has_res and not glu and not stats and B != 2,
                                              aff=not stats and B != 3, stats=bool(stats), up=up)
                                    yield form, T.fake_conv(c), stats
        # alignments: one operand at a time, and each batch stride
        for H, W, Cout, Cin in ((5, 36, 128, 8), (8, 64, 64, 16)):
            for B in (1, 2):
                base = _case(form, B, Cin, H, W, Cout, 1 if RULES[form][7] else 0, res=has_res)
                for name in ("x", "out", "res", "pack"):
                    for words in (1, 2):
                        yield form, T.fake_conv(base, {name: words}), 0
                for xpad, opad, radd in ((1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2)):
                    kw = T.fake_conv(dict(base, xpad=xpad, opad=opad))
                    kw["rbs"] += radd
                    yield form, kw, 0


def test_form_planner_is_the_restated_launchers_over_the_sweep():
    L = _L()
    seen, refused, n = set(), {E: 0, U: 0}, 0
    for form, kw, stats in sweep():
        rc, plan = T.form_plan(L, form, kw, stats)
        want_rc, want = restated_plan(form, kw, stats)
        n += 1
        assert rc == want_rc, (form, kw, stats, rc)
        if rc:
            refused[rc] += 1
            assert plan == [-7] * M().CONV_PLAN_FIELDS, "a refused plan writes nothing"
            continue
        assert plan == want, (form, kw, stats, plan, want)
        seen.add(T.instance_of(plan))
        if RULES[form][9]:                                       # the *_stats_nslots answer from the same plan
            assert getattr(L, T.ops_forms()[form].nslots)(kw["B"], kw["H"], kw["W"], kw["Cout"]) == plan[M().CONV_PLAN_NSLOTS] > 0
    assert n > 20000 and refused[E] > 1000 and refused[U] > 1000          # (E: the sub-pixel form asked for its plain epilogue)
    inst = {r[1] for r in T._rows(T.UPCONV, T.UPWINO, T.UPWINO4, T.WINO, T.WINO4, T.WIDE)}
    assert inst <= seen and len(inst) == 1 + 2 + 2 + 6 + 3 + 6, sorted(inst - seen)


@pytest.mark.parametrize("fn,rf", [q for q in T._refusal_params() if q.values[1]["tag"] != "null_stat_partial"])
def test_form_planner_refuses_what_the_entry_points_refuse(fn, rf):
    """Every row of tests/test_hip_infer_abi.py's REFUSALS but the entry points' own NULL stat_partial: the planner answers the code
    the table says the call returns, from the operands' addresses alone, and writes none of its outputs."""
    entry = T.ENTRY_OF[fn]
    c = dict(T.REFUSALS[fn][0], xextra=2, oextra=2, rextra=2, **rf["case"])
    kw = T.fake_conv(c, rf["skew"])
    over = dict(rf["kw"])
    kw["rbs"] += over.pop("rbs_add", 0)
    kw.update(over)
    for name in rf["null"]:
        kw[name] = None
    assert fn == T.fn_of(entry, c)
    rc, plan = T.form_plan(_L(), T.FORM_OF[entry], kw, c["stats"])
    assert rc == rf["code"] and plan == [-7] * M().CONV_PLAN_FIELDS
    assert restated_plan(T.FORM_OF[entry], kw, c["stats"])[0] == rf["code"]
    rc, plan = T.form_plan(_L(), T.FORM_OF[entry], T.fake_conv(dict(c, **{k: T.REFUSALS[fn][0][k] for k in rf["case"]})), c["stats"])
    assert rc == 0 and plan[0] >= 0, "the row's base case is accepted"


def test_form_planner_refuses_an_unknown_form_and_takes_a_null_plan():
    L = _L()
    kw = T.fake_conv(T.REFUSALS["tgsr_conv3x3_fwd"][0])
    for form in (-1, len(M().CONV_FORMS), 99):
        assert L.tgsr_conv3x3_form_plan(form, kw["x"], kw["xbs"], 1, 4, 3, 8, kw["pack"], 64, None, None, None, 0, kw["out"], kw["obs"], 0, 0, 0,
                                        None) == E
    assert L.tgsr_conv3x3_form_plan(0, kw["x"], kw["xbs"], 1, 4, 3, 8, kw["pack"], 64, None, None, None, 0, kw["out"], kw["obs"], 0, 0, 0, None) == 0
    # a grid beyond 2^31 - 1 workgroups is refused, not wrapped (the launchers used to wrap it)
    big = T.fake_conv(_case("upwino", 1 << 20, 4, 1 << 9, 1 << 12, 64, 1))
    assert T.form_plan(L, "upwino", big)[0] == U
    # ... and the *_stats_nslots answer 0 wherever the launcher refuses the sizes: an image of 2^28 pixels too (include/tgsr_hip.h)
    for form in ("wino", "wino4", "wino4w"):
        fn = getattr(L, T.ops_forms()[form].nslots)
        assert fn(1, 1 << 14, 1 << 14, 64) == 0 and fn(1, (1 << 14) - 1, 1 << 14, 64) > 0 and fn(1 << 24, 1 << 10, 1 << 10, 64) == 0
        assert T.form_plan(L, form, T.fake_conv(_case(form, 1, 8, 1 << 14, 1 << 14, 64, 0)))[0] == U


class _FakeTensor:
    """What ops.conv3x3_form reads of a tensor: a dense NCHW block at an address."""

    def __init__(self, shape, addr=1 << 24, bstride=None):
        self.shape, self._addr, self._bstride = tuple(shape), addr, bstride

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        B, C, H, W = self.shape
        st = (self._bstride or C * H * W, H * W, W, 1)
        return st if i is None else st[i]

    def data_ptr(self):
        return self._addr


def test_python_routing_is_never_laxer_than_the_plan():
    """Where ops.FORMS[form].shape holds and the operands pass the routing's own alignment predicate (ops._aligned: out / residual at
    FORMS[form].align, x at the 16 bytes ops.conv3x3_form asks for every Winograd form), the planner accepts: Python may be stricter
    than the library, never laxer.  One sample: ops._aligned asks no batch stride and ops._conv3x3 passes the dense one, so the call
    is planned with it.  The packs come from the allocator (16 bytes).  The direct form is what conv3x3_form answers when nothing else
    takes a layer and its shape rule is `True`: it is held here where Cout % 32 (% 64 with GLU) holds - the one refusal that reaches
    the caller as the wrapper's error."""
    from tgsr_amd import ops
    L, n, per_form = _L(), 0, dict.fromkeys(RULES, 0)
    for form, kw, stats in sweep():
        f = ops.FORMS[form]
        B, Cin, Cout, H, W, glu = (kw[k] for k in ("B", "Cin", "Cout", "H", "W", "epilogue"))
        if not f.shape(Cin, Cout, H, W) or (f.gate_only and not glu) or (form == "direct" and Cout % (64 if glu else 32)):
            continue
        s_ = 2 if kw["upsample"] or f.up else 1
        co = Cout // 2 if glu else Cout
        x = _FakeTensor((B, Cin, H, W), kw["x"], kw["xbs"])
        out = _FakeTensor((B, co, s_ * H, s_ * W), kw["out"], kw["obs"])
        res = _FakeTensor((B, co, s_ * H, s_ * W), kw["res"], kw["rbs"]) if kw["res"] else None
        x_need = 16 if form not in ("direct", "upconv") else 0
        if kw["pack"] % 16 or (x_need and not ops._aligned(x, x_need)) or (f.align and not (ops._aligned(out, f.align) and ops._aligned(res, f.align))):
            continue
        if B == 1:
            kw = dict(kw, xbs=Cin * H * W, obs=co * s_ * s_ * H * W, rbs=co * s_ * s_ * H * W if kw["res"] else 0)
        assert T.form_plan(L, form, kw, stats)[0] == 0, (form, kw)
        n += 1
        per_form[form] += 1
    assert n > 8000 and min(per_form.values()) > 100, per_form


def test_python_workgroup_rules_count_the_plans_grid():
    """ops.wino4_wanted, ops.upwino4_wanted and the 32-channel-group rule of ops.conv3x3_form compare a workgroup count with a
    threshold; that count is the plan's grid for every shape the rules admit (moved through ROUTING.min_workgroups: the rule holds at
    the plan's count and fails one above it)."""
    from tgsr_amd import ops
    L, R = _L(), ops.ROUTING
    was = (R.wino4, R.min_workgroups, R.pin_batch, R.min_cin, R.min_pixels, R.upwino4_min_cin)
    n = 0
    try:
        R.wino4, R.pin_batch, R.min_cin, R.min_pixels, R.upwino4_min_cin = True, 0, 0, 0, 0
        for B in (1, 2, 5, 16):
            for H, W in ((64, 64), (64, 128), (128, 128), (136, 192), (256, 256)):
                for cin in (4, 8, 12, 64):
                    for cout in (64, 128, 192):
                        for wanted, form, h, w in ((ops.wino4_wanted, ops._wino4_form(cin), H, W), (ops.upwino4_wanted, "upwino4", H // 2, W // 2)):
                            R.min_workgroups = 1
                            if not wanted(cin, cout, h, w, B):
                                continue                                  # a shape or numerics rule, not the work rule
                            rc, plan = T.form_plan(L, form, T.fake_conv(_case(form, B, cin, h, w, cout, 1)))
                            wgs = plan[M().CONV_PLAN_GRID_X] * plan[M().CONV_PLAN_GRID_Y]
                            assert rc == 0
                            R.min_workgroups = wgs
                            assert wanted(cin, cout, h, w, B)
                            R.min_workgroups = wgs + 1
                            assert not wanted(cin, cout, h, w, B)
                            n += 1
        assert n > 100
        # 32-channel groups (Cout % 64 != 0): F(2x2) from 256 workgroup tiles of 8 x 32 - grid.x / channel groups of the plan
        for B in (1, 3, 16):
            for H, W in ((8, 32), (32, 32), (33, 36), (64, 64), (61, 132), (128, 128)):
                for cout in (32, 96):
                    x = _FakeTensor((B, 8, H, W))
                    rc, plan = T.form_plan(L, "wino", T.fake_conv(_case("wino", B, 8, H, W, cout, 0)))
                    assert rc == 0 and plan[M().CONV_PLAN_GRID_Y] == 1 and plan[M().CONV_PLAN_GRID_X] % plan[M().CONV_PLAN_GROUPS] == 0
                    tiles = plan[M().CONV_PLAN_GRID_X] // plan[M().CONV_PLAN_GROUPS]
                    assert ops.conv3x3_form(x, cout) == ("wino" if tiles >= 256 else "direct"), (B, H, W, cout)
    finally:
        R.wino4, R.min_workgroups, R.pin_batch, R.min_cin, R.min_pixels, R.upwino4_min_cin = was


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


# ---- the answers of the exports that were there before csrc/tgsr_conv_plan.h, pinned ----
GOLD_SHAPES = [(B, H, W) for B in (1, 3, 16) for H, W in ((1, 4), (5, 33), (9, 68), (17, 449), (64, 64), (61, 36), (128, 128), (16, 2051))]
GOLD_COUT = (32, 48, 64, 96, 128, 192)
GOLD_ELEMS = ("tgsr_packed_weight_elems", "tgsr_packed_upconv_weight_elems", "tgsr_packed_upwino_weight_elems",
              "tgsr_packed_upwino4_weight_elems", "tgsr_packed_wino_weight_elems", "tgsr_packed_wino4_weight_elems")
GOLD_NSLOTS = ("tgsr_wino_stats_nslots", "tgsr_wino4_stats_nslots", "tgsr_wino4_wide_stats_nslots")


def record():
    """{call: answer} of tgsr_conv3x3_fwd_plan ([status, nob, rows per wave, groups]; -7 = not written), the three *_stats_nslots and the
    tgsr_packed_*_elems (the two wide packs take tgsr_packed_wino4_weight_elems floats: six functions for seven packs) over accepted
    and refused shapes.  No image of 2^28 pixels or more for the *_stats_nslots: there they answer 0 now, as the launchers refuse."""
    L, out = _L(), {}
    plans = [(B, H, W, Cout, epi, up) for B, H, W in GOLD_SHAPES[::2] for Cout in GOLD_COUT[1:] for epi in (0, 1) for up in (0, 1)]
    plans += [(0, 4, 4, 64, 0, 0), (-1, 4, 4, 64, 0, 0), (1, 0, 4, 64, 0, 0), (1, 4, -3, 64, 0, 0), (1, 4, 4, 0, 0, 0), (1, 4, 4, -32, 0, 0),
              (1, 4, 4, 64, 2, 0), (1, 4, 4, 64, -1, 1), (1, 1 << 14, 1 << 14, 64, 0, 0), (1, 1 << 14, (1 << 14) - 1, 64, 1, 0),
              (2, 1 << 13, 1 << 15, 32, 0, 1), (1, 4, 4, 48, 2, 0)]
    for a in plans:
        out["tgsr_conv3x3_fwd_plan %s" % ",".join(map(str, a))] = list(_plan(L, *a))
    slots = [(B, H, W, Cout) for B, H, W in GOLD_SHAPES for Cout in GOLD_COUT]
    slots += [(0, 8, 8, 64), (2, 0, 8, 64), (2, 8, 0, 64), (2, 8, 8, 0), (-2, 8, 8, 64), (2, 8, 8, -64), (2, 8, 8, 16), (1, 1 << 13, 1 << 14, 64)]
    for fn in GOLD_NSLOTS:
        for a in slots:
            out["%s %s" % (fn, ",".join(map(str, a)))] = int(getattr(L, fn)(*a))
    for fn in GOLD_ELEMS:
        for Cout in GOLD_COUT:
            for Cin in (1, 3, 4, 6, 8, 12, 20, 64):
                a = (Cout, Cin, 3) if fn == "tgsr_packed_weight_elems" else (Cout, Cin)
                out["%s %s" % (fn, ",".join(map(str, a)))] = int(getattr(L, fn)(*a))
    return out


def test_the_older_exports_answer_as_recorded():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record()
    assert sorted(got) == sorted(want), "the grid and the fixture name different cases"
    bad = ["%s: %s, was %s" % (k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not bad, "%d of %d answers moved:\n  %s" % (len(bad), len(got), "\n  ".join(bad[:20]))
    assert sum(1 for k, v in got.items() if "fwd_plan" in k and v[0] == 0) >= 150 and sum(1 for v in got.values() if v == 0) >= 100


if __name__ == "__main__":
    if "--write" in sys.argv:
        fx = record()
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(fx[k])) for k in sorted(fx)) + "\n}\n")
        print("%s: %d cases" % (FIXTURE, len(fx)))
