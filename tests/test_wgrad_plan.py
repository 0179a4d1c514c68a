"""The fp32 weight gradients' host-side plan (csrc/tgsr_wgrad_plan.h) through the library's exported planners.

* `tgsr_conv3x3_wgrad_ws_elems`, `tgsr_wino_wgrad_ws_elems`, `tgsr_upwino_wgrad_ws_elems` and `tgsr_conv_to3_bwd_ws_elems`, pinned to
  what they answered before their arithmetic was gathered into one plan per launch (tests/golden/wgrad_plan.json), over the shapes
  their launchers accept: every case of tests/test_hip_train_abi.py's table, the generator's layers at batch 16 (tools/exp_wgrad.py's
  at 32^2, 64^2 and 128^2, the Cin = 3 stems, upBlock(32, 16), the 3x3 and 5x5 image heads at 64^2 .. 256^2 and one Cin = 64 head at
  batch 64, whose weight gradient takes 8 rows per wave) and the shapes of tests/test_hip_train.py.
* What the launchers refuse is held by contract, not recorded: every `*_ws_elems` answers 0 and the planners answer the
  launcher's status with `ws_elems` 0 - each call in a child process of its own, because a planner that divides before it refuses
  dies of SIGFPE and takes the caller with it.

The planners are host arithmetic: nothing here needs a GPU.  `python tests/test_wgrad_plan.py --write` regenerates the fixture from
the library that is built (a pull request that moves a tile, a split or a predicate on purpose regenerates it and says what moved).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import test_hip_train_abi as T  # noqa: E402
from tgsr_amd import _lib as M  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "wgrad_plan.json")
KNOBS = ("TGSR_WGRAD_TILE", "TGSR_WGRAD_DMA", "TGSR_WGRAD_SPLIT_PCT")

# (B, Cin, Cout, H, W, upsample) of a conv3x3 layer (H, W: pre-upsample)
CONV = [(c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["up"]) for _e, _i, _c, c in T._rows(T.DIRECT, T.WINO, T.UPWINO)] + [
    # tools/exp_wgrad.py: NetG_lowweight / NetG_highweight convolutions and upBlocks at batch 16
    (16, cin, cout, r, r, up) for cin, cout, up in ((64, 128, 0), (64, 64, 0), (32, 64, 0), (32, 32, 0), (64, 64, 1), (32, 64, 1))
    for r in (32, 64, 128)] + [
    # the stems on the 3-channel image; upBlock(32, 16): Cout = 32 stays on the direct kernel
    (16, 3, cout, r, r, 0) for cout in (32, 64, 128) for r in (32, 64, 128)] + [(16, 32, 32, r, r, 1) for r in (32, 64, 128)] + [
    # tests/test_hip_train.py: CASES
    (3, 64, 128, 16, 32, 0), (3, 64, 64, 16, 32, 0), (2, 64, 64, 16, 16, 1), (3, 32, 64, 9, 20, 1), (2, 64, 128, 24, 40, 1),
    (4, 32, 64, 32, 32, 0), (4, 32, 32, 32, 32, 0), (2, 32, 32, 16, 32, 0), (2, 3, 64, 32, 32, 0), (16, 64, 128, 32, 32, 0),
    (2, 32, 64, 13, 20, 0), (1, 64, 64, 5, 40, 0), (3, 32, 32, 11, 24, 0), (2, 64, 32, 8, 40, 0), (2, 32, 32, 12, 20, 1),
    (2, 32, 96, 8, 16, 1),
    # ... test_batch_statistics_in_the_conv_epilogue
    (2, 32, 64, 16, 32, 0), (3, 64, 128, 12, 40, 0), (1, 32, 32, 32, 32, 0), (2, 8, 96, 6, 4, 0)]
# (B, Cin, H, W, K) of an image head
TO3 = [(c["B"], c["Cin"], c["H"], c["W"], c["K"]) for _e, _i, _c, c in T._rows(T.TO3)] + [
    (16, cin, r, r, K) for cin in (16, 32, 64) for r in (64, 128, 256) for K in (3, 5)] + [
    (64, 64, 256, 256, 3), (64, 64, 256, 256, 5),                   # >= 1024 workgroups at 8 rows per wave
    # tests/test_hip_train.py: test_conv_to3_backward
    (2, 32, 32, 64, 3), (2, 32, 32, 64, 5), (3, 32, 19, 70, 5), (1, 32, 64, 64, 3), (2, 20, 16, 16, 5), (2, 64, 41, 48, 3),
    (2, 16, 24, 32, 5), (3, 48, 18, 80, 5), (8, 32, 256, 256, 5), (16, 32, 256, 256, 3)]


def record():
    """{key: ws_elems} of every planner over the shapes its launcher accepts"""
    L, out = M.lib(), {}
    for B, Cin, Cout, H, W, up in dict.fromkeys(CONV):
        shape = "%d,%d,%d,%d,%d" % (B, Cin, Cout, H, W)
        assert Cout % 32 == 0
        out["direct %s up%d" % (shape, up)] = int(L.tgsr_conv3x3_wgrad_ws_elems(B, Cin, Cout, H, W, up))
        if Cin % 32 == 0:
            out["wino " + shape] = int(L.tgsr_wino_wgrad_ws_elems(B, Cin, Cout, H, W))
            if Cout % 64 == 0:
                out["upwino " + shape] = int(L.tgsr_upwino_wgrad_ws_elems(B, Cin, Cout, H, W))
    for B, Cin, H, W, K in dict.fromkeys(TO3):
        out["to3 %d,%d,%d,%d,%d" % (B, Cin, H, W, K)] = int(L.tgsr_conv_to3_bwd_ws_elems(B, Cin, H, W, K))
    return out


def test_planners_answer_as_recorded():
    set_ = [k for k in KNOBS if k in os.environ]
    if set_:
        pytest.skip("%s set in the environment: the fixture holds the defaults' answers" % ", ".join(set_))
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record()
    assert sorted(got) == sorted(want), "the grid and the fixture name different cases"
    assert all(v > 0 for v in got.values())
    bad = ["%s: %s, was %s" % (k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not bad, "%d of %d planner answers moved:\n  %s" % (len(bad), len(got), "\n  ".join(bad[:20]))


# ---- what the launchers refuse: (function, arguments, the status its launcher answers) ----
_ZERO = [(0, 8, 8), (2, 0, 8), (2, 8, 0)]                           # B == 0, H == 0, W == 0
REFUSED = (
    [("tgsr_conv3x3_wgrad_ws_elems", (B, 32, 32, H, W, 0), M.EINVAL) for B, H, W in _ZERO]
    + [(fn, (B, 64, 64, H, W), M.EINVAL) for fn in ("tgsr_wino_wgrad_ws_elems", "tgsr_upwino_wgrad_ws_elems") for B, H, W in _ZERO]
    + [("tgsr_conv_to3_bwd_ws_elems", (B, 32, H, W, 3), M.EINVAL) for B, H, W in _ZERO]
    + [("tgsr_wino_wgrad_ws_elems", (2, Cin, Cout, 8, 8), M.EUNSUPPORTED) for Cin, Cout in ((16, 32), (48, 32), (32, 16), (32, 48))]
    + [("tgsr_upwino_wgrad_ws_elems", (2, Cin, Cout, 8, 8), M.EUNSUPPORTED) for Cin, Cout in ((32, 32), (32, 96), (16, 64))]
    + [("tgsr_conv_to3_bwd_ws_elems", (2, 32, 8, 8, 4), M.EUNSUPPORTED), ("tgsr_conv_to3_bwd_ws_elems", (2, 65, 8, 8, 3), M.EUNSUPPORTED)])

# the child loads the library with bare ctypes (no torch: a tenth of a second): argv[1] = [path, function, ints, planner call or None]
_CHILD = r"""
import ctypes, json, sys
path, name, args, plan = json.loads(sys.argv[1])
L = ctypes.CDLL(path)
f = getattr(L, name)
f.restype = ctypes.c_int64
ws = int(f(*args))
rc, out = None, None
if plan:
    pname, lead, ints, nout, ws_field = plan
    p = getattr(L, pname)
    p.restype = ctypes.c_int
    buf = (ctypes.c_int64 * nout)(*([-7] * nout))
    p.argtypes = [ctypes.c_int] * (1 if lead else 0) + ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] if lead else []) + \
        [ctypes.c_int] * len(ints) + [ctypes.c_void_p]
    rc = p(*(([lead[0], 4096, 4096, lead[1]] if lead else []) + ints + [buf]))
    out = int(buf[ws_field])
print(json.dumps([ws, rc, out]))
"""


def _planner_call(fn, args):
    """The exported planner's call for the same shape: [name, (kind, x_bstride) or None, the int arguments, fields, ws_elems' field]"""
    if fn == "tgsr_conv_to3_bwd_ws_elems":
        return ["tgsr_conv_to3_bwd_plan", None, list(args), M.TO3_BWD_PLAN_FIELDS, M.TO3_BWD_PLAN_WS]
    kind = {"tgsr_conv3x3_wgrad_ws_elems": T.DIRECT, "tgsr_wino_wgrad_ws_elems": T.WINO, "tgsr_upwino_wgrad_ws_elems": T.UPWINO}[fn]
    B, Cin, Cout, H, W = args[:5]
    return ["tgsr_conv3x3_wgrad_plan", [T.WGRAD_KIND[kind], Cin * H * W], [B, Cin, H, W, Cout, 1 if kind == T.UPWINO else 0],
            M.WGRAD_PLAN_FIELDS, M.WGRAD_PLAN_WS]


@pytest.mark.parametrize("fn,args,status", REFUSED, ids=lambda v: v[5:] if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_planners_refuse_what_their_launchers_refuse(fn, args, status):
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps([M.LIB_PATH, fn, list(args), _planner_call(fn, args)])],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "%s%s: the child ended with %d\n%s" % (fn, args, r.returncode, r.stderr[-2000:])
    ws, rc, plan_ws = json.loads(r.stdout)
    assert ws == 0, "%s%s answers %d for a shape its launcher refuses" % (fn, args, ws)
    assert rc == status and plan_ws == 0, "the planner answers status %s, ws_elems %s" % (rc, plan_ws)


if __name__ == "__main__":
    if "--write" in sys.argv:
        assert not [k for k in KNOBS if k in os.environ], "unset %s first" % (KNOBS,)
        fx = record()
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(fx[k])) for k in sorted(fx)) + "\n}\n")
        print("%s: %d cases" % (FIXTURE, len(fx)))
