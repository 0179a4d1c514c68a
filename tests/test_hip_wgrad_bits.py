"""GPU: the bits of the generator's fp32 weight gradients (csrc/tgsr_conv3x3_wgrad.hip, tgsr_wino_wgrad.hip, tgsr_upwino_wgrad.hip,
tgsr_conv_to3_bwd.hip) on every covered row of tests/test_hip_train_abi.py's instance table: the entry point is called through
ctypes on the row's seeded inputs, placed in the arena as the ABI test places them (the row's alignments and strides), and the
sha256 of dw (and dx for the image heads) equals the recorded one (tests/golden/wgrad_bits.json).  These kernels sum their slabs
in a fixed order and use no atomics: no tolerance.

The digests pin ARITHMETIC, not correctness (tests/test_hip_train_abi.py holds the kernels to fp64): a host-side change - the launch
plan of csrc/tgsr_wgrad_plan.h - must leave them alone, and a pull request that changes a kernel's arithmetic on purpose regenerates
them on an MI355X with `python tests/test_hip_wgrad_bits.py --write`.  Every case re-checks through the exported planners
(tgsr_conv3x3_wgrad_plan, tgsr_conv_to3_bwd_plan) that it still reaches the instance its row names.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import test_hip_train_abi as T  # noqa: E402
from arena import Arena  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "wgrad_bits.json")
pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = T._rows(T.DIRECT, T.WINO, T.UPWINO, T.TO3)


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def wgrad_bits(row, check_plan=True):
    entry, instance, _cond, c = row
    M, L = T._lib()
    a = Arena(DEV)
    gr, xr, xbs = T._place_wgrad(a, entry, c)
    ws, dw = a.place_ws(T.ws_elems(L, entry, c)), a.place_output((c["Cout"], c["Cin"], 3, 3))
    if check_plan:
        plan = T.exported_plan(entry, c, gr.address, xr.address, xbs)
        assert plan["instance"] == instance, "the case reaches %s" % plan["instance"]
    assert T._call_wgrad(L, entry, c, gr, xr, xbs, ws, dw) == M.OK
    torch.cuda.synchronize()
    return _digest(dw.read())


def to3_bits(row, check_plan=True):
    _entry, instance, _cond, c = row
    M, L = T._lib()
    B, Cin, H, W, K, act = (c[k] for k in ("B", "Cin", "H", "W", "K", "act"))
    x, w, add, dy = T.to3_inputs(T._tkey(c))
    if check_plan:
        inst, _slabs = T.exported_to3_plan(c)
        assert inst == instance, "the case reaches %s" % inst
    a = Arena(DEV)
    xbs = (Cin + c["xextra"]) * H * W
    dyr, xr, wr = a.place_input(dy), a.place_input(x, bstride=xbs), a.place_input(w)
    outr = a.place_input(T.to3_refs(T._tkey(c))[0].float()) if act else None       # the forward output, as the forward stores it
    addr = a.place_input(add) if add is not None else None
    dx = a.place_output((B, Cin, H, W), written=c["dx"])
    ws = a.place_ws(L.tgsr_conv_to3_bwd_ws_elems(B, Cin, H, W, K))
    dw = a.place_output((3, Cin, K, K), written=c["dw"])
    rc = L.tgsr_conv_to3_bwd(dyr.ptr, outr.ptr if outr else None, addr.ptr if addr else None, T.ALPHA, xr.ptr, xbs, wr.ptr,
                             B, Cin, H, W, K, M.ACT_TANH_AXPY if act else M.ACT_NONE, dx.ptr if c["dx"] else None,
                             ws.ptr if c["dw"] else None, dw.ptr if c["dw"] else None, T._stream())
    assert rc == M.OK
    torch.cuda.synchronize()
    return _digest(*([dx.read()] if c["dx"] else []) + ([dw.read()] if c["dw"] else []))


def bits(row, check_plan=True):
    return (to3_bits if row[0] == T.TO3 else wgrad_bits)(row, check_plan)


@pytest.fixture(scope="module")
def want():
    assert torch.cuda.is_available()
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("row", ROWS, ids=T.row_id)
def test_weight_gradient_bits(row, want):
    key = T.row_id(row)
    assert key in want, "%s: not in the fixture" % key
    assert bits(row) == want[key], "%s: the output's bits moved" % key


def test_fixture_holds_exactly_these_cases(want):
    keys = [T.row_id(r) for r in ROWS]
    assert len(set(keys)) == len(keys) and sorted(keys) == sorted(want)


if __name__ == "__main__":
    if "--write" in sys.argv:
        # the planners' cross-check is the tests': a fixture can be recorded from a library that does not export them yet
        fx = {T.row_id(r): bits(r, check_plan=False) for r in ROWS}
        assert len(fx) == len(ROWS)
        path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(fx[k])) for k in sorted(fx)) + "\n}\n")
        print("%s: %d digests, %d distinct" % (path, len(fx), len(set(fx.values()))))
