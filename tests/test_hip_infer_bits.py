"""GPU: the bits of the fp32 inference convolutions (csrc/tgsr_conv3x3.hip, tgsr_upconv.hip, tgsr_upwino.hip, tgsr_upwino4.hip,
tgsr_winograd.hip, tgsr_winograd4.hip) on every convolution row of tests/test_hip_infer_abi.py's instance table: the entry point is
called through ctypes on the row's seeded inputs, placed in the arena as the ABI test places them (the row's strides and pads, the
filter packed by its pack kernel), and the sha256 of out (and of stat_partial for the *_stats_fwd rows) equals the recorded one
(tests/golden/infer_bits.json).  These kernels use no atomics and the ABI test asserts that a second call gives the same bits: no
tolerance.

The digests pin ARITHMETIC, not correctness (tests/test_hip_infer_abi.py holds the kernels to fp64): a host-side change - the launch
plan of csrc/tgsr_conv_plan.h - must leave them alone, and a pull request that changes a kernel's arithmetic on purpose regenerates
them on an MI355X with `python tests/test_hip_infer_bits.py --write`.  Every case first checks through the exported planner
(tgsr_conv3x3_form_plan) that it still reaches the instance its row names.
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

import test_hip_infer_abi as T  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "infer_bits.json")
pytestmark = pytest.mark.gpu
ROWS = T._rows(*T.CONVS)


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def bits(row, check_plan=True):
    entry, instance, _cond, c = row
    M, L = T._lib()
    w = T.conv_inputs(T._ckey(c))[1]
    pack = T.run_pack(L, T.PACK_OF[entry], w, c["Cout"], c["Cin"], c["glu"])
    a, r, kw = T.place_conv(L, entry, c, pack)
    if check_plan:
        reached = T.conv_plan(L, entry, c, kw)[0]
        assert reached == instance, "the case reaches %s" % reached
    assert T.call(L, T.fn_of(entry, c), kw) == M.OK
    torch.cuda.synchronize()
    a.check()
    return _digest(*[r["out"].read()] + ([r["stat"].read()] if c["stats"] else []))


@pytest.fixture(scope="module")
def want():
    assert torch.cuda.is_available()
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("row", ROWS, ids=T.row_id)
def test_inference_convolution_bits(row, want):
    key = T.row_id(row)
    assert key in want, "%s: not in the fixture" % key
    assert bits(row) == want[key], "%s: the output's bits moved" % key


def test_fixture_holds_exactly_these_cases(want):
    keys = [T.row_id(r) for r in ROWS]
    assert len(set(keys)) == len(keys) and sorted(keys) == sorted(want)


if __name__ == "__main__":
    if "--write" in sys.argv:
        # the planner's cross-check is the tests': a fixture can be recorded from a library that does not export it yet
        fx = {T.row_id(r): bits(r, check_plan=False) for r in ROWS}
        assert len(fx) == len(ROWS)
        path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(fx[k])) for k in sorted(fx)) + "\n}\n")
        print("%s: %d digests, %d distinct" % (path, len(fx), len(set(fx.values()))))
