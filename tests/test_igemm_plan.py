"""The implicit-GEMM family's exported planners (csrc/tgsr_down.hip, csrc/tgsr_igemm.hip), pinned to what they answered before
their arithmetic was gathered into one host-side plan per call (tests/golden/igemm_plan.json):

* the discriminators' 4x4 stride-2 and 3x3 convolutions: `tgsr_conv4x4s2_split_form` / `tgsr_conv3x3_gemm_split_form` and
  `tgsr_conv4x4s2_ws_elems` / `tgsr_conv3x3_gemm_ws_elems` over kind {4, 3} x op {0, 1, 2} x switch {0, 1, 3};
* the Inception trunk's generic taps: `tgsr_gconv_nsplit`, `tgsr_gconv_ws_elems`, `tgsr_gconv_stats_nslots` and
  `tgsr_gconv_stats_slot_pixels` of every layer's forward and data-gradient GEMM, under form {0, 1}, at the default TGSR_GCONV_FILL.

The planners are host arithmetic: nothing here needs a GPU.  `python tests/test_igemm_plan.py --write` regenerates the fixture from
the library that is built (a pull request that moves a tile, a split or a predicate on purpose regenerates it and says what moved).
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "igemm_plan.json")
KNOBS = ("TGSR_GCONV_FILL", "TGSR_GCONV_SPLIT", "TGSR_DCONV_SPLIT")

# (B, Cin, Cout, H, W) of the 4x4 stride-2 convolution
D4 = [
    # test_hip_gan.test_conv4x4s2_fwd_dgrad_wgrad
    (2, 3, 8, 16, 16), (3, 8, 16, 8, 12), (1, 40, 33, 4, 4), (2, 64, 128, 8, 8), (5, 16, 32, 32, 32), (4, 256, 520, 8, 8),
    (16, 3, 64, 64, 64), (3, 130, 200, 6, 10), (3, 3, 64, 6, 10), (2, 1, 8, 8, 8), (1, 4, 16, 12, 260), (2, 6, 10, 8, 8),
    # D_NET64 / 128 / 256 at B = 16, DF_DIM = 64: encode_image_by_16times, then the extra downBlocks
    (16, 64, 128, 32, 32), (16, 128, 256, 16, 16), (16, 256, 512, 8, 8),
    (16, 3, 64, 128, 128), (16, 64, 128, 64, 64), (16, 128, 256, 32, 32), (16, 256, 512, 16, 16), (16, 512, 1024, 8, 8),
    (16, 3, 64, 256, 256), (16, 64, 128, 128, 128), (16, 128, 256, 64, 64), (16, 256, 512, 32, 32), (16, 512, 1024, 16, 16),
    (16, 1024, 2048, 8, 8),
    # test_host_logic.test_split_form_eligibility_is_host_arithmetic
    (32, 64, 128, 128, 128), (1, 40, 33, 4, 4), (2, 8, 8, 7, 8), (1 << 20, 64, 128, 128, 128),
    # tests/test_hip_igemm_bits.py
    (2, 8, 16, 8, 8), (2, 128, 64, 8, 8), (2, 72, 10, 8, 8), (4, 8, 16, 16, 16),
]
# (B, Cin, Cout, H, W) of the 3x3 stride-1 convolution in its GEMM form
D3 = [
    # test_hip_gan.test_conv3x3_gemm_fwd_dgrad_wgrad
    (2, 256, 256, 4, 4), (16, 512, 384, 4, 4), (3, 300, 260, 5, 7), (1, 8, 16, 12, 9), (5, 48, 80, 4, 8), (2, 768, 512, 4, 4),
    # the discriminators' reduce blocks and jointConv (8 ndf + 256 sentence channels) at B = 16, DF_DIM = 64
    (16, 1024, 512, 4, 4), (16, 2048, 1024, 4, 4), (16, 768, 512, 4, 4),
    # test_split_form_eligibility_is_host_arithmetic, tests/test_hip_igemm_bits.py
    (1, 48, 80, 4, 8),
]
# (B, Cin, H, W, Cout, kh, kw, stride, ph, pw) of a generic-tap layer
GC = [
    # test_hip_inception.GEOM = test_hip_inception_train.GEOM
    (2, 3, 39, 39, 32, 3, 3, 2, 0, 0), (2, 32, 19, 19, 32, 3, 3, 1, 0, 0), (2, 32, 17, 17, 64, 3, 3, 1, 1, 1),
    (3, 64, 9, 9, 80, 1, 1, 1, 0, 0), (2, 48, 12, 12, 64, 5, 5, 1, 2, 2), (2, 128, 17, 17, 128, 1, 7, 1, 0, 3),
    (2, 128, 17, 17, 192, 7, 1, 1, 3, 0), (2, 192, 17, 17, 320, 3, 3, 2, 0, 0), (4, 384, 8, 8, 384, 1, 3, 1, 0, 1),
    (4, 448, 8, 8, 384, 3, 3, 1, 1, 1), (4, 1280, 8, 8, 320, 1, 1, 1, 0, 0), (1, 5, 7, 11, 7, 3, 1, 1, 1, 0),
    (2, 288, 35, 35, 384, 3, 3, 2, 0, 0), (2, 96, 35, 35, 96, 3, 3, 2, 0, 0), (1, 3, 299, 299, 32, 3, 3, 2, 0, 0),
    (2, 192, 35, 35, 48, 1, 1, 1, 0, 0),
    # test_hip_inception_train.test_new_operators_opcheck
    (2, 32, 9, 9, 48, 3, 3, 1, 1, 1),
    # tests/test_hip_igemm_bits.py
    (2, 16, 8, 8, 32, 3, 3, 1, 1, 1), (2, 32, 9, 9, 96, 3, 3, 2, 0, 0), (2, 16, 8, 8, 32, 1, 7, 1, 0, 3),
    (2, 16, 8, 8, 32, 7, 1, 1, 3, 0), (2, 3, 17, 17, 32, 3, 3, 2, 0, 0), (2, 4, 10, 10, 16, 6, 6, 1, 0, 0),
    (2, 80, 8, 8, 32, 3, 3, 1, 1, 1),
]


def _uniq(rows):
    return list(dict.fromkeys(rows))


def record():
    """{key: answers} of every planner over the grid; every switch is put back."""
    from tgsr_amd import _lib
    L = _lib.lib()
    out = {}
    was = L.tgsr_dconv_set_split(1)
    try:
        for sw in (0, 1, 3):
            L.tgsr_dconv_set_split(sw)
            for kind, shapes, form, ws in ((4, D4, L.tgsr_conv4x4s2_split_form, L.tgsr_conv4x4s2_ws_elems),
                                           (3, D3, L.tgsr_conv3x3_gemm_split_form, L.tgsr_conv3x3_gemm_ws_elems)):
                for B, Cin, Cout, H, W in _uniq(shapes):
                    for op in (0, 1, 2):
                        out["d%d sw%d op%d %d,%d,%d,%d,%d" % (kind, sw, op, B, Cin, Cout, H, W)] = \
                            [int(form(op, B, Cin, H, W, Cout)), int(ws(op, B, Cin, H, W, Cout))]
    finally:
        L.tgsr_dconv_set_split(was)
    was = L.tgsr_gconv_set_form(1)
    try:
        for gf in (0, 1):
            L.tgsr_gconv_set_form(gf)
            for B, Cin, H, W, Cout, kh, kw, st, ph, pw in _uniq(GC):
                OH, OW = (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1
                Kf, Kd = Cin * kh * kw, Cout * kh * kw
                out["g form%d %s" % (gf, ",".join(map(str, (B, Cin, H, W, Cout, kh, kw, st, ph, pw))))] = [
                    # forward GEMM: slabs, workspace, statistics slots, pixels per slot
                    int(L.tgsr_gconv_nsplit(Cout, B * OH * OW, Kf)), int(L.tgsr_gconv_ws_elems(B, Cout, OH, OW, Kf)),
                    int(L.tgsr_gconv_stats_nslots(B, Cout, OH, OW, Kf)), int(L.tgsr_gconv_stats_slot_pixels(B, Cout, OH, OW, Kf)),
                    # data-gradient GEMM: slabs, workspace
                    int(L.tgsr_gconv_nsplit(Cin, B * H * W, Kd)), int(L.tgsr_gconv_ws_elems(B, Cin, H, W, Kd))]
    finally:
        L.tgsr_gconv_set_form(was)
    return out


def test_planners_answer_as_recorded():
    set_ = [k for k in KNOBS if k in os.environ]
    if set_:
        pytest.skip("%s set in the environment: the fixture holds the defaults' answers" % ", ".join(set_))
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record()
    assert sorted(got) == sorted(want), "the grid and the fixture name different cases"
    bad = ["%s: %s, was %s" % (k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not bad, "%d of %d planner answers moved:\n  %s" % (len(bad), len(got), "\n  ".join(bad[:20]))


def test_switches_are_restored():
    from tgsr_amd import _lib
    L = _lib.lib()
    before = (L.tgsr_dconv_set_split(1), L.tgsr_gconv_set_form(1))
    L.tgsr_dconv_set_split(before[0])
    L.tgsr_gconv_set_form(before[1])
    record()
    after = (L.tgsr_dconv_set_split(before[0]), L.tgsr_gconv_set_form(before[1]))
    assert after == before


if __name__ == "__main__":
    if "--write" in sys.argv:
        assert not [k for k in KNOBS if k in os.environ], "unset %s first" % (KNOBS,)
        fx = record()
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(fx[k], separators=(",", ":"))) for k in sorted(fx)) + "\n}\n")
        print("%s: %d cases" % (FIXTURE, len(fx)))
