"""GPU: the bits of the implicit-GEMM family (csrc/tgsr_down.hip, csrc/tgsr_igemm.hip) - the discriminators' 4x4 stride-2 and 3x3
convolutions and the Inception trunk's generic taps - on one small case per kernel instance and launch path (WIDE and 128-row tile,
one slab and a K split, three-piece bf16 form, pre-split A images, fp32 MFMA, the image data-gradient kernels, the statistics form
and its finish).  These kernels are deterministic (slabs summed in a fixed order, no atomics), so the sha256 of the output bytes
equals the recorded one (tests/golden/igemm_bits.json): no tolerance.

The digests pin ARITHMETIC, not correctness (tests/test_hip_gan.py and tests/test_hip_inception*.py hold the kernels to torch): a
host-side change must leave them alone, and a pull request that changes a kernel's arithmetic on purpose regenerates them on an
MI355X with `python tests/test_hip_igemm_bits.py --write`.  Every case re-checks through the exported planners that it still reaches
the instance it names.
"""
import hashlib
import json
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "igemm_bits.json")
pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---- the discriminators: (kind, (B, Cin, Cout, H, W), leaky, ops, {op: (split form under switch 1, slabs)})
DCASES = [
    (4, (2, 3, 8, 16, 16), True, "fdw", {"f": (1, 1), "d": (0, 1), "w": (1, 1)}),   # WIDE forward, one slab, epilogue activation; image dgrad
    (4, (2, 64, 128, 8, 8), True, "fw", {"f": (1, 8), "w": (1, 1)}),      # 128-tile forward, 8 slabs, activation in the slab sum; 16 px / image
    (4, (2, 8, 16, 8, 8), False, "d", {"d": (1, 1)}),                     # WIDE data gradient, four parity classes
    (4, (2, 128, 64, 8, 8), False, "d", {"d": (1, 2)}),                   # 128-tile data gradient, 2 slabs
    (4, (2, 72, 10, 8, 8), False, "d", {"d": (0, 1)}),                    # 4 Cout = 40: a partial chunk, fp32 MFMA under every switch
    (4, (4, 8, 16, 16, 16), False, "w", {"w": (1, 2)}),                   # K = 256 pixels, 2 slabs
    (4, (3, 8, 16, 8, 12), False, "w", {"w": (0, 1)}),                    # 24 pixels per image: fp32
    (3, (1, 48, 80, 4, 8), False, "fdw", {"f": (1, 4), "d": (1, 6), "w": (1, 1)}),  # the split form with a K split
    (3, (1, 8, 16, 12, 9), False, "fdw", {"f": (0, 1), "d": (1, 2), "w": (0, 1)}),  # forward / weight gradient fp32, data gradient split
]
OPS = {"f": 0, "d": 1, "w": 2}

# ---- generic taps: (name, mode, (B, Cin, H, W, Cout, kh, kw, st, ph, pw), flags, (form under gconv_set_form(1), WIDE, slabs))
# mode f: forward (flags: b = bias + relu, s = channel slices of wider tensors); d: data gradient (m = mask, a = accumulate); s: stats
L1, L2 = (2, 16, 8, 8, 32, 3, 3, 1, 1, 1), (2, 32, 9, 9, 96, 3, 3, 2, 0, 0)
L27, L36, L80 = (2, 3, 17, 17, 32, 3, 3, 2, 0, 0), (2, 4, 10, 10, 16, 6, 6, 1, 0, 0), (2, 80, 8, 8, 32, 3, 3, 1, 1, 1)
GCASES = [
    ("fwd 3x3 s1", "f", L1, "", ("split", True, 1)),
    ("fwd 3x3 s2 bias relu", "f", L2, "b", ("split", False, 2)),          # 128-tile, 2 slabs, gconv_finish_kernel
    ("fwd 1x7", "f", (2, 16, 8, 8, 32, 1, 7, 1, 0, 3), "", ("split", True, 1)),
    ("fwd 7x1", "f", (2, 16, 8, 8, 32, 7, 1, 1, 3, 0), "", ("split", True, 1)),
    ("fwd K27", "f", L27, "", ("fp32", True, 1)),                         # K = 27: not whole chunks
    ("fwd 6x6", "f", L36, "", ("fp32", True, 1)),                         # 36 taps > 25
    ("fwd 3x3 s1 slices", "f", L1, "bs", ("split", True, 1)),             # o_coff > 0 of a wider output, a slice of a wider input
    ("dgrad 3x3 s1", "d", L1, "ma", ("split", True, 2)),                  # M = 16: WIDE
    ("dgrad 3x3 s1 M80", "d", L80, "ma", ("split", False, 2)),            # M = 80: the 128-row tile
    ("dgrad 3x3 s2", "d", L2, "ma", ("fp32", True, 6)),                   # stride 2: fp32
    ("dgrad image", "d", L27, "a", ("image", True, 1)),                   # M = 3, no mask: gconv_image_dgrad_kernel
    ("stats 3x3 s1", "s", L1, "", ("split", True, 1)),
    ("stats 3x3 s2", "s", L2, "", ("split", False, 2)),                   # K split: gconv_finish_stats_kernel
    ("stats K27", "s", L27, "", ("fp32", True, 1)),
]


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _lib():
    from tgsr_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------- discriminators
def _dplan(kind, shape, op):
    """(split form, slabs, workspace) as the planners state them under the current switch"""
    L = _lib()
    B, Cin, Cout, H, W = shape
    form, wsf = (L.tgsr_conv4x4s2_split_form, L.tgsr_conv4x4s2_ws_elems) if kind == 4 else \
        (L.tgsr_conv3x3_gemm_split_form, L.tgsr_conv3x3_gemm_ws_elems)
    T, Ho, Wo = (16, H // 2, W // 2) if kind == 4 else (9, H, W)
    out_elems = (B * Cout * Ho * Wo, B * Cin * H * W, Cout * Cin * T)[op]
    ws = int(wsf(op, B, Cin, H, W, Cout))
    head = 16 * Cin * Cout if (kind == 4 and op == 1) else 0        # (switches 0 / 1: the data gradient's fp32 class pack)
    return int(form(op, B, Cin, H, W, Cout)), max(1, (ws - head) // out_elems), ws


def _dinputs(kind, shape):
    B, Cin, Cout, H, W = shape
    g = _gen("d%d %s" % (kind, shape))
    Ho, Wo = (H // 2, W // 2) if kind == 4 else (H, W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, kind, kind, generator=g) / (Cin * kind * kind) ** 0.5
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    return x, w, dy


def _drun(kind, shape, leaky, op):
    from tgsr_amd import ops
    x, w, dy = _dinputs(kind, shape)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    if kind == 4:
        return (ops.conv4x4s2(xd, wd, leaky) if op == "f" else ops.conv4x4s2_dgrad(dyd, wd, shape[3], shape[4]) if op == "d"
                else ops.conv4x4s2_wgrad(dyd, xd))
    return ops.conv3x3_gemm(xd, wd) if op == "f" else ops.conv3x3_gemm_dgrad(dyd, wd) if op == "d" else ops.conv3x3_gemm_wgrad(dyd, xd)


def _dref(kind, shape, leaky, op):
    x, w, dy = (t.double() for t in _dinputs(kind, shape))
    st, pad = (2, 1) if kind == 4 else (1, 1)
    if op == "f":
        y = F.conv2d(x, w, None, st, pad)
        return F.leaky_relu(y, 0.2) if leaky else y
    if op == "d":
        return torch.nn.grad.conv2d_input(x.shape, w, dy, st, pad)
    return torch.nn.grad.conv2d_weight(x, w.shape, dy, st, pad)


def dcase(case, sw):
    """{key: (digest, report)} of one discriminator case under switch sw; asserts that the planners still name its instance"""
    from tgsr_amd import ops
    kind, shape, leaky, oplist, expect = case
    was = ops.dconv_set_split(1)
    try:
        for op in oplist:
            form, slabs, _ = _dplan(kind, shape, OPS[op])
            assert (form, slabs) == expect[op], "d%d %s %s: the planners say (split form, slabs) = %s, the case claims %s" % (
                kind, shape, op, (form, slabs), expect[op])
        ops.dconv_set_split(sw)
        out = {}
        for op in oplist:
            got = _drun(kind, shape, leaky, op)
            key = "d%d %s%s %s sw%d" % (kind, ",".join(map(str, shape)), " leaky" if leaky else "", op, sw)
            out[key] = (_digest(got), lambda got=got, op=op: "max |out - fp64 conv2d| = %.3g; (split form, slabs, ws) = %s" % (
                float((got.cpu().double() - _dref(kind, shape, leaky, op)).abs().max()), _dplan(kind, shape, OPS[op])))
        torch.cuda.synchronize()
        return out
    finally:
        ops.dconv_set_split(was)


# --------------------------------------------------------------------------------------------------------------- generic taps
def _gplan(mode, geom, flags):
    """(form under gconv_set_form(1), WIDE, slabs): the slabs from tgsr_gconv_nsplit as the launchers use them (no empty slab), the
    form from the conditions include/tgsr_hip.h documents for tgsr_gconv (the library exports no planner for it)"""
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = geom
    OH, OW = (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1
    M, N, K = (Cin, B * H * W, Cout * kh * kw) if mode == "d" else (Cout, B * OH * OW, Cin * kh * kw)
    ns, chunks = int(_lib().tgsr_gconv_nsplit(M, N, K)), (K + 15) // 16
    cps = (chunks + ns - 1) // ns
    ns = (chunks + cps - 1) // cps
    if mode == "d" and M <= 4 and "m" not in flags and M * K * 4 <= 48 * 1024:
        return "image", True, 1
    split = K % 16 == 0 and kh * kw <= 25 and (mode != "d" or st == 1)
    return "split" if split else "fp32", M <= 64, ns


def _ginputs(name, mode, geom, flags):
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = geom
    g = _gen("g " + name)
    OH, OW = (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1
    pre, post = (3, 2) if "s" in flags else (0, 0)
    t = {"x": torch.randn(B, pre + Cin + post, H, W, generator=g),
         "w": torch.randn(Cout, Cin, kh, kw, generator=g) / (Cin * kh * kw) ** 0.5,
         "bias": torch.randn(Cout, generator=g) * 0.2,
         "dy": torch.randn(B, Cout, OH, OW, generator=g),
         "base": torch.randn(B, Cin, H, W, generator=g),
         "mask": (torch.randn(B, Cin, H, W, generator=g) > 0).float()}        # about half zeros
    return t, pre, (5 if "s" in flags else 0), OH, OW


def _grun(name, mode, geom, flags):
    """the output tensors of one case (whole buffers: the channels beside a slice are part of the digest)"""
    from tgsr_amd import ops
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = geom
    t, s_coff, o_coff, OH, OW = _ginputs(name, mode, geom, flags)
    wd = t["w"].to(DEV)
    if mode == "d":
        A = ops.gconv_pack(wd, None, True)
        ws = torch.empty(max(ops.gconv_ws_elems(B, Cin, H, W, Cout * kh * kw), 1), device=DEV)
        dx = t["base"].to(DEV).clone()                                         # prefilled: the cases accumulate
        ops.gconv(True, A, t["dy"].to(DEV), 0, Cout, dx, 0, kh, kw, st, ph, pw, None, False, "a" in flags, ws,
                  t["mask"].to(DEV) if "m" in flags else None)
        return (dx,)
    A = ops.gconv_pack(wd, None, False)
    ws = torch.empty(max(ops.gconv_ws_elems(B, Cout, OH, OW, Cin * kh * kw), 1), device=DEV)
    out = torch.full((B, Cout + (9 if o_coff else 0), OH, OW), 7.0, device=DEV)
    if mode == "s":
        part = ops.gconv_stats(A, t["x"].to(DEV), s_coff, Cin, out, o_coff, kh, kw, st, ph, pw, ws)
        return out, part
    ops.gconv(False, A, t["x"].to(DEV), s_coff, Cin, out, o_coff, kh, kw, st, ph, pw, t["bias"].to(DEV) if "b" in flags else None,
              "b" in flags, False, ws)
    return (out,)


def _gref(name, mode, geom, flags):
    B, Cin, H, W, Cout, kh, kw, st, ph, pw = geom
    t, s_coff, o_coff, OH, OW = _ginputs(name, mode, geom, flags)
    w = t["w"].double()
    if mode == "d":
        dx = torch.nn.grad.conv2d_input((B, Cin, H, W), w, t["dy"].double(), st, (ph, pw))
        dx = dx * t["mask"].double() if "m" in flags else dx
        return dx + t["base"].double() if "a" in flags else dx
    y = F.conv2d(t["x"][:, s_coff:s_coff + Cin].double(), w, t["bias"].double() if "b" in flags else None, st, (ph, pw))
    y = F.relu(y) if "b" in flags else y
    out = torch.full((B, Cout + (9 if o_coff else 0), OH, OW), 7.0, dtype=torch.float64)
    out[:, o_coff:o_coff + Cout] = y
    return out


def gcase(case, form):
    from tgsr_amd import ops
    name, mode, geom, flags, expect = case
    assert _gplan(mode, geom, flags) == expect, "%s: the planners say (form, WIDE, slabs) = %s, the case claims %s" % (
        name, _gplan(mode, geom, flags), expect)
    was = ops.gconv_set_form(bool(form))
    try:
        got = _grun(name, mode, geom, flags)
        torch.cuda.synchronize()
        return {"g %s form%d" % (name, form): (_digest(*got), lambda: "max |out - fp64 conv2d| = %.3g; (form at 1, WIDE, slabs) = %s" % (
            float((got[0].cpu().double() - _gref(name, mode, geom, flags)).abs().max()), _gplan(mode, geom, flags)))}
    finally:
        ops.gconv_set_form(was)


# ------------------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def want():
    assert torch.cuda.is_available()
    with open(FIXTURE) as f:
        return json.load(f)


def _compare(got, want):
    for key, (digest, report) in got.items():
        assert key in want, "%s: not in the fixture" % key
        assert digest == want[key], "%s: the output's bits moved (%s)" % (key, report())


@pytest.mark.parametrize("sw", [1, 0, 3])
@pytest.mark.parametrize("case", DCASES, ids=lambda c: "d%d-%s" % (c[0], "x".join(map(str, c[1]))))
def test_discriminator_conv_bits(case, sw, want):
    _compare(dcase(case, sw), want)


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("case", GCASES, ids=lambda c: c[0].replace(" ", "-"))
def test_generic_tap_bits(case, form, want):
    _compare(gcase(case, form), want)


def test_fixture_holds_exactly_these_cases(want):
    keys = ["d%d %s%s %s sw%d" % (k, ",".join(map(str, s)), " leaky" if lk else "", op, sw) for k, s, lk, ol, _ in DCASES for op in ol
            for sw in (1, 0, 3)] + ["g %s form%d" % (c[0], f) for c in GCASES for f in (1, 0)]
    assert sorted(keys) == sorted(want)


if __name__ == "__main__":
    if "--write" in sys.argv:
        fx = {}
        for c in DCASES:
            for sw in (1, 0, 3):
                fx.update({k: v[0] for k, v in dcase(c, sw).items()})
        for c in GCASES:
            for f in (1, 0):
                fx.update({k: v[0] for k, v in gcase(c, f).items()})
        path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(fx[k])) for k in sorted(fx)) + "\n}\n")
        print("%s: %d digests, %d distinct" % (path, len(fx), len(set(fx.values()))))
