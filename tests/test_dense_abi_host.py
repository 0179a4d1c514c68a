"""CPU: what tests/test_hip_dense_abi.py rests on, checked without a GPU.

  * every refusal of the GPU file's test_refusals, here on host memory: each is a return in front of the first launch;
  * the table against the kernel launches in tgsr_amd/csrc/tgsr_gemm.hip, tgsr_text_tail.hip and tgsr_misc.hip (and tgsr_sumpool2x2's
    in tgsr_bn.hip): every instance they launch has a row with a case, and the table names nothing they do not launch;
  * every launcher's grid arithmetic restated in that file: the cases named for a short last block, a second trip, an idle wave, a
    code branch or a dispatch condition really have one - ca_net_kernel, the row dot product's scalar branch and every tail guard of
    the GEMM among them;
  * the inputs: a non-zero denominator for every ratio bound, the CPU's own fp32 run within every cap of fp64 (a cap the
    reference's arithmetic misses says nothing about a kernel), the saturated cases really saturated, both LeakyReLU sides, every
    bce weight another value;
  * tolerance discrimination, once per case: the fp64 reference built again with one change a kernel bug would make must leave the
    case's tolerance in at least one element.  GEMM: the last k dropped (a K guard one short) and, where there is a bias, the bias
    of row m - 1; row dot product: the sum stops at (K - 1) & ~3; CA_NET: Linear rows i + 2 ncf and ncf + i swapped; bce: w[i - na]
    for the b part (no target where there is no b part); axpy_map: the map indexed by the flat index; affine_act: B and C swapped in
    the channel index; Adam: no bias correction, and weight decay applied after the moments.  A case that cannot tell gets another
    shape, never a wider cap.
"""
import os
import re

import pytest
import torch

import test_hip_dense_abi as A

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgsr_amd", "csrc")
SOURCES = ("tgsr_gemm.hip", "tgsr_text_tail.hip", "tgsr_misc.hip")
ELSEWHERE = {"pack_conv_weight_kernel": "test_hip_infer_abi.py"}           # launched by tgsr_misc.hip, held by another file


def launched(name):
    text = open(os.path.join(CSRC, name)).read()
    return {re.sub(r"\s", "", m) for m in re.findall(r"hipLaunchKernelGGL\(\(?([A-Za-z_0-9]+(?:<[^>]*>)?)", text)}


# ---- the table against the source ----
def test_the_table_names_every_instance_the_sources_launch():
    inst = set().union(*(launched(s) for s in SOURCES))
    for k, where in ELSEWHERE.items():
        assert k in inst and "tgsr_" + k[:-len("_kernel")] in open(os.path.join(os.path.dirname(A.__file__), where)).read()
        inst.remove(k)
    assert A.K_POOL in launched("tgsr_bn.hip")
    inst.add(A.K_POOL)
    assert len(inst) == 21 and {A.K_NN, A.K_NT, A.K_CA_ROWS, A.K_CA_MFMA, A.K_TAIL, A.K_ADV, A.K_ADAM} <= inst
    with_case = " ".join(r[1] for r in A.TABLE if r[3] is not None)
    for k in inst:
        assert k in with_case, k + " has no row with a case"
    named = set(re.findall(r"[a-z_0-9]+_kernel(?:<[a-z]+>)?", " ".join(r[1] for r in A.TABLE)))
    assert named == inst, "the table names an instance the sources do not launch: %s" % sorted(named ^ inst)
    for r in A.TABLE:
        if r[3] is None:
            assert "refused" in r[2] or "in front of the launch" in r[2]
    entries = {r[0] for r in A.TABLE if r[3] is not None}
    assert entries == set(A.SPEC), sorted(entries ^ set(A.SPEC))
    from tgsr_amd import _lib
    for e, spec in A.SPEC.items():                                      # the refusals' argument lists are the bindings'
        assert len(spec) + 1 == len(_lib.SIGNATURES[e][1]), e
    names = [n for n, *_ in A.refusals()]
    assert len(set(names)) == len(names)
    assert set(A.NULLS) == set(A.SIZES) == set(A.SPEC)
    for wanted in ("rowdot_fwd-x-unaligned", "rowdot_fwd-unaligned-scalar-K", "ca_net_fwd-lds-limit", "text_tail_fwd-width-below-T",
                   "multi_copy-17", "multi_copy-odd-size", "multi_copy-negative-size", "multi_copy-all-zero", "axpy_images-5",
                   "axpy_map_fwd-HW-6", "adam_flat-beta1-1", "adam_flat-lr-nan", "adam_flat-param-unaligned", "affine_act_fwd-HW-6"):
        assert wanted in names, wanted


def test_every_refusal_returns_in_front_of_the_first_launch(monkeypatch):
    """The refusals of test_hip_dense_abi.test_refusals on host memory: whatever passed one of them on to a launch would hand a
    kernel a host pointer - or, without a device, answer TGSR_ELAUNCH.  The code each gives, and an untouched arena, say none does."""
    monkeypatch.setattr(A, "DEV", "cpu")
    monkeypatch.setattr(A, "_stream", lambda: None)
    A.test_refusals()


def test_arena_byte_output_off_a_word():
    """place_output_u8(lead=, expect=): the operand starts `lead` bytes into its first word; the bytes in front of it and behind it
    are guarded; a byte still holding PATTERN's counts as unwritten only where the right result is another value."""
    from arena import PATTERN, Arena
    pat = torch.tensor([PATTERN], dtype=torch.int32).view(torch.uint8)          # A5 A5 C5 7F
    expect = torch.tensor([int(pat[1]), 1, 2, 3, 4, 5], dtype=torch.uint8)     # byte 0 of the result IS the pattern's byte there

    def fresh():
        a = Arena("cpu", guard=4)
        x = a.place_input(torch.zeros(2), skew=1)
        out = a.place_output_u8((6,), lead=1, expect=expect)
        assert x.address % 16 == 4 and out.address % 4 == 1 and out.span == 2
        return a, out, a.buffer()[out.offset:out.offset + 2].view(torch.uint8)
    a, out, raw = fresh()
    assert len(a.violations()) == 1 and "5 of 5 elements never written" in a.violations()[0]
    raw[1:7] = expect
    a.check()
    assert torch.equal(out.read(), expect)
    raw[3] = int(pat[3])                                                        # a byte the call had to change still holds the pattern's
    assert any("never written" in v for v in a.violations())
    for where in (0, 7):                                                        # the byte in front of the operand, the one behind it
        a, out, raw = fresh()
        raw[1:7] = expect
        raw[where] = 0
        assert any("outside every output" in v for v in a.violations()), where


def test_arena_byte_input_and_workspace_off_a_word():
    """place_input_u8(lead=) and place_ws_u8(n, lead=): both start `lead` bytes into their first word; a byte input must hold every
    byte, the bytes in front of it and behind it too; a byte workspace may be written in its n bytes and nowhere else."""
    from arena import PATTERN, Arena
    pat = torch.tensor([PATTERN], dtype=torch.int32).view(torch.uint8)
    data = torch.tensor([9, 8, 7, 6, 5], dtype=torch.uint8)

    def fresh():
        a = Arena("cpu", guard=4)
        x = a.place_input_u8(data, lead=3)
        ws = a.place_ws_u8(6, lead=1)
        assert x.address % 4 == 3 and ws.address % 4 == 1 and x.span == 2 and ws.span == 2
        buf = a.buffer()
        return a, x, ws, buf[x.offset:x.offset + 2].view(torch.uint8), buf[ws.offset:ws.offset + 2].view(torch.uint8)
    a, x, ws, rx, rw = fresh()
    a.check()
    assert torch.equal(x.read(), data) and torch.equal(rx[3:8], data) and torch.equal(rx[:3], pat[:3])
    assert torch.equal(rw, torch.cat([pat, pat])) and ws.kind == "ws"
    rw[1:7] = 0                                                                 # all n bytes written: fine; none written: fine too (above)
    a.check()
    for which, where in ((0, 2), (0, 3), (0, 7), (1, 0), (1, 7)):               # in front of the input, its first and last byte; around ws
        a, x, ws, rx, rw = fresh()
        (rx, rw)[which][where] ^= 1
        assert any("outside every output" in v for v in a.violations()), (which, where)
    a, x, ws, rx, rw = fresh()
    rw[1:7] = 3
    a.rearm()
    assert torch.equal(rw, torch.cat([pat, pat]))


def test_arena_byte_inout_with_a_mask():
    """place_inout_u8(t, lead=, may=, expect=): a byte image with prior contents of which the call owns `may`: a byte outside `may`
    (a hole) must keep its value, one inside that has to change and did not counts as unwritten, the bytes around the operand are
    guarded; rearm() puts the prior contents back."""
    from arena import Arena
    prior = torch.tensor([10, 11, 12, 13, 14, 15, 16], dtype=torch.uint8)
    may = torch.tensor([1, 1, 0, 0, 1, 1, 1], dtype=torch.bool)
    expect = torch.tensor([20, 11, 12, 13, 24, 25, 26], dtype=torch.uint8)      # byte 1 is owned and the right value IS the prior one

    def fresh():
        a = Arena("cpu", guard=4)
        img = a.place_inout_u8(prior, lead=2, may=may, expect=expect)
        assert img.address % 4 == 2 and img.span == 3 and img.kind == "inout"
        return a, img, a.buffer()[img.offset:img.offset + 3].view(torch.uint8)
    a, img, raw = fresh()
    assert torch.equal(img.read(), prior)
    assert len(a.violations()) == 1 and "4 of 4 elements never written" in a.violations()[0]
    raw[2:9] = expect
    a.check()
    assert torch.equal(img.read(), expect)
    raw[6] = 14                                                                 # an owned byte that had to change holds the prior value
    assert any("1 of 4 elements never written" in v for v in a.violations())
    for where in (1, 4, 5, 9):                                                  # in front of the operand, the hole's two bytes, behind it
        a, img, raw = fresh()
        raw[2:9] = expect
        raw[where] ^= 1
        assert any("outside every output" in v for v in a.violations()), where
    a, img, raw = fresh()
    raw[2:9] = expect
    a.rearm(ws_fill=1.5)
    assert torch.equal(img.read(), prior)


def test_arena_float_output_with_a_mask():
    """place_masked(base or shape, may): only the elements of `may` are the call's.  Over a shape they start as PATTERN and have to
    be written; over a finite base nothing has to, and an element outside `may` must keep its bits either way."""
    from arena import PATTERN, Arena
    may = torch.tensor([[1, 1, 0], [0, 1, 1]], dtype=torch.bool)
    a = Arena("cpu", guard=4)
    x = a.place_input(torch.zeros(3))
    out = a.place_masked((2, 3), may, skew=1)
    base = torch.arange(6, dtype=torch.float32).reshape(2, 3) + 0.5
    over = a.place_masked(base, may)
    assert x.address % 16 == 0 and out.address % 16 == 4 and over.address % 16 == 0 and out.kind == over.kind == "inout"
    raw, rover = a.buffer()[out.offset:out.offset + 6], a.buffer()[over.offset:over.offset + 6]
    assert bool((raw == PATTERN).all()) and torch.equal(over.read(), base)
    v = a.violations()
    assert len(v) == 1 and "4 of 4 elements never written" in v[0]              # the base is written nowhere and that is fine
    raw.view(torch.float32)[may.reshape(-1)] = 2.0
    a.check()
    assert torch.equal(out.read()[may], torch.full((4,), 2.0)) and bool((out.words()[~may.reshape(-1)] == PATTERN).all())
    rover.view(torch.float32)[4] = -1.0                                         # an owned element of the based output: allowed
    a.check()
    raw.view(torch.float32)[1] = float("inf")
    assert any("non-finite" in m for m in a.violations())
    raw.view(torch.float32)[1] = 2.0
    for region, where in ((raw, 2), (raw, 3), (rover, 2), (rover, 3)):          # the elements outside `may`, PATTERN or base
        keep = int(region[where])
        region[where] = keep ^ 1
        assert any("outside every output" in m for m in a.violations()), where
        region[where] = keep
    a.check()
    a.rearm(ws_fill=1.5)
    assert bool((raw == PATTERN).all()) and torch.equal(over.read(), base)


# ---- the launch arithmetic ----
def test_gemm_rows_have_the_tails_they_name():
    g = A.gemm_plan
    c = A.NN_TAILS
    p = g(c["Cout"], c["N"], c["K"])
    assert (p["row_blocks"], p["last_rows"], p["k_chunks"], p["last_k"], p["col_blocks"], p["last_cols"], p["idle_waves"]) == (2, 8, 2, 6, 2, 2, 3)
    assert c["B"] == 2 and A.NN_SKEW == dict(c, skew=True)
    # every guard of the kernel is false somewhere in this one case: m0 + r < M, k0 + k < K (a_s), kk < K and n < N (bv), n < N and m < M
    assert p["last_rows"] < 32 and p["last_k"] < 64 and p["last_cols"] < 32
    c = A.NN_TILE
    p = g(c["Cout"], c["N"], c["K"])
    assert (p["row_blocks"], p["last_rows"], p["k_chunks"], p["last_k"], p["col_blocks"], p["last_cols"]) == (1, 32, 1, 64, 1, 32) and not c["bias"]
    c = A.NN_MODEL
    p = g(c["Cout"], c["N"], c["K"])
    assert (p["row_blocks"], p["last_rows"], p["k_chunks"], p["last_k"], p["col_blocks"], p["last_cols"]) == (8, 32, 12, 64, 3, 33)
    c = A.NT_33
    p = g(c["Cout"], c["N"], c["K"])
    assert (p["col_blocks"], p["last_cols"], p["idle_waves"], p["last_wave_cols"], p["last_rows"], p["last_k"]) == (1, 33, 2, 1, 8, 6)
    c = A.NT_130
    assert g(c["Cout"], c["N"], c["K"])["col_blocks"] == 2
    c = A.NT_MODEL
    p = g(c["Cout"], c["N"], c["K"])
    assert (p["row_blocks"], p["k_chunks"], p["last_cols"], p["idle_waves"]) == (8, 32, 5, 3)
    assert not A.NT_NOBIAS["bias"] and A.NN_ONE == A.NT_ONE == A._g(1, 1, 1)
    assert [r[3] for r in A._rows(A.CONV1X1)] == [A.NN_TAILS, A.NN_TILE, A.NN_ONE, A.NN_MODEL, A.NN_SKEW]
    assert [r[3] for r in A._rows(A.LINEAR)] == [A.NT_33, A.NT_130, A.NT_MODEL, A.NT_ONE, A.NT_NOBIAS]


def test_rowdot_rows_take_the_branch_they_name():
    rp = A.rowdot_plan
    assert [r[3]["K"] for r in A._rows(A.ROWDOT)] == [8192, 1028, 4, 1023, 257, 1, 1028]
    for _e, instance, _cond, c in A._rows(A.ROWDOT):
        assert instance == A.K_ROWDOT + " " + rp(c["K"])["branch"] and (rp(c["K"])["branch"] == "scalar") == (c["K"] % 4 != 0)
    assert (rp(8192)["trips"], rp(8192)["last_threads"]) == (8, 256)
    assert (rp(1028)["trips"], rp(1028)["last_threads"]) == (2, 1) and (rp(4)["trips"], rp(4)["last_threads"]) == (1, 1)
    assert (rp(1023)["trips"], rp(1023)["last_threads"]) == (4, 255) and (rp(257)["trips"], rp(257)["last_threads"]) == (2, 1)
    assert rp(1)["trips"] == 1 and sum(rp(c["K"])["branch"] == "scalar" for c in A._cases(A.ROWDOT)) == 3
    assert A.rowdot_depth(8192) == 41 and A.rowdot_depth(1) == 10
    for c in A._cases(A.ROWDOT_BWD):                                    # grid ceil(K / 256): the second workgroup holds one k
        assert -(-c["K"] // 256) == 2 and (c["K"] - 1) % 256 + 1 == 1
    assert [(c["B"], c["dx"], c["dw"], c["skew"]) for c in A._cases(A.ROWDOT_BWD)] == [
        (1, True, True, False), (3, True, True, False), (3, False, True, False), (3, True, False, False), (3, True, True, True)]


def test_ca_net_rows_reach_the_kernel_they_name():
    al, off = 0x1000, 0x1004
    for _e, instance, _cond, c in A._rows(A.CA_NET):
        form = A.ca_form(c["tdim"], off if c["skew_s"] else al, off if c["skew_w"] else al)
        assert " ".join(form) == instance, (instance, form)
    mf = [c for c in A._cases(A.CA_NET) if A.ca_form(c["tdim"], al, al)[0] == A.K_CA_MFMA and not (c["skew_w"] or c["skew_s"])]
    assert [c["tdim"] for c in mf] == [256, 64, 320, 48, 16]
    assert {c["ncf"] for c in mf} == {100, 6, 1} and {c["B"] for c in mf} == {17, 1}
    assert any(not c["c_code"] for c in mf) and sum(c["sat"] for c in mf) == 1
    p = A.ca_mfma_plan
    assert (p(256, 100, 17)["trips"], p(256, 100, 17)["last_float4"], p(256, 100, 17)["sample_blocks"], p(256, 100, 17)["last_samples"]) == (1, 4, 2, 1)
    assert (p(64, 6, 1)["trips"], p(64, 6, 1)["last_float4"], p(64, 6, 1)["chan_blocks"], p(64, 6, 1)["last_chans"]) == (1, 1, 2, 2)
    assert (p(320, 1, 17)["trips"], p(320, 1, 17)["last_float4"]) == (2, 1) and p(320, 1, 17)["float4"]
    assert (p(48, 6, 17)["kc"], p(48, 6, 17)["float4"]) == (3, False) and (p(16, 1, 1)["kc"], p(16, 1, 1)["float4"]) == (1, False)
    rows = [c for c in A._cases(A.CA_NET) if c not in mf]
    assert rows == [A.CR_40, A.CR_13, A.CR_13_1, A.CR_64_W, A.CR_64_S]
    q = A.ca_rows_plan
    assert (q(40, 130)["ni"], q(40, 130)["trips"]) == ([65, 65], [2, 2]) and 4 * 65 == 260
    assert q(13, 5)["ni"] == [3, 2] and q(13, 1)["ni"] == [1, 0] and q(13, 1)["trips"] == [1, 0]
    assert A.ca_form(64, al, off) == (A.K_CA_ROWS, "scalar") and A.ca_form(64, off, al) == (A.K_CA_ROWS, "float4")
    assert A.ca_form(48, off, off) == (A.K_CA_MFMA, "scalar")             # tdim % 64 != 0: the MFMA form reads single floats
    assert q(13, 3840)["refused"] and not q(13, 3836)["refused"] and (13 + 4 * 3840) * 4 > 60 * 1024 >= (13 + 4 * 3836) * 4
    for c in rows:
        assert not q(c["tdim"], c["ncf"])["refused"] and q(c["tdim"], c["ncf"])["lds_bytes"] <= 64 * 1024
    for c in A._cases(A.TAIL):                                           # the text tail takes the MFMA form alone
        assert c["tdim"] % 16 == 0 and c["width"] == c["T"] + 3 and c["idf"] % 32 == 0
    assert [(c["B"], c["T"], c["nsets"], c["tdim"]) for c in A._cases(A.TAIL)] == [(17, 5, 3, 48), (2, 32, 1, 64), (1, 1, 4, 16)]
    assert (A.TT_17["idf"], A.TT_17["cdf"], A.TT_17["ncf"]) == (64, 41, 6)


def test_pointwise_rows_make_the_trips_they_name():
    sp = A.stride_plan
    p = sp(3 * A.GLU_BIG, 256, 4096)                                     # tgsr_glu: blocks = min(ceil(n / 256), 4096)
    assert (p["blocks"], p["trips"], p["last"]) == (4096, 2, 5) and sp(21, 256, 4096)["trips"] == 1
    p = sp((A.U8_BIG + 3) // 4, 256, 2048)                               # tgsr_to_uint8: work = ceil(n / 4)
    assert (p["blocks"], p["trips"], p["last"]) == (2048, 2, 1) and A.U8_BIG % 4 == 0
    assert A.u8_branch(A.U8_BIG, 0x1000, 0x2000) == "float4" and A.u8_branch(7, 0x1000, 0x2000) == "scalar"
    assert A.u8_branch(1028, 0x1004, 0x2000) == "scalar" and A.u8_branch(1028, 0x1000, 0x2001) == "scalar"
    assert [(r[3]["n"], r[3]["skew"], r[3]["lead"]) for r in A._rows(A.TO_U8)] == [(A.U8_BIG, 0, 0), (7, 0, 0), (1028, 1, 0), (1028, 0, 1)]
    most = max(A.COPY_BYTES)                                             # tgsr_multi_copy: words = ceil(most / 16), blocks <= 64
    p = sp((most + 15) // 16, 256, 64)
    assert (p["blocks"], p["trips"], p["last"]) == (64, 2, 3) and most == 262192 and most % 16 == 0
    assert len(A.COPY_BYTES) == 16 and {0, 4, 16, 20} <= set(A.COPY_BYTES) and all(b % 4 == 0 for b in A.COPY_BYTES)
    assert A.COPY_BYTES[A.COPY_SRC_SKEW] % 16 == 0 and A.COPY_BYTES[A.COPY_DST_SKEW] % 16 == 0
    assert A.copy_branch(64, 0x1000, 0x2004) == "dword" and A.copy_branch(64, 0x1000, 0x2000) == "uint4" and A.copy_branch(20, 0, 0) == "dword"
    p = sp(A.AXPY_NUMEL[3] // 4, 256, 512)                               # tgsr_axpy_images: blocks = min(ceil(most n4 / 256), 512)
    assert (p["blocks"], p["trips"], p["last"]) == (512, 2, 1) and A.AXPY_NUMEL == (4, 12, 12288, 524292)
    assert sorted(r[3]["n"] for r in A._rows(A.AXPY)) == [1, 2, 3, 4]
    c = A.MAP_BIG                                                        # tgsr_axpy_map_fwd: n4 = BC HW / 4, blocks <= 2048
    p = sp(c["BC"] * c["HW"] // 4, 256, 2048)
    assert (p["blocks"], p["trips"], p["last"]) == (2048, 2, 528000 - 524288)
    hw4 = c["HW"] // 4                                                   # ... _bwd: ceil(hw4 / 256) workgroups
    assert (-(-hw4 // 256), hw4 - 62 * 256) == (63, 128) and A.MAP_SMALL == dict(BC=3, HW=4)
    mb = [r[3] for r in A._rows(A.MAP_BWD)]
    assert [(c["ds"], c["damap"]) for c in mb] == [(True, True), (True, True), (False, True), (True, False)]
    p = A.affine_plan(**A.AFF_WIDE)
    assert (p["grid_y"], p["trips"], p["crosses"]) == (1, 2, True) and A.AFF_WIDE["HW"] % 4 == 0
    assert A.affine_plan(**A.AFF_SMALL) == dict(grid_y=1, trips=1, crosses=True)
    for e in (A.AFF_FWD, A.AFF_BWD):
        assert [(r[3]["C"], r[3]["act"]) for r in A._rows(e)] == [(3, 0), (3, 2), (2048, 2)]
    c = A.BCE_BOTH                                                       # one workgroup of 256 / ceil(n / 256) workgroups
    n = c["na"] + c["nb"]
    assert -(-n // 256) == 3 and n - 512 == 5 and c["na"] % 64 != 0 and c["na"] // 64 == (c["na"] + 1) // 64
    assert A.BCE_ONE == dict(na=1, nb=0, da=True, db=False)
    assert [A.adam_plan(n) for n in A.ADAM_N] == [
        dict(n4=0, tail=1, blocks=1, trips=0), dict(n4=0, tail=3, blocks=1, trips=0), dict(n4=1, tail=3, blocks=1, trips=1),
        dict(n4=257, tail=1, blocks=2, trips=1), dict(n4=1048577, tail=3, blocks=4096, trips=2)]
    assert sorted((r[3]["n"], r[3]["wd"]) for r in A._rows(A.ADAM)) == sorted((n, wd) for n in A.ADAM_N for wd in (0.0, 0.01))
    assert A.ADAM_ADVANCE == (1, 1, 1, 0)
    assert [r[3]["C"] for r in A._rows(A.BN_FOLD)] == [1, 257] and -(-257 // 256) == 2
    assert [(r[3]["half"], r[3]["bwd"]) for r in A._rows(A.GLU)] == [(7, False), (7, True), (A.GLU_BIG, False), (A.GLU_BIG, True)]
    assert [(r[3]["H"], r[3]["W"], r[3]["skew"]) for r in A._rows(A.SUMPOOL)] == [(3, 5, 0), (3, 5, 1)]


# ---- the inputs, the CPU's own fp32 run, and tolerance discrimination ----
@pytest.mark.parametrize("row", A._rows(A.CONV1X1, A.LINEAR), ids=A.row_id)
def test_gemm_references(row):
    entry, _inst, _cond, c = row
    nt = entry == A.LINEAR
    i = A.gemm_inputs(nt, c)
    ref64, ref32 = A.gemm_refs(nt, c)
    tol = A.TOL_GEMM[nt]
    A.close(ref32, ref64, tol, "CPU fp32")
    assert A.max_dist([ref32], [ref64]) > 0.0
    assert A.moved(ref64, A.gemm_reference(nt, c, i, variant="k_last"), tol)
    if c["bias"] and c["Cout"] > 1:
        assert A.moved(ref64, A.gemm_reference(nt, c, i, variant="bias_row"), tol)


@pytest.mark.parametrize("row", A._rows(A.ROWDOT), ids=A.row_id)
def test_rowdot_references(row):
    c = row[3]
    i = A.rowdot_inputs(c)
    ref64, ref32 = A.rowdot_reference(c, i), A.rowdot_reference(c, i, torch.float32)
    cap = A.rowdot_cap(c, i)
    A.close(ref32, ref64, cap, "CPU fp32")
    assert A.max_dist([ref32], [ref64]) > 0.0
    assert A.moved(ref64, A.rowdot_reference(c, i, variant="stops_short"), cap)


@pytest.mark.parametrize("row", A._rows(A.ROWDOT_BWD), ids=A.row_id)
def test_rowdot_backward_references(row):
    c = row[3]
    i = A.rowdot_inputs(c)
    (dx64, dw64), (dx32, dw32) = A.rowdot_bwd_reference(c, i), A.rowdot_bwd_reference(c, i, torch.float32)
    assert A.same_bits(dx32, A.rounded(dx64))                           # one product: the CPU's fp32 run is the rounded fp64 one
    A.close(dw32, dw64, (A.dot_cap(c["B"], (i["dy"].double().abs()[:, None] * i["x"].double().abs()).sum(0)), 0.0), "dw")
    assert A.max_dist([dx32], [dx64]) > 0.0 and A.max_dist([dw32], [dw64]) > 0.0


@pytest.mark.parametrize("c", A._cases(A.CA_NET), ids=A.case_id)
def test_ca_net_references(c):
    i = A.ca_inputs(c)
    ref64, ref32 = A.ca_refs(c)
    keys = ("mu", "logvar") + (("c_code",) if c["c_code"] else ())
    for k in keys:
        A.close(ref32[k], ref64[k], A.TOL_CA, k)
    assert A.max_dist([ref32[k] for k in keys], [ref64[k] for k in keys]) > 0.0
    other = A.ca_reference(c, i, variant="rows_swapped")
    assert A.moved(ref64["mu"], other["mu"], A.TOL_CA) and A.moved(ref64["logvar"], other["logvar"], A.TOL_CA)
    if c["sat"]:                                                        # pre-activations of +-30 and beyond: sigmoids at 0 and at 1
        g = ref64["gates"]
        assert float(g.max()) > 30.0 and float(g.min()) < -30.0
        s = torch.sigmoid(g)
        assert float(s.min()) < 1e-13 and float((1 - s).min()) < 1e-13
    else:
        assert float(ref64["gates"].abs().max()) < 30.0


@pytest.mark.parametrize("c", A._cases(A.TAIL), ids=A.case_id)
def test_text_tail_references(c):
    i = A.tail_inputs(c)
    cap = i["captions"]
    assert cap.shape == (c["B"], c["width"]) and cap.dtype == torch.int64
    inside = cap[:, :c["T"]]
    assert bool((inside == 0).any()) and (c["B"] * c["T"] == 1 or bool((inside != 0).any()))
    src64, mag = A.project_reference(c, i)
    src32, _ = A.project_reference(c, i, torch.float32)
    A.close(src32, src64, (A.dot_cap(c["cdf"], mag) + 1e-45, 0.0), "src_out")
    assert float(src64[..., c["T"]:].abs().sum()) == 0.0
    ref64, ref32 = A.ca_reference(c, i), A.ca_reference(c, i, torch.float32)
    for k in ("mu", "logvar"):
        A.close(ref32[k], ref64[k], A.TOL_CA, k)
        assert A.moved(ref64[k], A.ca_reference(c, i, variant="rows_swapped")[k], A.TOL_CA)


def test_pointwise_references():
    """GLU, bn_fold, sumpool2x2, to_uint8: the CPU's fp32 run within the caps; the inputs hold what the rows say."""
    for half in (7, A.GLU_BIG):
        i = A.glu_inputs(half)
        assert i["x"][0, 1, :3].tolist() == [100.0, -100.0, 0.0]
        for bwd in (False, True):
            ref, cap = A.glu_reference(i, bwd)
            A.close(A.glu_reference(i, bwd, torch.float32)[0], ref, (cap, 0.0), "glu")
    for C in (1, 257):
        i = A.fold_inputs(C)
        assert float(i["var"].min()) == 0.0 and int((i["var"] == 0).sum()) == 1
        s64, t64, cap_s, cap_t = A.fold_reference(i)
        s32, t32, _, _ = A.fold_reference(i, torch.float32)
        A.close(s32, s64, (cap_s, 0.0), "scale")
        A.close(t32, t64, (cap_t, 0.0), "shift")
        assert bool(torch.isfinite(s64).all())
    x = A.pool_input(3, 3, 5)
    A.close(A.pool_reference(x), A.pool_reference(x.double()), (A.dot_cap(2, A.pool_reference(x.double().abs())), 0.0), "sumpool")
    for n in (A.U8_BIG, 7, 1028):
        x = A.u8_input(n)
        assert x.numel() == n and not bool(torch.isnan(x).any())
        assert bool(torch.isinf(x).any()) and float(x[torch.isfinite(x)].min()) < -1.0 and float(x[torch.isfinite(x)].max()) > 1.0
        ref = A.u8_reference(x)
        assert ref.dtype == torch.uint8 and int(ref.min()) == 0 and int(ref.max()) == 255
        if n >= 515:
            k = torch.arange(0, 256, dtype=torch.float32)
            assert torch.equal(x[4:259], (k[:255] + 0.5) / 127.5 - 1.0) and torch.equal(x[259:515], k / 127.5 - 1.0)
            assert len(set(ref[259:515].tolist())) == 256                # every byte value, from its own k / 127.5 - 1
    i = A.axpy_inputs()
    assert tuple(t.numel() for t in i["t"]) == A.AXPY_NUMEL


@pytest.mark.parametrize("c", [A.BCE_ONE, A.BCE_BOTH], ids=A.case_id)
def test_bce_references(c):
    i = A.bce_inputs(c["na"], c["nb"])
    v64, a64, b64 = A.bce_reference(i)
    v32, a32, b32 = A.bce_reference(i, torch.float32)
    assert abs(float(v32) - float(v64)) <= A.bce_value_cap(v64)
    A.close(a32, a64, A.TOL_BCE_GRAD, "da")
    A.close(b32, b64, A.TOL_BCE_GRAD, "db")
    assert len(set(i["w"].tolist())) == c["na"] + c["nb"]
    if c["nb"]:
        l, t = torch.cat([i["a"], i["b"]]), i["t"]
        for v in (100.0, -100.0, 20.0, -20.0, 0.0):
            assert {float(x) for x in t[l == v].tolist()} >= {0.0, 1.0} and bool((t[l == v] == torch.tensor(0.3)).any())
        assert set(l[c["na"] - 3:c["na"] + 3].tolist()) == {100.0, -100.0, 20.0, -20.0, 0.0}
        vv, aa, bb = A.bce_reference(i, variant="b_weights")
        assert abs(float(vv) - float(v64)) > A.bce_value_cap(v64) and A.moved(b64, bb, A.TOL_BCE_GRAD) and not A.moved(a64, aa, A.TOL_BCE_GRAD)
    else:
        i = dict(i, t=torch.tensor([0.3]))                               # (the one target of this case is 0: give the change something to drop)
        v64, a64, _ = A.bce_reference(i)
        vv, aa, _ = A.bce_reference(i, variant="no_target")
        assert abs(float(vv) - float(v64)) > A.bce_value_cap(v64) and A.moved(a64, aa, A.TOL_BCE_GRAD)


@pytest.mark.parametrize("c", [A.MAP_SMALL, A.MAP_BIG], ids=A.case_id)
def test_axpy_map_references(c):
    i = A.map_inputs(c["BC"], c["HW"])
    ref = A.map_reference(i)
    cpu = torch.addcmul(i["t"], i["amap"][None, :], i["s"])             # the CPU's own fp32 run: two roundings, within one ulp
    A.close(cpu, ref, (2 * A.half_ulp(ref), 0.0), "CPU fp32")
    assert A.moved(ref, A.map_reference(i, variant="flat_index"), (A.half_ulp(ref), 0.0))


@pytest.mark.parametrize("row", A._rows(A.AFF_FWD), ids=A.row_id)
def test_affine_act_references(row):
    c = row[3]
    i = A.affine_inputs(c["B"], c["C"], c["HW"])
    ref = A.affine_reference(i, c["act"])
    assert bool((ref > 0).any()) and bool((ref < 0).any())
    cpu = i["raw"] * i["scale"][None, :, None] + i["shift"][None, :, None]
    if c["act"] == 2:
        cpu = torch.nn.functional.leaky_relu(cpu, 0.2)
    # the CPU's own run is not fused: the product's rounding (u |raw scale|, more than an ulp of a result that cancels), the sum's
    # (u |raw scale + shift|), then LeakyReLU's - the fused kernel is held to the 0.5 ulp that this run misses
    prod = (i["raw"].double() * i["scale"].double()[None, :, None]).abs()
    pre = A.affine_reference(i, 0).abs()
    A.close(cpu, ref, (1.01 * A.U * (prod + pre) + A.half_ulp(ref), 0.0), "CPU fp32")
    assert A.moved(ref, A.affine_reference(i, c["act"], variant="b_c_swapped"), (A.half_ulp(ref), 0.0))
    fwd = A.rounded(ref)
    back = A.affine_bwd_reference(i, c["act"], fwd)
    assert A.moved(back, A.affine_bwd_reference(i, c["act"], fwd, variant="b_c_swapped"), (A.half_ulp(back), 0.0))


@pytest.mark.parametrize("row", A._rows(A.ADAM), ids=A.row_id)
def test_adam_references(row):
    n, wd = row[3]["n"], row[3]["wd"]
    i = A.adam_inputs(n)
    assert float(i["g"][0]) == 0.0 and (n == 1 or float(i["g"].max()) == float(torch.tensor(1e18))) and float(i["v"].min()) >= 0.0
    ref = A._adam_ref(n, wd)
    assert ref["state"][0] == 3.0 and all(bool(torch.isfinite(ref[k]).all()) for k in ("p", "m", "v"))
    cpu = A.adam_reference(i, wd, torch.float32)
    for k in ("p", "m", "v"):
        A.close(cpu[k], ref[k], A.TOL_ADAM[k], "CPU fp32 " + k)
    # torch.optim.Adam itself, in fp64: three steps are the reference's first three
    p = torch.nn.Parameter(i["p"].double().clone())
    opt = torch.optim.Adam([p], lr=A.ADAM_HYPER["lr"], betas=(A.ADAM_HYPER["b1"], A.ADAM_HYPER["b2"]), eps=A.ADAM_HYPER["eps"], weight_decay=wd)
    if n <= 1029:
        opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=i["m"].double().clone(), exp_avg_sq=i["v"].double().clone())
        for _ in range(3):
            p.grad = i["g"].double().clone()
            opt.step()
        saved, A.ADAM_ADVANCE = A.ADAM_ADVANCE, (1, 1, 1)
        try:
            three = A.adam_reference(i, wd)
        finally:
            A.ADAM_ADVANCE = saved
        assert float((three["p"] - p.detach()).abs().max()) <= 1e-12 * max(1.0, float(p.detach().abs().max()))
        assert float((three["v"] - opt.state[p]["exp_avg_sq"]).abs().max()) <= 1e-12 * float(opt.state[p]["exp_avg_sq"].abs().max())
    other = A.adam_reference(i, wd, variant="no_bias_correction")
    assert A.moved(ref["p"], other["p"], A.TOL_ADAM["p"])
    if wd:
        other = A.adam_reference(i, wd, variant="decoupled_decay")
        assert A.moved(ref["p"], other["p"], A.TOL_ADAM["p"])
