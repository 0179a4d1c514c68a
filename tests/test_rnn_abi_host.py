"""CPU: what tests/test_hip_rnn_abi.py rests on, checked without a GPU.

  * every refusal of the GPU file's test_refusals, here on host memory: each is a return in front of the first launch;
  * the instance table against the kernel launches in tgsr_amd/csrc/tgsr_lstm.hip (every instance the source launches has a row with
    a case or a refusal), against the library's own planner tgsr_lstm_recurrent_plan, and against the gate GEMM's launch arithmetic
    restated in that file: the cases named for a short last row block, column block or K chunk really have one;
  * the inputs: every length in [1, Tmax], every token in range, ntoken - 1 in use, the restated recurrences equal to the oracle's,
    the CPU's own fp32 run within every elementwise cap of fp64 (a cap the reference's arithmetic misses says nothing about a
    kernel), a non-zero denominator for every ratio bound, and the gates of the saturated cases really saturated;
  * tolerance discrimination, once per case: the fp64 reference built again with one change a kernel bug would make - one length off
    by one, the reverse direction started at Tmax - 1, the sentence code read at column Tmax - 1, two gates swapped, the GRU's b_hn
    moved outside r * (...), and for the backwards d_sent dropped and cprev / hprev taken from step t instead of the previous step -
    must leave the case's tolerance in at least one element.  A case that cannot tell gets another shape, never a wider tolerance.
"""
import os
import re

import pytest
import torch

import test_hip_rnn_abi as A

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgsr_amd", "csrc", "tgsr_lstm.hip")


def _M():
    from tgsr_amd import _lib
    return _lib, _lib.lib()


def _moved(ref, other, tol):
    atol, rtol = tol
    return bool(((ref - other).abs() > atol + rtol * ref.abs()).any())


def launched_instances():
    """Every kernel instance tgsr_lstm.hip launches, spaces dropped: `lstm_recurrent2_kernel<128,24,4>`, `gru_bwd_kernel<32>`, ..."""
    text = open(SRC).read()
    return {re.sub(r"\s", "", m) for m in re.findall(r"hipLaunchKernelGGL\(\(?([A-Za-z_0-9]+(?:<[^>]*>)?)", text)}


# ---- the table against the source, the planner and the restated launch arithmetic ----
def test_the_table_names_every_instance_the_source_launches():
    inst = launched_instances()
    assert len(inst) == 16 and A.REC2 in inst and A.GENERIC in inst and A.GEMM in inst and A.COLSUM in inst
    assert {A.REC % h for h in (32, 64, 128)} | {A.GRU % h for h in (32, 64, 128)} <= inst
    assert {A.LBWD % h for h in (32, 64, 128)} | {A.GRUBWD % h for h in (32, 64, 128)} <= inst
    with_case = " ".join(r[1] for r in A.TABLE if r[3] is not None)
    for k in inst:
        assert k in with_case, k + " has no row with a case"
    named = set(re.findall(r"[a-z_0-9]+_kernel(?:<[0-9,]+>)?", " ".join(r[1] for r in A.TABLE)))
    assert named == inst, "the table names an instance the source does not launch"
    none = [r for r in A.TABLE if r[3] is None]
    assert {r[0] for r in none} == {A.FWD, A.GTFWD, A.BWD, A.GBWD} and all("refused" in r[2] for r in none)
    entries = {r[0] for r in A.TABLE if r[3] is not None}
    assert entries == {A.FWD, A.GT, A.TFWD, A.TRAIN, A.BWD, A.GGT, A.GTFWD, A.GTRAIN, A.GBWD}
    names = {n for n, *_ in A.refusals()}
    assert len(names) == len(A.refusals())
    for e in A.NULLS:                                                   # the refusals cover what the table's None rows say
        assert any(n.startswith(e[5:]) for n in names)
    assert sum("w_hh-unaligned" in n for n in names) == 15


@pytest.mark.parametrize("row", A._rows(A.FWD, A.TFWD, A.TRAIN), ids=A.row_id)
def test_lstm_forward_rows_agree_with_the_planner(row):
    _entry, instance, cond, c = row
    M, L = _M()
    H, Tmax = c["H"], c["Tmax"]
    plan = L.tgsr_lstm_recurrent_plan(H, Tmax)
    assert M.LSTM_RECURRENT[plan] in instance and A.recurrent_instance(c) == M.LSTM_RECURRENT[plan]
    want = (A.REC2 if Tmax <= 24 else A.REC % 128) if H == 128 else A.REC % H if H in (32, 64) else A.GENERIC     # launch_recurrent
    assert M.LSTM_RECURRENT[plan] == want
    assert A.reads_w_hh_as_float4(c) == (plan != M.LSTM_RECURRENT_GENERIC)
    assert (4 * H) % 64 == 0 and H <= 256 and 4 * H <= 1024
    if "fills the TP = 24" in cond:
        assert Tmax == 24 and 24 in c["lens"] and 24 * 4 * H * 4 + 2 * H * 4 + 24 * 4 <= 64 * 1024
    if "the limit" in cond:
        assert H == 256


def test_the_planner_at_its_edges():
    M, L = _M()
    plan = L.tgsr_lstm_recurrent_plan
    if "TGSR_LSTM_ONE_ROW" not in os.environ:
        assert [plan(128, t) for t in (1, 24, 25, 200)] == [1, 1, 2, 2]
    assert [plan(64, 1), plan(64, 100), plan(32, 25)] == [3, 3, 4]
    assert [plan(h, 5) for h in (16, 48, 80, 96, 112, 144, 256)] == [5] * 7
    assert [plan(h, 5) for h in (0, -16, 8, 24, 100, 257, 272, 512)] == [M.EUNSUPPORTED] * 8
    assert sorted(M.LSTM_RECURRENT) == [1, 2, 3, 4, 5] and set(M.LSTM_RECURRENT.values()) <= launched_instances()


def test_gemm_rows_have_the_short_blocks_they_name():
    g = A.gemm_plan
    c = A.L_REC2_FULL                                                   # M = 72, K = 70
    p = g(c["B"] * c["Tmax"], 8 * c["H"], c["ninput"])
    assert (p["row_blocks"], p["last_rows"], p["k_chunks"], p["last_k"], p["col_blocks"], p["last_cols"]) == (3, 8, 2, 6, 8, 128)
    c = A.L_REC128                                                      # M = 50
    p = g(c["B"] * c["Tmax"], 8 * c["H"], c["ninput"])
    assert (p["row_blocks"], p["last_rows"]) == (2, 18)
    c = A.L_REC32                                                       # M = 27, K = 13: one short block, one short chunk
    p = g(c["B"] * c["Tmax"], 8 * c["H"], c["ninput"])
    assert (p["row_blocks"], p["last_rows"], p["k_chunks"], p["last_k"], p["col_blocks"]) == (1, 27, 1, 13, 2)
    p = g(A.NTOKEN, 8 * 32, 13)                                         # the gate tables: M = ntoken = 41
    assert (p["row_blocks"], p["last_rows"]) == (2, 9)
    c = A.G_32                                                          # the GRU at H = 32: N = 192
    p = g(c["B"] * c["Tmax"], 6 * c["H"], c["ninput"])
    assert (p["col_blocks"], p["last_cols"]) == (2, 64) and (6 * c["H"]) % 128 != 0
    c = A.L_GEN48                                                       # N = 384: three full column blocks
    assert g(1, 8 * c["H"], 1)["col_blocks"] == 3 and A.L_GEN16["H"] * 8 == 128
    for r in A.TABLE:
        if r[3] is not None:
            assert A.gate_ws_elems(r[3]) == r[3]["B"] * r[3]["Tmax"] * 2 * (4 if r[3]["cell"] == "lstm" else 3) * r[3]["H"]


def test_the_cases_cover_what_the_table_says():
    fw = A._cases(A.FWD, A.TFWD, A.TRAIN)
    assert [(c["H"], c["Tmax"]) for c in fw] == [(128, 24), (128, 1), (128, 25), (64, 5), (32, 9), (16, 4), (48, 7), (256, 3), (128, 9)]
    assert fw[0]["lens"] == (24, 7, 1) and fw[0]["ninput"] == 70 and fw[1]["B"] == 1 and fw[2]["lens"] == (25, 2)
    assert (fw[4]["B"], fw[4]["ninput"]) == (3, 13) and fw[6]["ninput"] == 13
    gr = A._cases(A.GTFWD, A.GTRAIN)
    assert [c["H"] for c in gr] == [32, 64, 128, 64]
    for cases in (fw, gr):
        assert sum(c["scale"] == 3.0 for c in cases) == 1 and any(c["skew"] for c in cases)
    assert any(c["skew"] and not A.reads_w_hh_as_float4(c) for c in fw) and any(c["skew"] and A.reads_w_hh_as_float4(c) for c in fw)
    for e in (A.BWD, A.GBWD):
        b = [r[3] for r in A._rows(e, chain=False)]
        assert [c["H"] for c in b] == [32, 64, 128] and all(5 <= c["Tmax"] <= 9 for c in b)
        assert sum(not c["d_sent"] for c in b) == 1 and sum(not c["dbias"] for c in b) == 1 and sum(c["skew"] for c in b) == 1
        assert len(A._rows(e, chain=True)) == 1
    for r in A.TABLE:
        c = r[3]
        if c is not None:
            assert 1 <= c["B"] <= 3 and c["width"] == c["Tmax"] + 3 and c["ntoken"] == 41
            assert c["Tmax"] in c["lens"] and (1 in c["lens"] or c["lens"] == (25, 2))


def test_every_refusal_returns_in_front_of_the_first_launch(monkeypatch):
    """The refusals of test_hip_rnn_abi.test_refusals on host memory: whatever passed one of them on to a launch would hand a kernel a
    host pointer - or, without a device, answer TGSR_ELAUNCH.  The code each gives, and an untouched arena, say none does."""
    monkeypatch.setattr(A, "DEV", "cpu")
    monkeypatch.setattr(A, "_stream", lambda: None)
    A.test_refusals()


# ---- the inputs ----
ALL_CASES = A._cases(A.FWD, A.TFWD, A.TRAIN, A.GTFWD, A.GTRAIN, A.BWD, A.GBWD)


@pytest.mark.parametrize("c", ALL_CASES, ids=A.case_id)
def test_inputs_are_regular(c):
    i = A.inputs(c)
    assert all(1 <= n <= c["Tmax"] for n in c["lens"])
    cap = i["captions"]
    assert cap.shape == (c["B"], c["width"]) and int(cap.min()) >= 0 and int(cap.max()) == c["ntoken"] - 1
    assert int(cap[0, 0]) == c["ntoken"] - 1 and c["lens"][0] >= 1     # ... inside a caption
    bound = c["scale"] / c["H"] ** 0.5
    assert float(i["w_hh"].abs().max()) <= bound and float(i["w_hh"].abs().max()) > 0.9 * bound


@pytest.mark.parametrize("c", A._cases(A.FWD, A.TFWD, A.TRAIN, A.GTFWD, A.GTRAIN), ids=A.case_id)
def test_forward_references(c):
    """The restated recurrence IS the oracle's; the CPU's fp32 run is within the forward caps and not exact."""
    i = A.inputs(c)
    (w64, s64), (w32, s32), a64 = A.fwd_refs(c)
    r = A.reference(c, i, grads=False)
    assert float((r["words"] - w64).abs().max()) < 1e-13 and float((r["sent"] - s64).abs().max()) < 1e-13
    A.close(w32, w64, A.TOL_FWD, "words_emb")
    A.close(s32, s64, A.TOL_FWD, "sent_emb")
    a32 = A.reference(c, i, torch.float32, grads=False)["acts"]
    A.close(a32, a64, A.acts_tol(a64), "acts")
    assert A.max_dist([w32, s32], [w64, s64]) > 0.0
    for b, n in enumerate(c["lens"]):
        assert float(w64[b, :, n:].abs().sum()) == 0.0
    if c["scale"] == 3.0:                                               # saturated: |h| near 1, a gate pre-activation beyond +-4.6
        assert float(w64.abs().max()) > 0.85
        gates = a64[..., :2, :] if c["cell"] == "gru" else a64[..., [0, 1, 3], :]       # the sigmoid gates: r, z / i, f, o
        inside = torch.zeros(c["B"], c["Tmax"], dtype=torch.bool)
        for b, n in enumerate(c["lens"]):
            inside[b, :n] = True
        g = gates[inside]
        assert float(torch.minimum(g, 1 - g).min()) < 1e-2


@pytest.mark.parametrize("row", A._rows(A.BWD, A.GBWD), ids=A.row_id)
def test_backward_references(row):
    c = row[3]
    i = A.inputs(c)
    ref64, ref32 = A.bwd_refs(c)
    (w64, s64) = A.oracle_forward(c, i)
    assert float((ref64["words"] - w64).abs().max()) < 1e-13 and float((ref64["sent"] - s64).abs().max()) < 1e-13
    assert torch.equal(ref64["hprev"].float(), A.expected_hprev(c, ref64["words"].float()))
    for k in A.GRAD_KEYS[c["cell"]]:
        A.close(ref32[k], ref64[k], A.grad_tol(ref64[k]), k)
        assert A.max_dist([ref32[k]], [ref64[k]]) > 0.0
        if k != "dbias":
            assert A.zero_behind(ref64[k], c)
    # the manual backward below (the kernels' own formulas) IS autograd's
    man = manual_backward(c, i, ref64)
    for k in A.GRAD_KEYS[c["cell"]]:
        assert float((man[k] - ref64[k]).abs().max()) < 1e-12 * max(1.0, float(ref64[k].abs().max())), k


# ---- tolerance discrimination ----
def _other_lens(c):
    lens = list(c["lens"])
    lens[-1] += 1 if lens[-1] < c["Tmax"] else -1                       # Tmax == 1: the one sample gets length 0, a zero row
    return lens


def _fwd_moved(c, r):
    (w64, s64), _, _ = A.fwd_refs(c)
    return _moved(w64, r["words"], A.TOL_FWD), _moved(s64, r["sent"], A.TOL_FWD)


@pytest.mark.parametrize("c", A._cases(A.FWD, A.TFWD, A.TRAIN, A.GTFWD, A.GTRAIN), ids=A.case_id)
def test_forward_tolerance_discriminates(c):
    i = A.inputs(c)
    ragged = min(c["lens"]) < c["Tmax"]
    w, s = _fwd_moved(c, A.reference(c, i, grads=False, lens=_other_lens(c)))
    assert w and s
    w, s = _fwd_moved(c, A.reference(c, i, grads=False, variant="gates_swapped"))
    assert w and s
    if ragged:                                                          # B == 1: the one sample is full, both changes change nothing
        w, s = _fwd_moved(c, A.reference(c, i, grads=False, variant="reverse_from_Tmax"))
        assert w and s
        w, s = _fwd_moved(c, A.reference(c, i, grads=False, variant="sent_at_Tmax"))
        assert s and not w
    else:
        assert c["B"] == 1
    if c["cell"] == "gru":
        w, s = _fwd_moved(c, A.reference(c, i, grads=False, variant="b_hn_outside"))
        assert w and s


def manual_backward(c, i, ref, stale=""):
    """The kernels' BPTT formulas in fp64 on the reference's acts and words_emb (tgsr_lstm.hip: lstm_bwd_kernel, gru_bwd_kernel);
    stale = "cprev" / "hprev": that operand taken from step t instead of the previous step."""
    H, Tmax, B, lstm = c["H"], c["Tmax"], c["B"], c["cell"] == "lstm"
    acts, words, w_hh = ref["acts"], ref["words"], i["w_hh"].double()
    dw, ds = i["d_words"].double(), i["d_sent"].double()
    G = 4 if lstm else 3
    dgx, dgh = torch.zeros(B, Tmax, 2, G * H, dtype=torch.float64), torch.zeros(B, Tmax, 2, G * H, dtype=torch.float64)
    hprev = torch.zeros(B, Tmax, 2, H, dtype=torch.float64)
    for d in range(2):
        sl = slice(d * H, (d + 1) * H)
        for b, n in enumerate(c["lens"]):
            dh_carry = ds[b, sl].clone() if c["d_sent"] else torch.zeros(H, dtype=torch.float64)
            dc_carry = torch.zeros(H, dtype=torch.float64)
            for s in range(n - 1, -1, -1):
                t = s if d == 0 else n - 1 - s
                tp = t - 1 if d == 0 else t + 1
                zero = torch.zeros(H, dtype=torch.float64)
                hp = words[b, sl, t] if stale == "hprev" else words[b, sl, tp] if s > 0 else zero
                dh = dw[b, sl, t] + dh_carry
                if lstm:
                    ig, fg, gg, og, cc = acts[b, t, d]
                    cprev = cc if stale == "cprev" else acts[b, tp, d, 4] if s > 0 else zero
                    tc = torch.tanh(cc)
                    dc = dc_carry + dh * og * (1 - tc * tc)
                    da = torch.cat([dc * gg * ig * (1 - ig), dc * cprev * fg * (1 - fg), dc * ig * (1 - gg * gg), dh * tc * og * (1 - og)])
                    dc_carry = dc * fg
                    dgx[b, t, d] = dgh[b, t, d] = da
                    dh_carry = w_hh[d].t() @ da
                else:
                    r, z, nn_, hn = acts[b, t, d]
                    dan = dh * (1 - z) * (1 - nn_ * nn_)
                    daz = dh * (hp - nn_) * z * (1 - z)
                    dar = dan * hn * r * (1 - r)
                    dgx[b, t, d] = torch.cat([dar, daz, dan])
                    dgh[b, t, d] = torch.cat([dar, daz, dan * r])
                    dh_carry = dh * z + w_hh[d].t() @ dgh[b, t, d]
                hprev[b, t, d] = hp
    if lstm:
        return dict(dgates=dgx, dbias=dgx.sum((0, 1)), hprev=hprev)
    return dict(dgx=dgx, dgh=dgh, dbias=torch.stack([dgx.sum((0, 1)), dgh.sum((0, 1))]), hprev=hprev)


def _grads_moved(c, ref64, other):
    return [_moved(ref64[k], other[k], A.grad_tol(ref64[k])) for k in A.GRAD_KEYS[c["cell"]] if k != "dbias" or c["dbias"]]


@pytest.mark.parametrize("row", A._rows(A.BWD, A.GBWD), ids=A.row_id)
def test_backward_tolerance_discriminates(row):
    c = row[3]
    i = A.inputs(c)
    ref64, _ = A.bwd_refs(c)
    for kw in (dict(lens=_other_lens(c)), dict(variant="gates_swapped"), dict(variant="reverse_from_Tmax")):
        assert all(_grads_moved(c, ref64, A.reference(c, i, **kw))), kw
    if c["d_sent"]:
        assert all(_grads_moved(c, ref64, A.reference(c, i, variant="d_sent_dropped")))
    if c["cell"] == "gru":
        assert all(_grads_moved(c, ref64, A.reference(c, i, variant="b_hn_outside")))
    # hprev is compared bit for bit: a stale one differs
    stale = manual_backward(c, i, ref64, stale="hprev")
    assert not torch.equal(stale["hprev"].float(), A.expected_hprev(c, ref64["words"].float()))
    if c["cell"] == "gru":                                              # ... and there it enters dz
        assert all(_grads_moved(c, ref64, stale))
    else:
        assert all(_grads_moved(c, ref64, manual_backward(c, i, ref64, stale="cprev")))
