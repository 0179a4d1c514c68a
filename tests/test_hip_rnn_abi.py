"""GPU: the text encoder's LSTM and GRU kernels (tgsr_amd/csrc/tgsr_lstm.hip) held to their C ABI contract, called directly through
ctypes.

    tgsr_bilstm_fwd        tgsr_lstm_gate_table   tgsr_bilstm_table_fwd   tgsr_bilstm_train_fwd   tgsr_bilstm_bwd
    tgsr_gru_gate_table    tgsr_bigru_table_fwd   tgsr_bigru_train_fwd    tgsr_bigru_bwd          (tgsr_lstm_recurrent_plan: host only)

The rest of the suite reaches them through tgsr_amd/ops.py and RNN_ENCODER only: H in {32, 64, 128}, Tmax <= 18 (so neither the
generic recurrence nor lstm_recurrent_kernel<128> ever runs, and lstm_recurrent2_kernel never fills the 24 steps it stages in LDS),
dense operands from the caching allocator, nn.LSTM-initialised weights that keep every gate in its linear range, `acts` zero-filled
by the wrapper.  Here every operand of a call lies in a guarded arena (tests/arena.py): the gate workspace of exactly its
documented size and NaN-prefilled, outputs prefilled with a pattern no arithmetic produces, captions `width = Tmax + 3` wide so the
row stride is real, guard bands around everything.  After a call the guard bands and the inputs hold their bits, every output word
is written and finite, a second call on a workspace holding a finite constant gives the same bits, and the values are within the
suite's own caps of the oracle's recurrences in float64 (oracle.tgsr_oracle.rnn_encoder / rnn_encoder_gru; for the backwards torch
autograd through the same recurrence restated with a zero leaf at every step's gate pre-activations, `lstm_reference` /
`gru_reference` below - tests/test_rnn_abi_host.py holds the restatement to the oracle).

TABLE has one row per (entry point, kernel instance), the dispatch condition copied from the extern "C" launcher; the instance of
every LSTM forward row is asserted from the library's own planner, tgsr_lstm_recurrent_plan.  tests/test_rnn_abi_host.py checks the
table against the kernel launches in the source, the launch arithmetic restated here, the inputs, and that every tolerance tells a
right result from the wrong ones a kernel bug would give.

Elementwise caps are the suite's: words_emb / sent_emb atol 1e-5 (test_hip_parity.py, test_hip_train.py), gradients
atol = 2e-5 max(1, max|ref|), rtol 1e-3 (test_rnn_encoder_train_backward_vs_oracle).  The saved activations `acts` carry the
forward's cap with the cell state's magnitude factored in (1e-5 max(1, max|ref|): the cell state is the one entry not bounded by 1).
1e-5 is 25 to 500 x the distance of the CPU's own fp32 run of the oracle from fp64 at these shapes, so every case also carries the
ratio bound of tests/test_hip_parity_margin.py: max |kernel - f64| over max |CPU fp32 oracle - f64|, R_* below.
"""
import functools

import pytest
import torch

from arena import Arena, PATTERN
from oracle import tgsr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NTOKEN = 41               # the gate tables: two row blocks of the GEMM, the last one 9 rows

# max |kernel - f64| / max |torch CPU fp32 - f64| over a case's outputs: 1.5 x the largest measured ratio of the group, rounded up
# to one decimal (the kernels' summation orders differ from torch's, so the ratio moves with the shape; the rule of R_DIRECT /
# R_WINO in tests/test_hip_train_abi.py).  Measured on the MI355X, 2026-10-20, over every case of the group (the RNN_RATIO lines
# this file prints; profiles/HISTORY.md).  The absolute distances behind them are 0.7e-7 .. 6.7e-7 forward (the largest with saturated
# gates, where the CPU's fp32 run is 3.9e-7 off) and 1.2e-7 .. 7.9e-7 backward: the largest ratios are the shortest recurrences, whose
# CPU runs are 2e-8 .. 3e-8 from fp64.
R_FAST = 6.4              # measured 1.06 .. 4.26 over 10 cases: v_exp_f32 / v_rcp_f32 forms (largest: H = 128, Tmax = 1, B = 1 - one step)
R_GENERIC = 6.5           # measured 1.22 .. 4.32 over 3 cases: library expf / tanhf (largest: H = 256, one chain of 256 FMAs per gate row)
R_LSTM_BWD = 1.8          # measured 0.71 .. 1.15 over 4 cases, dgates and dbias each (largest: dgates at H = 32)
R_GRU_BWD = 1.8           # measured 0.56 .. 1.16 over 4 cases, dgx, dgh and dbias each (largest: dgh behind the kernel's own forward)

FWD, GT, TFWD, TRAIN, BWD = ("tgsr_bilstm_fwd", "tgsr_lstm_gate_table", "tgsr_bilstm_table_fwd", "tgsr_bilstm_train_fwd",
                             "tgsr_bilstm_bwd")
GGT, GTFWD, GTRAIN, GBWD = "tgsr_gru_gate_table", "tgsr_bigru_table_fwd", "tgsr_bigru_train_fwd", "tgsr_bigru_bwd"
GEMM, COLSUM = "lstm_input_gates_kernel", "lstm_colsum_kernel"
REC2, REC, GENERIC = "lstm_recurrent2_kernel<128,24,4>", "lstm_recurrent_kernel<%d>", "lstm_recurrent_generic_kernel"
GRU, LBWD, GRUBWD = "gru_recurrent_kernel<%d>", "lstm_bwd_kernel<%d>", "gru_bwd_kernel<%d>"


# ----------------------------------------------------------------------------------------------------------------------------
# Case fields: cell, H, Tmax, lens (one per sample: B = len(lens)), ninput, scale = factor on the +-1/sqrt(H) weights (3: the gates
# saturate), skew = every operand the code reads by single floats lies one word off 16 bytes (the bits must not change), d_sent /
# dbias = operand given (backward), chain = the backward runs behind the kernel's own training forward.
# ----------------------------------------------------------------------------------------------------------------------------
def _c(cell, H, Tmax, lens, ninput=20, scale=1.0, skew=False, d_sent=True, dbias=True, chain=False):
    assert 1 <= len(lens) <= 3 and all(1 <= n <= Tmax for n in lens) and max(lens) == Tmax
    return dict(cell=cell, H=H, Tmax=Tmax, lens=tuple(lens), B=len(lens), ninput=ninput, ntoken=NTOKEN, width=Tmax + 3,
                scale=scale, skew=skew, d_sent=d_sent, dbias=dbias, chain=chain)


def _lstm_rows(instance, cond, c):
    """The three forward entry points run the same recurrence instance on the same gate pre-activations."""
    return [(FWD, GEMM + " (caption gather) + " + instance, cond, c),
            (TFWD, instance + " through the caption", cond + "; table of " + GT, c),
            (TRAIN, GEMM + " (dense x) + " + instance + ", acts", cond, c)]


def _gru_rows(H, cond, c):
    return [(GTFWD, GRU % H + " through the caption", cond + "; table of " + GGT, c),
            (GTRAIN, GEMM + " (dense x, N = 6H) + " + GRU % H + ", acts", cond, c)]


L_REC2_FULL = _c("lstm", 128, 24, [24, 7, 1], ninput=70)
L_REC2_ONE = _c("lstm", 128, 1, [1])
L_REC128 = _c("lstm", 128, 25, [25, 2])
L_REC64 = _c("lstm", 64, 5, [5, 3, 1])
L_REC32 = _c("lstm", 32, 9, [9, 4, 1], ninput=13, skew=True)
L_GEN16 = _c("lstm", 16, 4, [4, 1, 2])
L_GEN48 = _c("lstm", 48, 7, [7, 1, 3], ninput=13, skew=True)
L_GEN256 = _c("lstm", 256, 3, [3, 1])
L_SAT = _c("lstm", 128, 9, [9, 5, 1], ninput=70, scale=3.0)
G_32 = _c("gru", 32, 6, [6, 1, 3], ninput=13, skew=True)
G_64 = _c("gru", 64, 5, [5, 2, 1])
G_128 = _c("gru", 128, 4, [4, 1])
G_SAT = _c("gru", 64, 7, [7, 2, 1], ninput=70, scale=3.0)

TABLE = (
    # entry point, kernel instance(s), dispatch condition, case (None: refused - the condition says why; test_refusals)
    _lstm_rows(REC2, "H == 128 and Tmax <= 24: Tmax == 24 with a sample of length 24 fills the TP = 24 staged steps; ninput = 70: two K "
               "chunks with a short last one; M = 72", L_REC2_FULL)
    + _lstm_rows(REC2, "H == 128 and Tmax <= 24: Tmax == 1, B == 1", L_REC2_ONE)
    + _lstm_rows(REC % 128, "H == 128 and Tmax > 24: Tmax == 25; M = 50: two row blocks with a short last one", L_REC128)
    + _lstm_rows(REC % 64, "H == 64", L_REC64)
    + _lstm_rows(REC % 32, "H == 32; B = 3, M = 27, ninput = 13; dword-read operands one word off 16 bytes", L_REC32)
    + _lstm_rows(GENERIC, "every other H with 4H % 64 == 0: H == 16, N = 128, 64 threads", L_GEN16)
    + _lstm_rows(GENERIC, "... H == 48, N = 384, ninput = 13; every operand, w_hh included, one word off 16 bytes", L_GEN48)
    + _lstm_rows(GENERIC, "... H == 256: the limit, 1024 threads", L_GEN256)
    + _lstm_rows(REC2, "H == 128 and Tmax <= 24; weights 3 / sqrt(H): saturated gates", L_SAT)
    + [(GT, GEMM + " (M = ntoken)", "ntoken = 41: two row blocks with a short last one; N = 8H", L_REC32),
       (GGT, GEMM + " (M = ntoken, N = 6H)", "H == 32: N = 192, a second column block of 64 columns (`n0 + r < N`, `n < N`)", G_32)]
    + _gru_rows(32, "H == 32; N = 192; dword-read operands one word off 16 bytes", G_32)
    + _gru_rows(64, "H == 64", G_64)
    + _gru_rows(128, "H == 128", G_128)
    + _gru_rows(64, "H == 64; weights 3 / sqrt(H): saturated gates", G_SAT)
    + [(BWD, LBWD % 32 + " + " + COLSUM, "H == 32; dword-read operands one word off 16 bytes", _c("lstm", 32, 9, [9, 4, 1], skew=True)),
       (BWD, LBWD % 64 + " + " + COLSUM, "H == 64; d_sent == NULL", _c("lstm", 64, 5, [5, 3, 1], d_sent=False)),
       (BWD, LBWD % 128, "H == 128; dbias == NULL: no column sum", _c("lstm", 128, 6, [6, 1, 3], dbias=False)),
       (BWD, REC2 + " -> " + LBWD % 128 + " + " + COLSUM, "H == 128, behind the kernel's own training forward",
        _c("lstm", 128, 7, [7, 3, 1], chain=True)),
       (GBWD, GRUBWD % 32 + " + " + COLSUM, "H == 32; dword-read operands one word off 16 bytes", _c("gru", 32, 9, [9, 4, 1], skew=True)),
       (GBWD, GRUBWD % 64 + " + " + COLSUM, "H == 64; d_sent == NULL", _c("gru", 64, 5, [5, 3, 1], d_sent=False)),
       (GBWD, GRUBWD % 128, "H == 128; dbias == NULL: no column sum", _c("gru", 128, 6, [6, 1, 3], dbias=False)),
       (GBWD, GRU % 64 + " -> " + GRUBWD % 64 + " + " + COLSUM, "H == 64, behind the kernel's own training forward",
        _c("gru", 64, 7, [7, 3, 1], chain=True)),
       (FWD, "no instance", "H > 256 or 4H % 64 != 0: refused, as in " + TFWD + " and " + TRAIN, None),
       (FWD, REC % 32 + ", " + REC % 64 + ", " + REC % 128 + ", " + REC2, "w_hh not 16-byte aligned where the instance reads it as float4: "
        "refused, as in " + TFWD + " and " + TRAIN, None),
       (GTFWD, "no instance", "H not in {32, 64, 128}: refused, as in " + GTRAIN, None),
       (GTFWD, GRU % 32 + ", " + GRU % 64 + ", " + GRU % 128, "w_hh not 16-byte aligned: refused, as in " + GTRAIN, None),
       (BWD, "no instance", "H not in {32, 64, 128}: refused", None),
       (GBWD, "no instance", "H not in {32, 64, 128}: refused", None)])


def _rows(*entries, chain=None):
    return [r for r in TABLE if r[0] in entries and r[3] is not None and (chain is None or r[3]["chain"] == chain)]


def _cases(*entries):
    """The distinct cases of these entry points' rows, in table order (the forward forms share a case)."""
    out = []
    for r in _rows(*entries):
        if r[3] not in out:
            out.append(r[3])
    return out


def case_id(c):
    return "%s-H%d-T%d-L%s-K%d%s%s%s%s%s" % (c["cell"], c["H"], c["Tmax"], ".".join(str(n) for n in c["lens"]), c["ninput"],
                                            "-x%g" % c["scale"] if c["scale"] != 1.0 else "", "-skew" if c["skew"] else "",
                                            "" if c["d_sent"] else "-nodsent", "" if c["dbias"] else "-nodbias",
                                            "-chain" if c["chain"] else "")


def row_id(r):
    return r[0][5:] + "-" + case_id(r[3])


# ----------------------------------------------------------------------------------------------------------------------------
# The launchers' arithmetic, restated
# ----------------------------------------------------------------------------------------------------------------------------
def gemm_plan(M, N, K):
    """lstm_input_gates_kernel: grid (ceil(N / 128), ceil(M / 32)), K in chunks of 64; what the last block / chunk of each holds."""
    return dict(row_blocks=-(-M // 32), last_rows=(M - 1) % 32 + 1, col_blocks=-(-N // 128), last_cols=(N - 1) % 128 + 1,
                k_chunks=-(-K // 64), last_k=(K - 1) % 64 + 1)


def gates_per_unit(c):
    return 4 if c["cell"] == "lstm" else 3


def gate_ws_elems(c):
    """gates_ws of the forwards (include/tgsr_hip.h): B * Tmax * 2 * 4H floats, 3H for the GRU."""
    return c["B"] * c["Tmax"] * 2 * gates_per_unit(c) * c["H"]


def recurrent_instance(c):
    """The recurrence instance of a forward case by the library's own planner (the GRU has one instance per H)."""
    from tgsr_amd import _lib as M
    if c["cell"] == "gru":
        return GRU % c["H"]
    return M.LSTM_RECURRENT[M.lib().tgsr_lstm_recurrent_plan(c["H"], c["Tmax"])]


def reads_w_hh_as_float4(c):
    return recurrent_instance(c) != GENERIC


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs and references (CPU; computed once per case and shared)
# ----------------------------------------------------------------------------------------------------------------------------
def _key(c):
    return tuple(sorted(c.items()))


@functools.lru_cache(maxsize=None)
def _inputs(key):
    c = dict(key)
    H, Tmax, B, K, G = c["H"], c["Tmax"], c["B"], c["ninput"], gates_per_unit(c)
    g = torch.Generator().manual_seed(1000 * H + 10 * Tmax + K + (7 if c["cell"] == "gru" else 0))
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * c["scale"] / H ** 0.5       # noqa: E731  nn.LSTM's own init, scaled
    i = dict(emb=torch.randn(c["ntoken"], K, generator=g), w_ih=u(2, G * H, K), w_hh=u(2, G * H, H), b_ih=u(2, G * H), b_hh=u(2, G * H))
    cap = torch.randint(1, c["ntoken"], (B, c["width"]), generator=g)                  # valid tokens behind every caption as well
    cap[0, 0] = c["ntoken"] - 1
    i["captions"] = cap
    i["d_words"] = torch.randn(B, 2 * H, Tmax, generator=g)                            # non-zero behind the captions: never read there
    i["d_sent"] = torch.randn(B, 2 * H, generator=g)
    return i


def inputs(c):
    return _inputs(_key(c))


def state_dict(i, dtype):
    """The operands as the oracle's state dict."""
    sd = {"encoder.weight": i["emb"].to(dtype)}
    for d, suf in enumerate(("", "_reverse")):
        sd["rnn.weight_ih_l0" + suf], sd["rnn.weight_hh_l0" + suf] = i["w_ih"][d].to(dtype), i["w_hh"][d].to(dtype)
        sd["rnn.bias_ih_l0" + suf], sd["rnn.bias_hh_l0" + suf] = i["b_ih"][d].to(dtype), i["b_hh"][d].to(dtype)
    return sd


def oracle_forward(c, i, dtype=torch.float64):
    """(words_emb [B][2H][Tmax], sent_emb [B][2H]) by the oracle in `dtype`."""
    fn = O.rnn_encoder if c["cell"] == "lstm" else O.rnn_encoder_gru
    words, sent = fn(state_dict(i, dtype), i["captions"], list(c["lens"]))
    assert words.shape[2] == c["Tmax"]
    return words.contiguous(), sent


def lstm_reference(c, i, dtype=torch.float64, lens=None, grads=True, variant=""):
    """The LSTM recurrence of the oracle restated with a zero leaf at every step's gate pre-activations: words_emb, sent_emb, acts
    [B][Tmax][2][5][H] = (i, f, g, o, c) and hprev [B][Tmax][2][H] of every step, and by torch autograd dgates [B][Tmax][2][4H] of
    (words_emb * d_words).sum() + (sent_emb * d_sent).sum(), dbias [2][4H] their sum over (b, t).  `variant` makes one change a
    kernel bug would make (tests/test_rnn_abi_host.py)."""
    H, Tmax, B = c["H"], c["Tmax"], c["B"]
    lens = list(c["lens"]) if lens is None else lens
    x = i["emb"].to(dtype)[i["captions"][:, :Tmax]]
    w_ih, w_hh, bias = i["w_ih"].to(dtype), i["w_hh"].to(dtype), (i["b_ih"].to(dtype) + i["b_hh"].to(dtype))
    leaf = torch.zeros(B, Tmax, 2, 4 * H, dtype=dtype, requires_grad=grads)
    words, sent = torch.zeros(B, 2 * H, Tmax, dtype=dtype), torch.zeros(B, 2 * H, dtype=dtype)
    acts, hprev = torch.zeros(B, Tmax, 2, 5, H, dtype=dtype), torch.zeros(B, Tmax, 2, H, dtype=dtype)
    for d in range(2):
        for b in range(B):
            h, cc = torch.zeros(H, dtype=dtype), torch.zeros(H, dtype=dtype)
            n = lens[b]
            steps = range(n) if d == 0 else range((Tmax if variant == "reverse_from_Tmax" else n) - 1, -1, -1)
            for t in steps:
                gts = w_ih[d] @ x[b, t] + w_hh[d] @ h + bias[d] + leaf[b, t, d]
                ig, fg, gg, og = gts[:H], gts[H:2 * H], gts[2 * H:3 * H], gts[3 * H:]
                if variant == "gates_swapped":
                    ig, fg = fg, ig
                ig, fg, gg, og = torch.sigmoid(ig), torch.sigmoid(fg), torch.tanh(gg), torch.sigmoid(og)
                hprev[b, t, d] = h.detach()
                cc = fg * cc + ig * gg
                h = og * torch.tanh(cc)
                words[b, d * H:(d + 1) * H, t] = h
                acts[b, t, d] = torch.stack([ig, fg, gg, og, cc]).detach()
            sent[b, d * H:(d + 1) * H] = words[b, d * H:(d + 1) * H, Tmax - 1] if variant == "sent_at_Tmax" and d == 0 else h
    out = dict(words=words.detach(), sent=sent.detach(), acts=acts, hprev=hprev)
    if grads:
        loss = (words * i["d_words"].to(dtype)).sum()
        if c["d_sent"] and variant != "d_sent_dropped":
            loss = loss + (sent * i["d_sent"].to(dtype)).sum()
        loss.backward()
        out["dgates"], out["dbias"] = leaf.grad, leaf.grad.sum((0, 1))
    return out


def gru_reference(c, i, dtype=torch.float64, lens=None, grads=True, variant=""):
    """The GRU recurrence of the oracle restated with zero leaves at every step's input-side and hidden-side gate pre-activations:
    words_emb, sent_emb, acts [B][Tmax][2][4][H] = (r, z, n, W_hn h + b_hn), hprev, and by torch autograd dgx / dgh [B][Tmax][2][3H],
    dbias [2][2][3H] = their sums over (b, t)."""
    H, Tmax, B = c["H"], c["Tmax"], c["B"]
    lens = list(c["lens"]) if lens is None else lens
    x = i["emb"].to(dtype)[i["captions"][:, :Tmax]]
    w_ih, w_hh, b_ih, b_hh = (i[k].to(dtype) for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
    lx = torch.zeros(B, Tmax, 2, 3 * H, dtype=dtype, requires_grad=grads)
    lh = torch.zeros(B, Tmax, 2, 3 * H, dtype=dtype, requires_grad=grads)
    words, sent = torch.zeros(B, 2 * H, Tmax, dtype=dtype), torch.zeros(B, 2 * H, dtype=dtype)
    acts, hprev = torch.zeros(B, Tmax, 2, 4, H, dtype=dtype), torch.zeros(B, Tmax, 2, H, dtype=dtype)
    for d in range(2):
        for b in range(B):
            h = torch.zeros(H, dtype=dtype)
            n = lens[b]
            steps = range(n) if d == 0 else range((Tmax if variant == "reverse_from_Tmax" else n) - 1, -1, -1)
            for t in steps:
                gi, gh = w_ih[d] @ x[b, t] + b_ih[d] + lx[b, t, d], w_hh[d] @ h + b_hh[d] + lh[b, t, d]
                ri, zi = (gi[:H] + gh[:H], gi[H:2 * H] + gh[H:2 * H])
                if variant == "gates_swapped":
                    ri, zi = zi, ri
                r, z = torch.sigmoid(ri), torch.sigmoid(zi)
                hn = gh[2 * H:]
                nn_ = torch.tanh(gi[2 * H:] + r * (hn - b_hh[d, 2 * H:]) + b_hh[d, 2 * H:]) if variant == "b_hn_outside" \
                    else torch.tanh(gi[2 * H:] + r * hn)
                hprev[b, t, d] = h.detach()
                h = (1 - z) * nn_ + z * h
                words[b, d * H:(d + 1) * H, t] = h
                acts[b, t, d] = torch.stack([r, z, nn_, hn]).detach()
            sent[b, d * H:(d + 1) * H] = words[b, d * H:(d + 1) * H, Tmax - 1] if variant == "sent_at_Tmax" and d == 0 else h
    out = dict(words=words.detach(), sent=sent.detach(), acts=acts, hprev=hprev)
    if grads:
        loss = (words * i["d_words"].to(dtype)).sum()
        if c["d_sent"] and variant != "d_sent_dropped":
            loss = loss + (sent * i["d_sent"].to(dtype)).sum()
        loss.backward()
        out["dgx"], out["dgh"] = lx.grad, lh.grad
        out["dbias"] = torch.stack([lx.grad.sum((0, 1)), lh.grad.sum((0, 1))])
    return out


def reference(c, i, dtype=torch.float64, **kw):
    return (lstm_reference if c["cell"] == "lstm" else gru_reference)(c, i, dtype, **kw)


@functools.lru_cache(maxsize=None)
def _fwd_refs(key):
    c = dict(key)
    i = _inputs(key)
    return oracle_forward(c, i), oracle_forward(c, i, torch.float32), reference(c, i, grads=False)["acts"]


def fwd_refs(c):
    """((words_emb, sent_emb) by the oracle in fp64, the same in fp32, acts of the restated recurrence in fp64)."""
    return _fwd_refs(_key(c))


@functools.lru_cache(maxsize=None)
def _bwd_refs(key):
    c = dict(key)
    i = _inputs(key)
    return reference(c, i), reference(c, i, torch.float32)


def bwd_refs(c):
    """(the restated recurrence and its gradients in fp64, the same in fp32)."""
    return _bwd_refs(_key(c))


GRAD_KEYS = {"lstm": ("dgates", "dbias"), "gru": ("dgx", "dgh", "dbias")}
TOL_FWD = (1e-5, 0.0)


def acts_tol(ref):
    return 1e-5 * max(1.0, float(ref.abs().max())), 0.0


def grad_tol(ref):
    return 2e-5 * max(1.0, float(ref.abs().max())), 1e-3


def close(got, ref, tol, what=""):
    atol, rtol = tol
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d of %d values beyond atol %.3g rtol %.3g, worst |err| %.3g at |ref| %.3g" % (
        what, int(bad.sum()), bad.numel(), atol, rtol, float(err.max()), float(ref.abs().flatten()[int(err.argmax())]))


def max_dist(xs, refs):
    return max(float((x.double() - r.double()).abs().max()) for x, r in zip(xs, refs))


def ratio_ok(tag, group, got, ref64, ref32, bound):
    """max |kernel - f64| against max |CPU fp32 - f64| over the listed outputs together."""
    own, cpu = max_dist(got, ref64), max_dist(ref32, ref64)
    print("RNN_RATIO %s %s own %.4g cpu %.4g ratio %s" % (tag, group, own, cpu, "%.3f" % (own / cpu) if cpu else "-"))
    assert cpu > 0.0, "%s: the CPU fp32 run is exact: the case says nothing" % tag
    assert own <= bound * cpu, "%s %s: max |kernel - f64| = %.3g is %.2f x the CPU fp32 run's %.3g (bound %.1f)" % (
        tag, group, own, own / cpu, cpu, bound)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def pattern_rows(t, c, lens=None):
    """`t` [B][Tmax][...] with the arena's pattern in the rows of the steps behind every caption."""
    t = t.clone().contiguous()
    for b, n in enumerate(c["lens"] if lens is None else lens):
        t[b, max(0, min(n, c["Tmax"])):].view(torch.int32).fill_(PATTERN)
    return t


def is_pattern(t):
    return bool((t.contiguous().view(torch.int32) == PATTERN).all())


def no_pattern(t):
    return not bool((t.contiguous().view(torch.int32) == PATTERN).any())


# ----------------------------------------------------------------------------------------------------------------------------
# Calls
# ----------------------------------------------------------------------------------------------------------------------------
def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    from tgsr_amd import ops
    return ops._stream()


def _p(r):
    return r.ptr if r is not None else None


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32)


def _twice(a, call, outs, M, wss=(), first=None):
    """The call on NaN workspaces, then on workspaces holding 1.0: the arena's contract both times, the same bits in every output and
    in every word of `wss` the first call wrote; `first` inspects the arena after the first call.  Returns the outputs."""
    assert call() == M.OK
    a.check()
    got, w1 = [o.read() for o in outs], [w.read().view(torch.int32) for w in wss]
    if first is not None:
        first()
    a.rearm(ws_fill=1.0)
    assert call() == M.OK
    a.check()
    for g, o in zip(got, outs):
        assert same_bits(g, o.read()), "the result depends on what the workspace held"
    for w, r in zip(w1, wss):
        w2, wrote = r.read().view(torch.int32), w != PATTERN
        assert torch.equal(w[wrote], w2[wrote]), "a workspace word depends on what the workspace held"
        assert bool((w2[~wrote] == 0x3F800000).all()), "the second call wrote workspace words the first did not"
    return got


def _w_hh(a, c, w, skew):
    """w_hh of a forward call: off 16 bytes only where the planner names the instance that reads it by single floats."""
    s = 1 if skew and not reads_w_hh_as_float4(c) else 0
    r = a.place_input(w, skew=s)
    return r, s


def _gru_biases(i, H):
    b_rz = i["b_hh"].clone()
    b_rz[:, 2 * H:] = 0
    return b_rz, i["b_hh"][:, 2 * H:].contiguous()


def run_fwd(M, L, c, i, skew=False, lens=None, captions=None):
    """tgsr_bilstm_fwd in an arena of its own: (words_emb, sent_emb)."""
    assert c["cell"] == "lstm"
    B, H, Tmax, s = c["B"], c["H"], c["Tmax"], 1 if skew else 0
    a = Arena(DEV)
    cap = a.place_input(i["captions"] if captions is None else captions)
    ln = a.place_input(_i32(c["lens"] if lens is None else lens))
    emb, w_ih = a.place_input(i["emb"], skew=s), a.place_input(i["w_ih"], skew=s)
    w_hh, ws_ = _w_hh(a, c, i["w_hh"], skew)
    b_ih, b_hh = a.place_input(i["b_ih"], skew=s), a.place_input(i["b_hh"], skew=s)
    ws = a.place_ws(gate_ws_elems(c), skew=s)
    words, sent = a.place_output((B, 2 * H, Tmax), skew=s), a.place_output((B, 2 * H), skew=s)
    assert w_hh.address % 16 == 4 * ws_ and (ws_ == 0 or not reads_w_hh_as_float4(c))

    def call():
        return L.tgsr_bilstm_fwd(cap.ptr, c["width"], ln.ptr, B, Tmax, emb.ptr, c["ntoken"], c["ninput"], w_ih.ptr, w_hh.ptr, b_ih.ptr,
                                 b_hh.ptr, H, ws.ptr, words.ptr, sent.ptr, _stream())
    return _twice(a, call, [words, sent], M, wss=[ws])


def run_gate_table(M, L, c, i, skew=False):
    """tgsr_lstm_gate_table / tgsr_gru_gate_table in an arena of its own: table [ntoken][2][4H | 3H]."""
    H, s, G = c["H"], 1 if skew else 0, gates_per_unit(c)
    a = Arena(DEV)
    emb, w_ih, b_ih = a.place_input(i["emb"], skew=s), a.place_input(i["w_ih"], skew=s), a.place_input(i["b_ih"], skew=s)
    b2 = a.place_input(i["b_hh"] if c["cell"] == "lstm" else _gru_biases(i, H)[0], skew=s)
    table = a.place_output((c["ntoken"], 2, G * H), skew=s)
    fn = L.tgsr_lstm_gate_table if c["cell"] == "lstm" else L.tgsr_gru_gate_table

    def call():
        return fn(emb.ptr, c["ntoken"], c["ninput"], w_ih.ptr, b_ih.ptr, b2.ptr, H, table.ptr, _stream())
    return _twice(a, call, [table], M)[0]


def run_table_fwd(M, L, c, i, table, skew=False, lens=None, captions=None):
    """tgsr_bilstm_table_fwd / tgsr_bigru_table_fwd in an arena of its own: (words_emb, sent_emb)."""
    B, H, Tmax, s = c["B"], c["H"], c["Tmax"], 1 if skew else 0
    a = Arena(DEV)
    cap = a.place_input(i["captions"] if captions is None else captions)
    ln = a.place_input(_i32(c["lens"] if lens is None else lens))
    tb = a.place_input(table, skew=s)
    w_hh, ws_ = _w_hh(a, c, i["w_hh"], skew)
    bn = a.place_input(_gru_biases(i, H)[1], skew=s) if c["cell"] == "gru" else None
    words, sent = a.place_output((B, 2 * H, Tmax), skew=s), a.place_output((B, 2 * H), skew=s)
    assert w_hh.address % 16 == 4 * ws_ and (ws_ == 0 or not reads_w_hh_as_float4(c))

    def call():
        if c["cell"] == "lstm":
            return L.tgsr_bilstm_table_fwd(cap.ptr, c["width"], ln.ptr, B, Tmax, tb.ptr, c["ntoken"], w_hh.ptr, H, words.ptr, sent.ptr,
                                           _stream())
        return L.tgsr_bigru_table_fwd(cap.ptr, c["width"], ln.ptr, B, Tmax, tb.ptr, c["ntoken"], w_hh.ptr, bn.ptr, H, words.ptr,
                                      sent.ptr, _stream())
    return _twice(a, call, [words, sent], M)


def run_train_fwd(M, L, c, i, skew=False, lens=None):
    """tgsr_bilstm_train_fwd / tgsr_bigru_train_fwd on x = emb[captions] in an arena of its own: (words_emb, sent_emb, acts as the
    arena holds it after the call: the pattern wherever no step wrote)."""
    B, H, Tmax, s, NA = c["B"], c["H"], c["Tmax"], 1 if skew else 0, 5 if c["cell"] == "lstm" else 4
    lens = list(c["lens"] if lens is None else lens)
    a = Arena(DEV)
    x = a.place_input(i["emb"][i["captions"][:, :Tmax]], skew=s)
    ln = a.place_input(_i32(lens))
    w_ih = a.place_input(i["w_ih"], skew=s)
    w_hh, ws_ = _w_hh(a, c, i["w_hh"], skew)
    b_ih = a.place_input(i["b_ih"], skew=s)
    if c["cell"] == "lstm":
        b_hh, bn = a.place_input(i["b_hh"], skew=s), None
    else:
        b_rz, b_hn = _gru_biases(i, H)
        b_hh, bn = a.place_input(b_rz, skew=s), a.place_input(b_hn, skew=s)
    ws = a.place_ws(gate_ws_elems(c), skew=s)
    acts = a.place_ws(B * Tmax * 2 * NA * H, skew=s)          # a workspace to the arena: its rows behind a caption stay unwritten
    words, sent = a.place_output((B, 2 * H, Tmax), skew=s), a.place_output((B, 2 * H), skew=s)
    assert w_hh.address % 16 == 4 * ws_ and (ws_ == 0 or not reads_w_hh_as_float4(c))
    seen = []

    def call():
        if c["cell"] == "lstm":
            return L.tgsr_bilstm_train_fwd(x.ptr, ln.ptr, B, Tmax, c["ninput"], w_ih.ptr, w_hh.ptr, b_ih.ptr, b_hh.ptr, H, ws.ptr,
                                           acts.ptr, words.ptr, sent.ptr, _stream())
        return L.tgsr_bigru_train_fwd(x.ptr, ln.ptr, B, Tmax, c["ninput"], w_ih.ptr, w_hh.ptr, b_ih.ptr, b_hh.ptr, bn.ptr, H, ws.ptr,
                                      acts.ptr, words.ptr, sent.ptr, _stream())

    def first():
        got = acts.read().reshape(B, Tmax, 2, NA, H)
        for b, n in enumerate(lens):
            n = max(0, min(n, Tmax))
            assert no_pattern(got[b, :n]) and bool(torch.isfinite(got[b, :n]).all()), "acts of a step inside the caption is unwritten"
            assert is_pattern(got[b, n:]), "acts rows behind the caption were written"
        seen.append(got)
    words_, sent_ = _twice(a, call, [words, sent], M, wss=[ws, acts], first=first)
    return words_, sent_, seen[0]


def run_bwd(M, L, c, i, acts, words, skew=False, lens=None, d_sent=None, dbias=None):
    """tgsr_bilstm_bwd / tgsr_bigru_bwd in an arena of its own: dict of the outputs (dbias None where it is not asked for)."""
    B, H, Tmax, s, G = c["B"], c["H"], c["Tmax"], 1 if skew else 0, gates_per_unit(c)
    d_sent, dbias = c["d_sent"] if d_sent is None else d_sent, c["dbias"] if dbias is None else dbias
    a = Arena(DEV)
    ln = a.place_input(_i32(c["lens"] if lens is None else lens))
    w_hh, ac, wd = a.place_input(i["w_hh"], skew=s), a.place_input(acts, skew=s), a.place_input(words, skew=s)
    dw = a.place_input(i["d_words"], skew=s)
    ds = a.place_input(i["d_sent"], skew=s) if d_sent else None
    dg = [a.place_output((B, Tmax, 2, G * H), skew=s) for _ in range(1 if c["cell"] == "lstm" else 2)]
    hp = a.place_output((B, Tmax, 2, H), skew=s)
    db = a.place_output((2, 4 * H) if c["cell"] == "lstm" else (2, 2, 3 * H), skew=s, written=dbias)

    def call():
        args = [ln.ptr, B, Tmax, H, w_hh.ptr, ac.ptr, wd.ptr, dw.ptr, _p(ds)] + [r.ptr for r in dg] + [hp.ptr, db.ptr if dbias else None,
                                                                                                        _stream()]
        return (L.tgsr_bilstm_bwd if c["cell"] == "lstm" else L.tgsr_bigru_bwd)(*args)
    got = _twice(a, call, dg + [hp] + ([db] if dbias else []), M)
    out = dict(zip(("dgates",) if c["cell"] == "lstm" else ("dgx", "dgh"), got[:len(dg)]))
    out["hprev"], out["dbias"] = got[len(dg)], got[-1] if dbias else None
    return out


def expected_hprev(c, words, lens=None):
    """hprev [B][Tmax][2][H] as the backward copies it out of words_emb: the hidden state that entered step t, zero at a direction's
    first step and behind the caption."""
    H, Tmax = c["H"], c["Tmax"]
    hp = torch.zeros(c["B"], Tmax, 2, H)
    for b, n in enumerate(c["lens"] if lens is None else lens):
        n = max(0, min(n, Tmax))
        for t in range(n):
            if t > 0:
                hp[b, t, 0] = words[b, :H, t - 1]
            if t + 1 < n:
                hp[b, t, 1] = words[b, H:, t + 1]
    return hp


def zero_behind(t, c, lens=None):
    """`t` [B][Tmax][...] is exactly zero at the steps behind every caption."""
    return all(float(t[b, max(0, min(n, c["Tmax"])):].abs().sum()) == 0.0 for b, n in enumerate(c["lens"] if lens is None else lens))


# ----------------------------------------------------------------------------------------------------------------------------
# Forward
# ----------------------------------------------------------------------------------------------------------------------------
def _forward_checks(c, words, sent, acts, group, bound):
    (w64, s64), (w32, s32), a64 = fwd_refs(c)
    for b, n in enumerate(c["lens"]):
        assert float(words[b, :, n:].abs().sum()) == 0.0, "words_emb[b, :, t >= len] is exactly zero"
    close(words, w64, TOL_FWD, "words_emb")
    close(sent, s64, TOL_FWD, "sent_emb")
    inside = torch.zeros(c["B"], c["Tmax"], dtype=torch.bool)
    for b, n in enumerate(c["lens"]):
        inside[b, :n] = True
    close(acts[inside], a64[inside], acts_tol(a64), "acts")
    ratio_ok(case_id(c), group, [words, sent], [w64, s64], [w32, s32], bound)


@pytest.mark.parametrize("c", _cases(FWD, TFWD, TRAIN), ids=case_id)
def test_lstm_forward_entry_points(c):
    """tgsr_bilstm_fwd, tgsr_bilstm_table_fwd over tgsr_lstm_gate_table and tgsr_bilstm_train_fwd on x = emb[captions]: one result, bit
    for bit (the same GEMM arithmetic per row, the same recurrence), within the caps of the fp64 oracle."""
    M, L = _lib()
    i = inputs(c)
    instance = recurrent_instance(c)
    assert all(instance in r[1] for r in TABLE if r[3] == c and r[0] in (FWD, TFWD, TRAIN))
    words, sent = run_fwd(M, L, c, i, skew=c["skew"])
    table = run_gate_table(M, L, c, i, skew=c["skew"])
    ref_table = torch.einsum("tk,dnk->tdn", i["emb"].double(), i["w_ih"].double()) + (i["b_ih"] + i["b_hh"]).double()
    close(table, ref_table, TOL_FWD, "gate table")
    tw, ts = run_table_fwd(M, L, c, i, table, skew=c["skew"])
    assert same_bits(words, tw) and same_bits(sent, ts), "the table form differs from tgsr_bilstm_fwd"
    nw, ns, acts = run_train_fwd(M, L, c, i, skew=c["skew"])
    assert same_bits(words, nw) and same_bits(sent, ns), "the training form on x = emb[captions] differs from tgsr_bilstm_fwd"
    if c["skew"]:                                              # one word off 16 bytes: the same bits as aligned
        aw, as_ = run_fwd(M, L, c, i)
        assert same_bits(words, aw) and same_bits(sent, as_)
        assert same_bits(table, run_gate_table(M, L, c, i))
        a_nw, a_ns, a_acts = run_train_fwd(M, L, c, i)
        assert same_bits(nw, a_nw) and same_bits(ns, a_ns) and same_bits(acts, a_acts)
    generic = instance == GENERIC
    _forward_checks(c, words, sent, acts, "generic" if generic else "fast", R_GENERIC if generic else R_FAST)


@pytest.mark.parametrize("c", _cases(GTFWD, GTRAIN), ids=case_id)
def test_gru_forward_entry_points(c):
    """tgsr_bigru_table_fwd over tgsr_gru_gate_table and tgsr_bigru_train_fwd on x = emb[captions]: one result, bit for bit, within
    the caps of the fp64 oracle."""
    M, L = _lib()
    i = inputs(c)
    H = c["H"]
    table = run_gate_table(M, L, c, i, skew=c["skew"])
    ref_table = torch.einsum("tk,dnk->tdn", i["emb"].double(), i["w_ih"].double()) + (i["b_ih"] + _gru_biases(i, H)[0]).double()
    close(table, ref_table, TOL_FWD, "gate table")
    words, sent = run_table_fwd(M, L, c, i, table, skew=c["skew"])
    nw, ns, acts = run_train_fwd(M, L, c, i, skew=c["skew"])
    assert same_bits(words, nw) and same_bits(sent, ns), "the training form on x = emb[captions] differs from the table form"
    if c["skew"]:
        a_table = run_gate_table(M, L, c, i)
        assert same_bits(table, a_table)
        aw, as_ = run_table_fwd(M, L, c, i, a_table)
        assert same_bits(words, aw) and same_bits(sent, as_)
        a_nw, a_ns, a_acts = run_train_fwd(M, L, c, i)
        assert same_bits(nw, a_nw) and same_bits(ns, a_ns) and same_bits(acts, a_acts)
    _forward_checks(c, words, sent, acts, "fast", R_FAST)


@pytest.mark.parametrize("c", [L_REC32, L_GEN16, G_32], ids=case_id)
def test_lengths_and_tokens_as_the_code_has_them(c):
    """include/tgsr_hip.h: a length above Tmax acts as Tmax, a length <= 0 gives zero rows and a zero sentence code, a caption entry
    outside [0, ntoken) reads row 0 - in the gather of the gate GEMM (tgsr_bilstm_fwd) and in the recurrence's own (table forms)."""
    M, L = _lib()
    i = inputs(c)
    Tmax, lens = c["Tmax"], list(c["lens"])
    assert lens[0] == Tmax and len(lens) == 3
    table = run_gate_table(M, L, c, i)
    forms = [lambda **kw: run_table_fwd(M, L, c, i, table, **kw)]
    if c["cell"] == "lstm":
        forms.append(lambda **kw: run_fwd(M, L, c, i, **kw))
    zero_tok, bad_tok = i["captions"].clone(), i["captions"].clone()
    zero_tok[0, 1], zero_tok[1, 0] = 0, 0
    bad_tok[0, 1], bad_tok[1, 0] = -1, c["ntoken"]
    for form in forms:
        words, sent = form()
        w2, s2 = form(lens=[Tmax + 5, 0, lens[2]])
        assert same_bits(words[0], w2[0]) and same_bits(sent[0], s2[0]), "a length above Tmax acts as Tmax"
        assert same_bits(words[2], w2[2]) and same_bits(sent[2], s2[2])
        assert float(w2[1].abs().sum()) == 0.0 and float(s2[1].abs().sum()) == 0.0, "length 0: zero rows, a zero sentence code"
        w3, s3 = form(lens=[Tmax, -4, lens[2]])
        assert same_bits(w2, w3) and same_bits(s2, s3)
        wz, sz = form(captions=zero_tok)
        wb, sb = form(captions=bad_tok)
        assert same_bits(wz, wb) and same_bits(sz, sb), "a token of -1 or ntoken gives the bits of token 0"
        assert not same_bits(words, wz), "the replaced tokens are inside their captions"
    nw, ns, acts = run_train_fwd(M, L, c, i, lens=[Tmax + 5, 0, lens[2]])         # acts: first() holds the rows to the clamped lengths
    assert float(nw[1].abs().sum()) == 0.0 and float(ns[1].abs().sum()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------
# Backward
# ----------------------------------------------------------------------------------------------------------------------------
def _backward_checks(c, got, words_in, ref64, ref32, group, bound):
    assert same_bits(got["hprev"], expected_hprev(c, words_in)), "hprev is words_emb of the previous step, zero elsewhere"
    keys = GRAD_KEYS[c["cell"]]
    for k in keys:
        if k == "dbias":
            if not c["dbias"]:
                assert got[k] is None
                continue
        else:
            assert zero_behind(got[k], c), k + " is exactly zero behind every caption"
        close(got[k], ref64[k], grad_tol(ref64[k]), k)
    for k in keys:
        if got[k] is not None:
            ratio_ok(case_id(c), group + "/" + k, [got[k]], [ref64[k]], [ref32[k]], bound)


@pytest.mark.parametrize("row", _rows(BWD, GBWD, chain=False), ids=row_id)
def test_backward_entry_points_in_isolation(row):
    """acts and words_emb of the fp64 reference rounded once to fp32, acts with the arena's pattern in the rows behind every caption
    (the forward never writes them; the backward must not read them), d_words non-zero behind the captions."""
    entry, instance, _cond, c = row
    M, L = _lib()
    i = inputs(c)
    ref64, ref32 = bwd_refs(c)
    assert (LBWD if entry == BWD else GRUBWD) % c["H"] in instance and (COLSUM in instance) == c["dbias"]
    acts, words = pattern_rows(ref64["acts"].float(), c), ref64["words"].float()
    got = run_bwd(M, L, c, i, acts, words, skew=c["skew"])
    if c["skew"]:
        al = run_bwd(M, L, c, i, acts, words)
        assert all(same_bits(got[k], al[k]) for k in got if got[k] is not None)
    _backward_checks(c, got, words, ref64, ref32, "lstm_bwd" if entry == BWD else "gru_bwd", R_LSTM_BWD if entry == BWD else R_GRU_BWD)


@pytest.mark.parametrize("row", _rows(BWD, GBWD, chain=True), ids=row_id)
def test_backward_behind_the_kernels_own_forward(row):
    """The training forward's acts as the arena holds them - the pattern still in the rows behind every caption - and its words_emb go
    into the backward unchanged."""
    entry, _instance, _cond, c = row
    M, L = _lib()
    i = inputs(c)
    ref64, ref32 = bwd_refs(c)
    words, sent, acts = run_train_fwd(M, L, c, i)
    close(words, ref64["words"], TOL_FWD, "words_emb")
    close(sent, ref64["sent"], TOL_FWD, "sent_emb")
    assert all(is_pattern(acts[b, n:]) for b, n in enumerate(c["lens"]))
    got = run_bwd(M, L, c, i, acts, words)
    _backward_checks(c, got, words, ref64, ref32, "lstm_bwd" if entry == BWD else "gru_bwd", R_LSTM_BWD if entry == BWD else R_GRU_BWD)


@pytest.mark.parametrize("row", [r for r in _rows(BWD, GBWD, chain=False) if r[3]["H"] == 32], ids=row_id)
def test_backward_lengths_as_the_code_has_them(row):
    """A length above Tmax acts as Tmax; a length <= 0 gives all-zero gradient and hprev rows (include/tgsr_hip.h)."""
    c = row[3]
    M, L = _lib()
    i = inputs(c)
    ref64, _ = bwd_refs(c)
    Tmax, lens = c["Tmax"], list(c["lens"])
    assert lens[0] == Tmax
    other = [Tmax + 5, 0, lens[2]]
    words = ref64["words"].float()
    base = run_bwd(M, L, c, i, pattern_rows(ref64["acts"].float(), c), words, dbias=False)
    got = run_bwd(M, L, c, i, pattern_rows(ref64["acts"].float(), c, other), words, lens=other, dbias=False)
    for k in ("hprev",) + GRAD_KEYS[c["cell"]][:-1]:
        assert same_bits(base[k][0], got[k][0]) and same_bits(base[k][2], got[k][2]), k
        assert float(got[k][1].abs().sum()) == 0.0, k + " of a sample of length 0 is zero"


# ----------------------------------------------------------------------------------------------------------------------------
# Refusals: every one a host-side return in front of the first launch - the error code, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------
def _refusal_call(L, a, entry, H=32, B=1, Tmax=2, width=3, ntoken=3, ninput=4, null=None, w_hh_skew=0):
    """A call of `entry` on zero operands with every output placed written=False; `null` names the operand passed as NULL."""
    lstm = entry in (FWD, GT, TFWD, TRAIN, BWD)
    G, NA = (4, 5) if lstm else (3, 4)
    Hs, Bs, Ts, Ks, Ns = max(H, 1), max(B, 1), max(Tmax, 1), max(ninput, 1), max(ntoken, 1)      # operand sizes of a refused call
    z = lambda *s, **kw: a.place_input(torch.zeros(*s), **kw)             # noqa: E731
    o = lambda *s: a.place_output(s, written=False)                       # noqa: E731
    r = dict(captions=a.place_input(torch.zeros(Bs, max(width, Ts), dtype=torch.int64)), cap_lens=a.place_input(_i32([1] * Bs)),
             emb=z(Ns, Ks), x=z(Bs, Ts, Ks), w_ih=z(2, G * Hs, Ks), w_hh=z(2, G * Hs, Hs, skew=w_hh_skew), b_ih=z(2, G * Hs),
             b_hh=z(2, G * Hs), b_hn=z(2, Hs), table=z(Ns, 2, G * Hs), acts_in=z(Bs, Ts, 2, NA, Hs), words_in=z(Bs, 2 * Hs, Ts),
             d_words=z(Bs, 2 * Hs, Ts), d_sent=z(Bs, 2 * Hs), gates_ws=o(Bs * Ts * 2 * G * Hs), acts=o(Bs, Ts, 2, NA, Hs),
             words_emb=o(Bs, 2 * Hs, Ts), sent_emb=o(Bs, 2 * Hs), table_out=o(Ns, 2, G * Hs), dgates=o(Bs, Ts, 2, G * Hs),
             dgh=o(Bs, Ts, 2, G * Hs), hprev=o(Bs, Ts, 2, Hs), dbias=o(2, 2, G * Hs))
    assert null is None or null in r
    p = lambda k: None if k == null else r[k].ptr                         # noqa: E731
    s = _stream()
    calls = {
        FWD: lambda: L.tgsr_bilstm_fwd(p("captions"), width, p("cap_lens"), B, Tmax, p("emb"), ntoken, ninput, p("w_ih"), p("w_hh"),
                                       p("b_ih"), p("b_hh"), H, p("gates_ws"), p("words_emb"), p("sent_emb"), s),
        GT: lambda: L.tgsr_lstm_gate_table(p("emb"), ntoken, ninput, p("w_ih"), p("b_ih"), p("b_hh"), H, p("table_out"), s),
        TFWD: lambda: L.tgsr_bilstm_table_fwd(p("captions"), width, p("cap_lens"), B, Tmax, p("table"), ntoken, p("w_hh"), H,
                                              p("words_emb"), p("sent_emb"), s),
        TRAIN: lambda: L.tgsr_bilstm_train_fwd(p("x"), p("cap_lens"), B, Tmax, ninput, p("w_ih"), p("w_hh"), p("b_ih"), p("b_hh"), H,
                                               p("gates_ws"), p("acts"), p("words_emb"), p("sent_emb"), s),
        BWD: lambda: L.tgsr_bilstm_bwd(p("cap_lens"), B, Tmax, H, p("w_hh"), p("acts_in"), p("words_in"), p("d_words"), p("d_sent"),
                                       p("dgates"), p("hprev"), p("dbias"), s),
        GGT: lambda: L.tgsr_gru_gate_table(p("emb"), ntoken, ninput, p("w_ih"), p("b_ih"), p("b_hh"), H, p("table_out"), s),
        GTFWD: lambda: L.tgsr_bigru_table_fwd(p("captions"), width, p("cap_lens"), B, Tmax, p("table"), ntoken, p("w_hh"), p("b_hn"), H,
                                              p("words_emb"), p("sent_emb"), s),
        GTRAIN: lambda: L.tgsr_bigru_train_fwd(p("x"), p("cap_lens"), B, Tmax, ninput, p("w_ih"), p("w_hh"), p("b_ih"), p("b_hh"),
                                               p("b_hn"), H, p("gates_ws"), p("acts"), p("words_emb"), p("sent_emb"), s),
        GBWD: lambda: L.tgsr_bigru_bwd(p("cap_lens"), B, Tmax, H, p("w_hh"), p("acts_in"), p("words_in"), p("d_words"), p("d_sent"),
                                       p("dgates"), p("dgh"), p("hprev"), p("dbias"), s),
    }
    return calls[entry]


# the operands each entry point refuses as NULL (d_sent and dbias of the backwards may be NULL: not here)
NULLS = {
    FWD: ("captions", "cap_lens", "emb", "w_ih", "w_hh", "b_ih", "b_hh", "gates_ws", "words_emb", "sent_emb"),
    GT: ("emb", "w_ih", "b_ih", "b_hh", "table_out"),
    TFWD: ("captions", "cap_lens", "table", "w_hh", "words_emb", "sent_emb"),
    TRAIN: ("x", "cap_lens", "w_ih", "w_hh", "b_ih", "b_hh", "gates_ws", "acts", "words_emb", "sent_emb"),
    BWD: ("cap_lens", "w_hh", "acts_in", "words_in", "d_words", "dgates", "hprev"),
    GGT: ("emb", "w_ih", "b_ih", "b_hh", "table_out"),
    GTFWD: ("captions", "cap_lens", "table", "w_hh", "b_hn", "words_emb", "sent_emb"),
    GTRAIN: ("x", "cap_lens", "w_ih", "w_hh", "b_ih", "b_hh", "b_hn", "gates_ws", "acts", "words_emb", "sent_emb"),
    GBWD: ("cap_lens", "w_hh", "acts_in", "words_in", "d_words", "dgates", "dgh", "hprev"),
}
# the sizes each entry point takes and refuses below 1 (TGSR_EINVAL); H < 1 of the backwards is "no instance" instead
SIZES = {
    FWD: ("B", "Tmax", "ntoken", "ninput", "H"), GT: ("ntoken", "ninput", "H"), TFWD: ("B", "Tmax", "ntoken", "H"),
    TRAIN: ("B", "Tmax", "ninput", "H"), BWD: ("B", "Tmax"), GGT: ("ntoken", "ninput", "H"), GTFWD: ("B", "Tmax", "ntoken", "H"),
    GTRAIN: ("B", "Tmax", "ninput", "H"), GBWD: ("B", "Tmax"),
}


def refusals():
    """(name, entry point, arguments of _refusal_call, code, whether tgsr_last_error names w_hh)."""
    out = []
    for e, names in NULLS.items():
        out += [("%s-%s-null" % (e[5:], n), e, dict(null=n), "EINVAL", False) for n in names]
    for e, names in SIZES.items():
        out += [("%s-%s-0" % (e[5:], n), e, {n: 0}, "EINVAL", False) for n in names]
    for e in (FWD, TFWD, GTFWD):
        out.append(("%s-Tmax-above-width" % e[5:], e, dict(Tmax=4, width=3), "EINVAL", False))
    for e in (FWD, TFWD, TRAIN):
        out += [("%s-H%d" % (e[5:], H), e, dict(H=H), "EUNSUPPORTED", False) for H in (257, 272, 24, 8)]
        out += [("%s-H%d-w_hh-unaligned" % (e[5:], H), e, dict(H=H, w_hh_skew=1), "EUNSUPPORTED", True) for H in (32, 64, 128)]
    for e in (GTFWD, GTRAIN):
        out += [("%s-H%d" % (e[5:], H), e, dict(H=H), "EUNSUPPORTED", False) for H in (16, 48, 256)]
        out += [("%s-H%d-w_hh-unaligned" % (e[5:], H), e, dict(H=H, w_hh_skew=1), "EUNSUPPORTED", True) for H in (32, 64, 128)]
    for e in (BWD, GBWD):
        out += [("%s-H%d" % (e[5:], H), e, dict(H=H), "EUNSUPPORTED", False) for H in (0, 16, 48, 256)]
    return out


def test_refusals():
    """Bad operands and sizes, shapes without an instance, and a w_hh the float4 instances cannot read: the code, and no word written."""
    M, L = _lib()
    for name, entry, kw, code, names_w_hh in refusals():
        a = Arena(DEV, guard=64)
        call = _refusal_call(L, a, entry, **kw)
        assert call() == getattr(M, code), name
        v = a.violations()
        assert not v, name + ": " + "; ".join(v)
        if names_w_hh:
            assert b"w_hh" in L.tgsr_last_error(), name
