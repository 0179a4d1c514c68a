"""GPU: the six entry points of the word-attention and DAMSM family held to their C ABI contract, called directly through ctypes.

    tgsr_word_attention_fwd   tgsr_word_project_fwd   tgsr_word_attention_bwd
    tgsr_damsm_words_fwd      tgsr_func_attention_fwd tgsr_damsm_words_bwd

tests/test_hip_parity.py and tests/test_hip_train.py reach them through tgsr_amd/ops.py only: B <= 16 and Q <= 4096 keep the forward's
grid below its cap (the tile loop never makes a second trip) and the backward at one pixel block per wave, every stride is passed
dense, no batch exceeds the 256 mask rows a workgroup caches, the projection runs at cdf = 256 and 64 alone, DAMSM at ndf in
{64, 128, 256}, and every workspace comes rounded up and recycled from the caching allocator.  Here every operand of a call is placed
in a guarded arena (tests/arena.py): workspaces of exactly the documented size prefilled with NaN, outputs prefilled with a pattern
no arithmetic produces, strided operands with NaN between their samples, guard bands around everything.  After the call the guard
bands, gaps and inputs must be untouched, every output word written and finite, the result within the suite's caps of the oracle's
own functions run in float64 (O.word_attention, O.func_attention, O.cosine_similarity are dtype-generic; torch autograd for the
backwards) - and a second call with the workspaces holding a finite constant instead of NaN must give the same bits.

TABLE has one row per (entry point, kernel instance or path), the dispatch condition copied from the extern "C" launcher; the tests
re-evaluate it (fwd_plan / bwd_plan / the host-callable planners tgsr_word_attention_bwd_chunks, tgsr_damsm_words_bwd_ws_elems).
Every caption length is >= 1 (asserted where the inputs are made), so no softmax row is fully masked.

Elementwise caps are the ones the suite already states for these operations (atol / rtol): attention map 5e-6 / 1e-4 and c_code
5e-5 / 1e-4 (test_word_attention_vs_oracle), the projection 2e-5 / 1e-5 (test_word_project_batched), sim 2e-5 / 1e-5 and att_diag
2e-6 / 1e-4 (test_damsm_similarity_vs_oracle; 1e-4 is its close()'s default), func_attention 2e-5 and 2e-6 / 1e-4
(test_func_attention_golden), DAMSM gradients 3e-5 max|ref| / 1e-3 (test_damsm_backward_vs_oracle_autograd), dh 5e-5 / 1e-3
(test_word_attention_backward).  d(src) had no fp64 cap; it and the other gradients carry the project's ratio bound (R_DIRECT /
R_WINO of tests/test_hip_train_abi.py): the kernel's mean distance from fp64 against the distance of the same oracle formula run by
torch on the CPU in fp32, R_* below.
"""
import ctypes
import functools

import pytest
import torch

from arena import Arena
from oracle import tgsr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAMMA1, GAMMA2 = 4.0, 5.0

# mean |kernel - f64| / mean |torch CPU fp32 - f64| over a case's gradient: 1.5 x the largest measured ratio of the group, rounded up
# to one decimal (__expf and the MFMA summation order make the ratio move with the shape; the rule of R_DIRECT / R_WINO in
# tests/test_hip_train_abi.py).  Measured on the MI355X over the four cases of each group (profiles/HISTORY.md).  A case whose CPU
# fp32 gradient IS the fp64 one (T = 1: dS = 0 exactly) must be exact on the device as well.
R_DH = 1.6                # measured 0.91 .. 1.01 (largest: Q = 8200, two blocks per wave)
R_DSRC = 1.8              # measured 0.92 .. 1.14 (largest: Q = 5, T = 1 - 32 sums of five products)
R_GWORDS = 2.3            # measured 0.93 .. 1.52 (largest: ndf = 256, Tw = 18, S = 289)
R_GCTX = 2.0              # measured 0.91 .. 1.32 (largest: the same case)

WAF, PROJ, WAB = "tgsr_word_attention_fwd", "tgsr_word_project_fwd", "tgsr_word_attention_bwd"
DF, FA, DB = "tgsr_damsm_words_fwd", "tgsr_func_attention_fwd", "tgsr_damsm_words_bwd"
CDF_MAX = 1024            # tgsr_word_attention_fwd with `words`: cdf * 128 bytes of LDS (include/tgsr_hip.h)


# ----------------------------------------------------------------------------------------------------------------------------
# Case fields.  Word attention: hextra / cextra = channels of the wider buffers h is a slice of / c_code is written into (h_bstride =
# (idf + hextra) Q), mode = mask_mode, mask / attn = operand given, nsets > 0: words == w_ctx == NULL and src_ws pre-filled by
# tgsr_word_project_fwd with that many weight sets (the last one attends), wskew = words the fused projection's w_ctx is placed off
# its 16-byte alignment.  DAMSM: lens = caption lengths (None: cap_lens == NULL), att = att_diag given.
# ----------------------------------------------------------------------------------------------------------------------------
def _wa(B, idf, Q, T, cdf, mode=0, mask=True, attn=True, hextra=0, cextra=0, nsets=0, wskew=0):
    return dict(B=B, idf=idf, Q=Q, T=T, cdf=cdf, mode=mode, mask=mask, attn=attn, hextra=hextra, cextra=cextra, nsets=nsets,
                wskew=wskew)


def _wb(B, idf, Q, T, mode=0, mask=True, hextra=0):
    return dict(B=B, idf=idf, Q=Q, T=T, mode=mode, mask=mask, hextra=hextra)


def _d(B, ndf, Tw, S, lens=None, att=True):
    assert lens is None or (len(lens) == B and all(1 <= n <= Tw for n in lens))
    return dict(B=B, ndf=ndf, Tw=Tw, S=S, lens=lens, att=att)


_A = "word_attention_kernel<%d>"             # <NI = idf / 32>
_B = "word_attention_bwd_kernel<%d>"
TABLE = [
    # entry point, kernel instance / path, dispatch condition, case (None: not covered, the condition says why)
    (WAF, "word_project_kernel (scalar tail) + " + _A % 1, "idf == 32, words given, cdf % 4 != 0; two tiles with a short last one, "
     "waves 2 and 3 exit early; h and c_code channel slices", _wa(2, 32, 40, 5, 37, hextra=8, cextra=3)),
    (WAF, "word_project_kernel (float4) + " + _A % 2, "idf == 64, cdf % 4 == 0 and w_ctx 16-byte aligned; Q < 32, T = 1, mask == NULL, "
     "attn == NULL", _wa(3, 64, 5, 1, 64, mask=False, attn=False)),
    (WAF, "word_project_kernel (float4, > 64 KB of LDS) + " + _A % 4, "idf == 128, cdf == 1024 (the limit: the LDS opt-in), T == 32 "
     "(valid = all ones), mask_mode 1", _wa(1, 128, 289, 32, CDF_MAX, mode=1)),
    (WAF, "word_project_kernel (scalar: w_ctx not 16-byte aligned) + " + _A % 1, "cdf % 4 == 0 but w_ctx % 16 == 4",
     _wa(2, 32, 40, 5, 64, wskew=1)),
    (WAF, _A % 1 + ", capped grid", "B > 256 and gx > cap = ceil(1024 / B): second trip of the tile loop, the ragged tile on that trip, "
     "mask rows >= 256 from global memory; mask_mode 0", _wa(257, 32, 520, 7, 20)),
    (WAF, _A % 1 + ", capped grid", "... mask_mode 1", _wa(257, 32, 520, 7, 20, mode=1)),
    (PROJ, "word_project_mfma_kernel + " + _A % 1, "words == w_ctx == NULL: src_ws read; nsets = 1, odd cdf",
     _wa(2, 32, 40, 5, 37, nsets=1, hextra=8)),
    (PROJ, "word_project_mfma_kernel + " + _A % 2, "words == w_ctx == NULL; nsets = 4, idf = 64 (two channel blocks per set)",
     _wa(3, 64, 40, 7, 100, nsets=4, mode=1)),
    (WAF, "word_project_kernel above 128 KB", "cdf > 1024: refused (test_refusals)", None),
    (WAB, _B % 1, "idf == 32; two chunks, blocks_per_wave 1, waves 1-3 of the second chunk empty (zero slabs); h a channel slice",
     _wb(2, 32, 130, 5, hextra=8)),
    (WAB, _B % 2, "idf == 64; Q > 8192: 64 chunks, blocks_per_wave == 2, ragged last block, T == 32, mask_mode 1",
     _wb(1, 64, 8200, 32, mode=1)),
    (WAB, _B % 1, "B > 256: mask rows >= 256 from global memory; mask_mode 0", _wb(257, 32, 33, 3)),
    (WAB, _B % 1, "Q < 32, T = 1, mask == NULL", _wb(1, 32, 5, 1, mask=False)),
    (WAB, "idf == 128", "no instance: refused (test_refusals)", None),
    (DF, "damsm_pair_kernel GRID", "ndf == 32 (phase C leaves three waves without a feature block), Tw = 1, cap_lens == NULL",
     _d(2, 32, 1, 5)),
    (DF, "damsm_pair_kernel GRID", "... S = 1", _d(2, 32, 1, 1)),
    (DF, "damsm_pair_kernel GRID", "the limits: ndf == 512 (140 KB of LDS), Tw == 32, S == 320", _d(2, 512, 32, 320, lens=[32, 1])),
    (DF, "damsm_pair_kernel GRID", "ndf no power of two, a region block of one region, att_diag == NULL",
     _d(3, 96, 7, 33, lens=[7, 3, 1], att=False)),
    (DF, "damsm_pair_kernel GRID", "the workload's own shape", _d(2, 256, 18, 289, lens=[18, 11])),
    (FA, "damsm_pair_kernel PAIRED", "ndf == 32, L = 1, S = 1", _d(2, 32, 1, 1)),
    (FA, "damsm_pair_kernel PAIRED", "ndf no power of two, odd L and S", _d(3, 160, 9, 65)),
    (FA, "damsm_pair_kernel PAIRED", "the limits", _d(1, 512, 32, 320)),
    (DB, "damsm_pair_bwd_kernel", "ndf == 32: seven of the eight (d, half) waves idle", _d(2, 32, 1, 5)),
    (DB, "damsm_pair_bwd_kernel", "ndf == 96: `dok` cuts a wave", _d(3, 96, 7, 33, lens=[7, 3, 1])),
    (DB, "damsm_pair_bwd_kernel", "ndf == 160, cap_lens == NULL", _d(3, 160, 9, 65)),
    (DB, "damsm_pair_bwd_kernel", "ndf == 256 (the limit), the workload's own shape", _d(2, 256, 18, 289, lens=[18, 11])),
    (DB, "ndf > 256", "the backward stops at 256: refused (test_refusals)", None),
]


def _rows(*entries):
    return [r for r in TABLE if r[0] in entries and r[3] is not None]


def row_id(r):
    c = r[3]
    if r[0] in (WAF, PROJ):
        return "%s-B%d-idf%d-Q%d-T%d-cdf%d-m%s%s%s%s" % (r[0][5:], c["B"], c["idf"], c["Q"], c["T"], c["cdf"],
                                                        c["mode"] if c["mask"] else "none", "" if c["attn"] else "-noattn",
                                                        "-sets%d" % c["nsets"] if c["nsets"] else "", "-skew" if c["wskew"] else "")
    if r[0] == WAB:
        return "%s-B%d-idf%d-Q%d-T%d-m%s" % (r[0][5:], c["B"], c["idf"], c["Q"], c["T"], c["mode"] if c["mask"] else "none")
    return "%s-B%d-ndf%d-T%d-S%d%s%s" % (r[0][5:], c["B"], c["ndf"], c["Tw"], c["S"], "" if c["lens"] else "-nolens",
                                        "" if c["att"] else "-noatt")


# ----------------------------------------------------------------------------------------------------------------------------
# The launchers' arithmetic, restated
# ----------------------------------------------------------------------------------------------------------------------------
def fwd_plan(c):
    """tgsr_word_attention_fwd: gx = min(ceil(Q / 128), ceil(1024 / B)) workgroups of four waves per sample, wave w of workgroup x
    walks the 32-pixel tiles 4 x + w, + 4 gx, ..."""
    B, Q = c["B"], c["Q"]
    want, cap = -(-Q // 128), -(-1024 // B)
    gx, ntiles = min(want, cap), -(-Q // 32)
    first = [4 * x + w for x in range(gx) for w in range(4)]
    return dict(want=want, cap=cap, gx=gx, ntiles=ntiles, stride=4 * gx, idle=[t for t in first if t >= ntiles],
                trips=max(len(range(t, ntiles, 4 * gx)) for t in first), ragged=Q % 32 != 0,
                ragged_on_second_trip=Q % 32 != 0 and ntiles - 1 >= 4 * gx, instance=_A % (c["idf"] // 32))


def bwd_plan(c, chunks):
    """tgsr_word_attention_bwd: `chunks` workgroups of four waves per sample, wave k (of 4 chunks) owns the pixel blocks
    [k bpw, (k + 1) bpw)."""
    nblk = -(-c["Q"] // 32)
    bpw = -(-nblk // (4 * chunks))
    empty = [k for k in range(4 * chunks) if k * bpw >= nblk]
    return dict(chunks=chunks, nblk=nblk, bpw=bpw, empty=empty, instance=_B % (c["idf"] // 32))


def damsm_ws_elems(c):
    return c["B"] * c["B"] * (3 * 32 * c["S"] + c["ndf"] * 32 + c["ndf"] * c["S"])


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs and references (CPU; computed once per case and shared)
# ----------------------------------------------------------------------------------------------------------------------------
def _key(c):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in c.items()))


def _mask_of(B, T, g):
    """bool [B][T], True = padded word: caption lengths 1 .. T, the first full; with B > 256 the rows from 256 on hold a pattern no
    length gives (word 0 kept, word 1 padded, the last word kept), so they differ from every row a workgroup caches."""
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    mask = torch.arange(T)[None, :] >= lens[:, None]
    if B > 256:
        assert T >= 3
        mask[256:] = False
        mask[256:, 1] = True
        assert all(bool((mask[r] != mask[:256]).any(1).all()) for r in range(256, B))
    assert bool((~mask).any(1).all()), "a fully masked row"
    return mask


@functools.lru_cache(maxsize=None)
def _wa_inputs(key):
    c = dict(key)
    B, idf, Q, T, cdf = c["B"], c["idf"], c["Q"], c["T"], c["cdf"]
    g = torch.Generator().manual_seed(B + 3 * idf + 5 * Q + 7 * T + 11 * cdf + c["mode"])
    h = torch.randn(B, idf, Q, generator=g)
    words = torch.randn(B, cdf, T, generator=g)
    ws = [torch.randn(idf, cdf, generator=g) / cdf ** 0.5 for _ in range(max(1, c["nsets"]))]
    mask = _mask_of(B, T, g) if c["mask"] else None
    return h, words, ws, mask


def wa_inputs(c):
    return _wa_inputs(_key(c))


def wa_reference(c, h, words, w, mask, dtype=torch.float64):
    """(c_code [B][idf][Q], attn [B][T][Q], src [B][idf][T]) by the oracle in `dtype`."""
    B, idf, Q, T = c["B"], c["idf"], c["Q"], c["T"]
    out, attn = O.word_attention(h.to(dtype).reshape(B, idf, 1, Q), words.to(dtype), w.to(dtype).reshape(idf, -1, 1, 1), mask,
                                 correct_mask=bool(c["mode"]))
    src = torch.einsum("ic,bct->bit", w.to(dtype), words.to(dtype))
    return out.reshape(B, idf, Q), attn.reshape(B, T, Q), src


@functools.lru_cache(maxsize=None)
def _wa_refs(key):
    c = dict(key)
    h, words, ws, mask = _wa_inputs(key)
    return wa_reference(c, h, words, ws[-1], mask)


def wa_refs(c):
    return _wa_refs(_key(c))


@functools.lru_cache(maxsize=None)
def _wb_inputs(key):
    c = dict(key)
    B, idf, Q, T = c["B"], c["idf"], c["Q"], c["T"]
    g = torch.Generator().manual_seed(2 * B + 3 * idf + 5 * Q + 7 * T + c["mode"])
    h = torch.randn(B, idf, Q, generator=g)
    src = torch.randn(B, idf, T, generator=g)              # unit-scale projected words, as w_ctx / sqrt(cdf) gives them
    dc = torch.randn(B, idf, Q, generator=g)
    mask = _mask_of(B, T, g) if c["mask"] else None
    return h, src, dc, mask


def wb_inputs(c):
    return _wb_inputs(_key(c))


def wb_reference(c, h, src, dc, mask, dtype=torch.float64):
    """(dh [B][idf][Q], dsrc [B][idf][T]) by torch autograd through O.word_attention in `dtype`; the projection is the identity
    (cdf = idf), so the words ARE src."""
    B, idf, Q = c["B"], c["idf"], c["Q"]
    hr, sr = h.to(dtype).reshape(B, idf, 1, Q).clone().requires_grad_(), src.to(dtype).clone().requires_grad_()
    out, _ = O.word_attention(hr, sr, torch.eye(idf, dtype=dtype).reshape(idf, idf, 1, 1), mask, correct_mask=bool(c["mode"]))
    out.backward(dc.to(dtype).reshape(B, idf, 1, Q))
    return hr.grad.reshape(B, idf, Q), sr.grad


@functools.lru_cache(maxsize=None)
def _wb_refs(key):
    c = dict(key)
    i = _wb_inputs(key)
    return wb_reference(c, *i), wb_reference(c, *i, dtype=torch.float32)


def wb_refs(c):
    """((dh, dsrc) in fp64, the same in fp32)."""
    return _wb_refs(_key(c))


@functools.lru_cache(maxsize=None)
def _d_inputs(key):
    c = dict(key)
    B, ndf, Tw, S = c["B"], c["ndf"], c["Tw"], c["S"]
    g = torch.Generator().manual_seed(B + 3 * ndf + 5 * Tw + 7 * S)
    return torch.randn(B, ndf, Tw, generator=g), torch.randn(B, ndf, S, generator=g), torch.randn(B, B, generator=g)


def d_inputs(c):
    """(words [B][ndf][Tw], ctx [B][ndf][S], grad_sim [B][B])."""
    return _d_inputs(_key(c))


def d_lens(c):
    return list(c["lens"]) if c["lens"] else [c["Tw"]] * c["B"]


def damsm_reference(c, words, ctx, gsim=None, lens=None, dtype=torch.float64):
    """sim [B img][B cap] and att_diag [B][Tw][S] by the oracle's per-caption loop (words_loss) in `dtype`; with gsim also
    (grad_words [B][ndf][Tw], grad_ctx [B][ndf][S]) of (sim * gsim).sum() by torch autograd."""
    B, ndf, Tw, S = c["B"], c["ndf"], c["Tw"], c["S"]
    lens = d_lens(c) if lens is None else lens
    assert all(1 <= n <= Tw for n in lens)
    wr, cr = words.to(dtype).clone().requires_grad_(gsim is not None), ctx.to(dtype).clone().requires_grad_(gsim is not None)
    cols, att = [], torch.zeros(B, Tw, S, dtype=dtype)
    for i, n in enumerate(lens):
        word = wr[i:i + 1, :, :n].expand(B, -1, -1)
        wc, attn = O.func_attention(word, cr.reshape(B, ndf, 1, S), GAMMA1)
        att[i, :n] = attn[i].reshape(n, S).detach()
        row = O.cosine_similarity(word.transpose(1, 2).reshape(B * n, -1), wc.transpose(1, 2).reshape(B * n, -1))
        cols.append(torch.log(torch.exp(row.reshape(B, n) * GAMMA2).sum(1)))
    sim = torch.stack(cols, 1)
    if gsim is None:
        return sim.detach(), att
    (sim * gsim.to(dtype)).sum().backward()
    return sim.detach(), att, wr.grad, cr.grad


@functools.lru_cache(maxsize=None)
def _d_refs(key):
    c = dict(key)
    words, ctx, gsim = _d_inputs(key)
    return damsm_reference(c, words, ctx, gsim), damsm_reference(c, words, ctx, gsim, dtype=torch.float32)


def d_refs(c):
    """((sim, att_diag, grad_words, grad_ctx) in fp64, the same in fp32)."""
    return _d_refs(_key(c))


def fa_reference(c, query, ctx, dtype=torch.float64):
    wc, attn = O.func_attention(query.to(dtype), ctx.to(dtype).reshape(c["B"], c["ndf"], 1, c["S"]), GAMMA1)
    return wc, attn.reshape(c["B"], c["Tw"], c["S"])


# elementwise caps (atol, rtol): see the module docstring for where the suite states each
TOL_ATTN, TOL_CCODE, TOL_SRC = (5e-6, 1e-4), (5e-5, 1e-4), (2e-5, 1e-5)
TOL_SIM, TOL_ATT_DIAG, TOL_FA_WC, TOL_FA_ATTN = (2e-5, 1e-5), (2e-6, 1e-4), (2e-5, 1e-4), (2e-6, 1e-4)
TOL_DH = (5e-5, 1e-3)


def damsm_grad_tol(ref):
    return 3e-5 * float(ref.abs().max()), 1e-3


def close(got, ref, tol, what=""):
    atol, rtol = tol
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d of %d values beyond atol %.3g rtol %.3g, worst |err| %.3g at |ref| %.3g" % (
        what, int(bad.sum()), bad.numel(), atol, rtol, float(err.max()), float(ref.abs().flatten()[int(err.argmax())]))


def ratio_ok(tag, name, got, ref64, ref32, bound):
    own, cpu = float((got.double() - ref64).abs().mean()), float((ref32.double() - ref64).abs().mean())
    print("GRAD_RATIO %s %s own %.4g cpu %.4g ratio %s max|err| %.4g" % (
        tag, name, own, cpu, "%.3f" % (own / cpu) if cpu else "-", float((got.double() - ref64).abs().max())))
    if cpu == 0.0:
        assert own == 0.0, "%s: the CPU fp32 gradient is exact, the kernel's is %.3g off" % (name, own)
    else:
        assert own <= bound * cpu, "%s: mean |kernel - f64| = %.3g is %.2f x the CPU fp32 gradient's %.3g (bound %.1f)" % (
            name, own, own / cpu, cpu, bound)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    from tgsr_amd import ops
    return ops._stream()


def _p(r):
    return r.ptr if r is not None else None


def _u8(mask):
    return None if mask is None else mask.to(torch.uint8)


def _twice(a, call, outs, M):
    """The call on NaN workspaces, then on workspaces holding 1.0: the arena's contract both times, the same bits; returns the outputs."""
    assert call() == M.OK
    a.check()
    got = [o.read() for o in outs]
    a.rearm(ws_fill=1.0)
    assert call() == M.OK
    a.check()
    for g, o in zip(got, outs):
        assert same_bits(g, o.read()), "the result depends on what the workspace held"
    return got


# ----------------------------------------------------------------------------------------------------------------------------
# Word attention, forward
# ----------------------------------------------------------------------------------------------------------------------------
def _project(M, L, c, words, ws):
    """tgsr_word_project_fwd in an arena of its own: src_out [nsets][B][idf][32]."""
    B, idf, T, cdf, n = c["B"], c["idf"], c["T"], c["cdf"], len(ws)
    a = Arena(DEV)
    wd = a.place_input(words)
    wr = [a.place_input(w) for w in ws]
    out = a.place_output((n, B, idf, 32))
    ptrs = (ctypes.c_void_p * n)(*[r.address for r in wr])

    def call():
        return L.tgsr_word_project_fwd(wd.ptr, ptrs, n, B, idf, cdf, T, out.ptr, _stream())
    src = _twice(a, call, [out], M)[0]
    for k, w in enumerate(ws):
        ref = torch.einsum("ic,bct->bit", w.double(), words.double())
        close(src[k, :, :, :T], ref, TOL_SRC, "src of set %d" % k)
        assert T == 32 or float(src[k, :, :, T:].abs().max()) == 0.0, "words >= T of the projection are zero"
    return src


def _wa_forward(M, L, c):
    """One tgsr_word_attention_fwd case in an arena of its own: (c_code, attn, src [B][idf][32] as the attention read it)."""
    B, idf, Q, T, cdf = c["B"], c["idf"], c["Q"], c["T"], c["cdf"]
    h, words, ws, mask = wa_inputs(c)
    hbs, cbs = (idf + c["hextra"]) * Q, (idf + c["cextra"]) * Q
    a = Arena(DEV)
    hr = a.place_input(h, bstride=hbs)
    mr = a.place_input(_u8(mask)) if c["mask"] else None
    if c["nsets"]:
        src = _project(M, L, c, words, ws)[-1]
        wdr = wr = None
        sr = a.place_input(src)                              # read-only here: the call must not write it
    else:
        wdr, wr = a.place_input(words), a.place_input(ws[0], skew=c["wskew"])
        sr = a.place_ws(B * idf * 32)
    cc = a.place_output((B, idf, Q), bstride=cbs)
    at = a.place_output((B, T, Q), written=c["attn"])
    assert wr is None or wr.address % 16 == 4 * c["wskew"]

    def call():
        return L.tgsr_word_attention_fwd(hr.ptr, hbs, _p(wdr), _p(wr), _p(mr), c["mode"], B, idf, cdf, T, Q, sr.ptr, cc.ptr, cbs,
                                         at.ptr if c["attn"] else None, _stream())
    got_c, got_a = _twice(a, call, [cc, at], M)
    return got_c, got_a, sr.read().reshape(B, idf, 32)


@pytest.mark.parametrize("row", _rows(WAF, PROJ), ids=row_id)
def test_word_attention_fwd_entry_point(row):
    _entry, instance, _cond, c = row
    M, L = _lib()
    B, Q, T = c["B"], c["Q"], c["T"]
    mask = wa_inputs(c)[3]
    ref_c, ref_a, ref_src = wa_refs(c)
    assert fwd_plan(c)["instance"] in instance
    got_c, got_a, src = _wa_forward(M, L, c)
    if not c["nsets"]:
        close(src[:, :, :T], ref_src, TOL_SRC, "src_ws")
        assert T == 32 or float(src[:, :, T:].abs().max()) == 0.0
    if c["wskew"]:                                           # the scalar stream gives the bits of the float4 stream (include/tgsr_hip.h)
        al_c, al_a, al_src = _wa_forward(M, L, dict(c, wskew=0))
        assert same_bits(src, al_src) and same_bits(got_c, al_c) and same_bits(got_a, al_a)
    close(got_c, ref_c, TOL_CCODE, "c_code")
    if c["attn"]:
        close(got_a, ref_a, TOL_ATTN, "attn")
        close(got_a.sum(1), torch.ones(B, Q), (1e-5, 0.0), "attention summed over the words")
        if mask is not None:                                 # a padded word of the row a pixel was masked with gets exactly zero
            rows = torch.arange(B)[:, None].expand(B, Q) if c["mode"] else (torch.arange(B * Q) % B).reshape(B, Q)
            assert float(got_a[mask[rows].permute(0, 2, 1)].abs().max() if bool(mask.any()) else 0.0) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------
# Word attention, backward
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", _rows(WAB), ids=row_id)
def test_word_attention_bwd_entry_point(row):
    _entry, instance, cond, c = row
    M, L = _lib()
    B, idf, Q, T = c["B"], c["idf"], c["Q"], c["T"]
    h, src, dc, mask = wb_inputs(c)
    (dh64, ds64), (dh32, ds32) = wb_refs(c)
    nch = L.tgsr_word_attention_bwd_chunks(Q)
    plan = bwd_plan(c, nch)
    assert plan["instance"] == instance
    if "blocks_per_wave == 2" in cond:
        assert nch == 64 and plan["bpw"] == 2 and Q % 32 != 0
    hbs = (idf + c["hextra"]) * Q
    src32 = torch.zeros(B, idf, 32)
    src32[:, :, :T] = src
    a = Arena(DEV)
    hr, sr, dr = a.place_input(h, bstride=hbs), a.place_input(src32), a.place_input(dc)
    mr = a.place_input(_u8(mask)) if c["mask"] else None
    dh, part = a.place_output((B, idf, Q)), a.place_output((B, nch, idf, 32))

    def call():
        return L.tgsr_word_attention_bwd(hr.ptr, hbs, sr.ptr, _p(mr), c["mode"], B, idf, T, Q, dr.ptr, dh.ptr, part.ptr, _stream())
    got_dh, got_part = _twice(a, call, [dh, part], M)          # check(): every slab written, the empty waves' included
    assert T == 32 or float(got_part[..., T:].abs().max()) == 0.0, "dsrc_part[..., t >= T] is exactly zero"
    for k in plan["empty"]:
        if k % 4 == 0:                                         # a chunk whose four waves are all empty: a zero slab
            assert float(got_part[:, k // 4].abs().max()) == 0.0
    got_ds = got_part.double().sum(1)[:, :, :T]                # the caller's sum over the chunks, here without rounding
    close(got_dh, dh64, TOL_DH, "dh")
    ratio_ok(row_id(row), "dh", got_dh, dh64, dh32, R_DH)
    ratio_ok(row_id(row), "dsrc", got_ds, ds64, ds32, R_DSRC)


# ----------------------------------------------------------------------------------------------------------------------------
# DAMSM forward, func_attention, DAMSM backward
# ----------------------------------------------------------------------------------------------------------------------------
def _damsm_fwd(M, L, c, lens):
    """One tgsr_damsm_words_fwd case in an arena of its own, caption lengths `lens` (None: cap_lens == NULL): (sim, att_diag | None)."""
    B, ndf, Tw, S = c["B"], c["ndf"], c["Tw"], c["S"]
    words, ctx, _ = d_inputs(c)
    a = Arena(DEV)
    wr, cr = a.place_input(words), a.place_input(ctx)
    lr = a.place_input(torch.tensor(lens, dtype=torch.int32)) if lens is not None else None
    sim, att = a.place_output((B, B)), a.place_output((B, Tw, S), written=c["att"])

    def call():
        return L.tgsr_damsm_words_fwd(wr.ptr, _p(lr), cr.ptr, B, ndf, Tw, S, GAMMA1, GAMMA2, sim.ptr, att.ptr if c["att"] else None,
                                      _stream())
    got = _twice(a, call, [sim, att], M)
    return got[0], got[1] if c["att"] else None


@pytest.mark.parametrize("row", _rows(DF), ids=row_id)
def test_damsm_words_fwd_entry_point(row):
    c = row[3]
    M, L = _lib()
    sim, att = _damsm_fwd(M, L, c, c["lens"])
    (sim64, att64, _gw, _gc), _ = d_refs(c)
    close(sim, sim64, TOL_SIM, "sim")
    if c["att"]:
        close(att, att64, TOL_ATT_DIAG, "att_diag")
        for i, n in enumerate(d_lens(c)):
            assert n == c["Tw"] or float(att[i, n:].abs().max()) == 0.0, "att_diag rows >= cap_lens[i] are zero"


def test_damsm_words_fwd_clamps_a_length_outside_1_to_Tw():
    M, L = _lib()
    c = _d(3, 96, 7, 33, lens=[7, 3, 1])
    sim, att = _damsm_fwd(M, L, c, [7, 3, 1])
    sim2, att2 = _damsm_fwd(M, L, c, [40, 3, 0])               # 40 -> Tw = 7, 0 -> 1 (include/tgsr_hip.h)
    assert same_bits(sim, sim2) and same_bits(att, att2)
    sim3, _ = _damsm_fwd(M, L, c, [7, 3, -5])
    assert same_bits(sim, sim3)


@pytest.mark.parametrize("row", _rows(FA), ids=row_id)
def test_func_attention_fwd_entry_point(row):
    c = row[3]
    M, L = _lib()
    B, ndf, Lq, S = c["B"], c["ndf"], c["Tw"], c["S"]
    query, ctx, _ = d_inputs(c)
    a = Arena(DEV)
    qr, cr = a.place_input(query), a.place_input(ctx)
    wc, attn = a.place_output((B, ndf, Lq)), a.place_output((B, Lq, S))

    def call():
        return L.tgsr_func_attention_fwd(qr.ptr, cr.ptr, B, ndf, Lq, S, GAMMA1, wc.ptr, attn.ptr, _stream())
    got_wc, got_attn = _twice(a, call, [wc, attn], M)
    ref_wc, ref_attn = fa_reference(c, query, ctx)
    close(got_attn, ref_attn, TOL_FA_ATTN, "attn")
    close(got_wc, ref_wc, TOL_FA_WC, "weighted_context")


def _damsm_bwd(M, L, c, lens):
    """One tgsr_damsm_words_bwd case in an arena of its own, an exact workspace: (grad_words32 [B][ndf][32], grad_ctx)."""
    B, ndf, Tw, S = c["B"], c["ndf"], c["Tw"], c["S"]
    words, ctx, gsim = d_inputs(c)
    n = L.tgsr_damsm_words_bwd_ws_elems(B, ndf, S)
    assert n == damsm_ws_elems(c)
    a = Arena(DEV)
    wr, cr, gr = a.place_input(words), a.place_input(ctx), a.place_input(gsim)
    lr = a.place_input(torch.tensor(lens, dtype=torch.int32)) if lens is not None else None
    ws, gw, gc = a.place_ws(n), a.place_output((B, ndf, 32)), a.place_output((B, ndf, S))

    def call():
        return L.tgsr_damsm_words_bwd(wr.ptr, _p(lr), cr.ptr, gr.ptr, B, ndf, Tw, S, GAMMA1, GAMMA2, ws.ptr, gw.ptr, gc.ptr, _stream())
    return _twice(a, call, [gw, gc], M)                        # check(): all 32 words of grad_words32 written and finite


def test_damsm_words_bwd_clamps_a_length_outside_1_to_Tw():
    M, L = _lib()
    c = _d(3, 96, 7, 33, lens=[7, 3, 1])
    gw, gc = _damsm_bwd(M, L, c, [7, 3, 1])
    gw2, gc2 = _damsm_bwd(M, L, c, [40, 3, 0])                 # 40 -> Tw = 7, 0 -> 1 (include/tgsr_hip.h)
    assert same_bits(gw, gw2) and same_bits(gc, gc2)


@pytest.mark.parametrize("row", _rows(DB), ids=row_id)
def test_damsm_words_bwd_entry_point(row):
    c = row[3]
    M, L = _lib()
    Tw = c["Tw"]
    (_s, _a, gw64, gc64), (_s32, _a32, gw32, gc32) = d_refs(c)
    got_gw, got_gc = _damsm_bwd(M, L, c, c["lens"])
    for i, ln in enumerate(d_lens(c)):                          # the contract: zero behind the caption, up to Tw
        if ln < Tw:
            assert float(got_gw[i, :, ln:Tw].abs().max()) == 0.0, "grad_words32[i][:, len_i:Tw] is zero"
    close(got_gw[:, :, :Tw], gw64, damsm_grad_tol(gw64), "grad_words")
    close(got_gc, gc64, damsm_grad_tol(gc64), "grad_ctx")
    ratio_ok(row_id(row), "grad_words", got_gw[:, :, :Tw], gw64, gw32, R_GWORDS)
    ratio_ok(row_id(row), "grad_ctx", got_gc, gc64, gc32, R_GCTX)


# ----------------------------------------------------------------------------------------------------------------------------
# Refusals: the error code, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------
def _refuse_wa_fwd(L, a, B=1, idf=32, cdf=8, T=3, Q=5, words=True, w_ctx=True):
    f = lambda *s: a.place_input(torch.zeros(*s))            # noqa: E731
    h, wd, w = f(B, idf, Q), f(B, cdf, T), f(idf, cdf)
    src, cc, at = (a.place_output(s, written=False) for s in ((B, idf, 32), (B, idf, Q), (B, T, Q)))
    return lambda: L.tgsr_word_attention_fwd(h.ptr, idf * Q, wd.ptr if words else None, w.ptr if w_ctx else None, None, 0, B, idf, cdf,
                                             T, Q, src.ptr, cc.ptr, idf * Q, at.ptr, _stream())


def _refuse_wa_bwd(L, a, idf):
    B, T, Q = 1, 3, 5
    f = lambda *s: a.place_input(torch.zeros(*s))            # noqa: E731
    h, src, dc = f(B, idf, Q), f(B, idf, 32), f(B, idf, Q)
    dh, part = a.place_output((B, idf, Q), written=False), a.place_output((B, 1, idf, 32), written=False)
    return lambda: L.tgsr_word_attention_bwd(h.ptr, idf * Q, src.ptr, None, 0, B, idf, T, Q, dc.ptr, dh.ptr, part.ptr, _stream())


def _refuse_damsm_fwd(L, a, ndf=32, Tw=3, S=5, sim=True):
    B = 1
    wd, cx = a.place_input(torch.zeros(B, ndf, Tw)), a.place_input(torch.zeros(B, ndf, S))
    sm, at = a.place_output((B, B), written=False), a.place_output((B, Tw, S), written=False)
    return lambda: L.tgsr_damsm_words_fwd(wd.ptr, None, cx.ptr, B, ndf, Tw, S, GAMMA1, GAMMA2, sm.ptr if sim else None, at.ptr, _stream())


def _refuse_fa(L, a):
    B, ndf, Lq, S = 1, 32, 3, 5
    q, cx = a.place_input(torch.zeros(B, ndf, Lq)), a.place_input(torch.zeros(B, ndf, S))
    wc, at = a.place_output((B, ndf, Lq), written=False), a.place_output((B, Lq, S), written=False)
    return lambda: L.tgsr_func_attention_fwd(q.ptr, cx.ptr, B, ndf, Lq, S, GAMMA1, wc.ptr, None, _stream()), at


def _refuse_damsm_bwd(L, a, ndf):
    B, Tw, S = 1, 3, 5
    wd, cx, gs = a.place_input(torch.zeros(B, ndf, Tw)), a.place_input(torch.zeros(B, ndf, S)), a.place_input(torch.zeros(B, B))
    ws = a.place_output((B * B * (96 * S + ndf * 32 + ndf * S),), written=False)
    gw, gc = a.place_output((B, ndf, 32), written=False), a.place_output((B, ndf, S), written=False)
    return lambda: L.tgsr_damsm_words_bwd(wd.ptr, None, cx.ptr, gs.ptr, B, ndf, Tw, S, GAMMA1, GAMMA2, ws.ptr, gw.ptr, gc.ptr, _stream())


REFUSALS = [
    ("word_attention_fwd-T33", lambda L, a: _refuse_wa_fwd(L, a, T=33), "EUNSUPPORTED"),
    ("word_attention_fwd-idf96", lambda L, a: _refuse_wa_fwd(L, a, idf=96), "EUNSUPPORTED"),
    ("word_attention_fwd-cdf%d" % (CDF_MAX + 1), lambda L, a: _refuse_wa_fwd(L, a, cdf=CDF_MAX + 1), "EUNSUPPORTED"),
    ("word_attention_fwd-words-without-w_ctx", lambda L, a: _refuse_wa_fwd(L, a, w_ctx=False), "EINVAL"),
    ("word_attention_bwd-idf128", lambda L, a: _refuse_wa_bwd(L, a, 128), "EUNSUPPORTED"),
    ("damsm_words_fwd-ndf48", lambda L, a: _refuse_damsm_fwd(L, a, ndf=48), "EUNSUPPORTED"),
    ("damsm_words_fwd-ndf544", lambda L, a: _refuse_damsm_fwd(L, a, ndf=544), "EUNSUPPORTED"),
    ("damsm_words_fwd-Tw33", lambda L, a: _refuse_damsm_fwd(L, a, Tw=33), "EUNSUPPORTED"),
    ("damsm_words_fwd-S321", lambda L, a: _refuse_damsm_fwd(L, a, S=321), "EUNSUPPORTED"),
    ("damsm_words_fwd-sim-null", lambda L, a: _refuse_damsm_fwd(L, a, sim=False), "EINVAL"),
    ("func_attention_fwd-attn-null", lambda L, a: _refuse_fa(L, a)[0], "EINVAL"),
    ("damsm_words_bwd-ndf288", lambda L, a: _refuse_damsm_bwd(L, a, 288), "EUNSUPPORTED"),
]


@pytest.mark.parametrize("name,make,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, make, code):
    M, L = _lib()
    a = Arena(DEV)
    call = make(L, a)
    assert call() == getattr(M, code)
    a.check()                                                  # every output was placed written=False: untouched
