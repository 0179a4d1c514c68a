"""GPU: the bf16 / f16 inference kernels held to their C ABI contract, called directly through ctypes.

    tgsr_lp_from_nchw / _to_nchw / _convert          tgsr_lp_pack_conv3x3_weight / _pack_upconv_weight / _pack_to3_weight
    tgsr_lp_conv3x3_fwd                              tgsr_lp_upconv_glu_fwd / _head_fwd / _att_fwd
    tgsr_lp_head_combine / _combine_map              tgsr_lp_stem_fwd / _stem_att_fwd
    tgsr_lp_conv_to3_fwd / _map_fwd                  tgsr_lp_word_attention_fwd          tgsr_text_tail_lp_fwd
    tgsr_lp_resblocks_fwd: its refusals only (see the table)

tests/test_hip_lp.py and tests/test_hip_lp_forms.py reach these kernels through tgsr_amd.lp / ops: zero-filled buffers from torch,
an fp32 CPU model as the reference, one whole ulp of the storage type as the tolerance.  Here every operand of a call lives in a
guarded arena (tests/arena.py): an lp image holds zeros on its border, a NaN pattern in every channel the call neither reads nor
writes and in the channels it has to write, and afterwards the border, the foreign channels, the inputs and the guard bands hold
their bits while the written range holds no pattern and only finite values.  Every launched case runs twice, the second time with
the outputs of 2-byte elements refilled with a finite constant: the two results are the same bits.

The reference is the header's formula in fp64 on the ALREADY ROUNDED operands.  Inputs are exactly representable in bf16 and in f16
(`both`), so one reference serves both types.  The tolerance is derived, not measured: an lp element is one round-to-nearest-even
of an fp32 value v, so against the unrounded reference r

    |got - r| <= u (|r| + e) + e,      u = 2^-8 (bf16) / 2^-11 (f16),

with e the fp32 error bound of v: n 2^-24 sum |terms| of the accumulation (the same convolution on absolute values, in fp64), carried
through the affine, the gate and the residual with their derivatives; v_exp_f32 / v_rcp_f32 are 1 ulp each, the argument of the
exponential is one rounded product ((|g| + 8) 2^-23 relative on the sigmoid covers both with room).  The fp32 outputs (head partials,
attention maps, the combine, the stand-alone heads) get e alone.  Converters, packs, the mask, mbits and the attention fragments are
compared by bits.  Worst err / tolerance per entry: profiles/HISTORY.md, "Later: the bf16 / f16 kernels under the arena".

TABLE: (entry, kernel instance, condition, case) - `T` in an instance stands for both BF16 and F16, every row runs for both.
tests/test_lp_abi_host.py checks the table against the launches in the sources and against tgsr_lp_conv3x3_plan.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, U = -1, -2                     # TGSR_EINVAL, TGSR_EUNSUPPORTED
F32 = 2.0 ** -24                  # unit roundoff of fp32
DTYPES = {"bf16": (1, torch.bfloat16, 2.0 ** -8), "f16": (2, torch.float16, 2.0 ** -11)}
ACT_NONE, ACT_TANH, ACT_IDENT = 0, 1, 2
ALPHA = 0.5


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(L, fn, kw):
    return getattr(L, fn)(*[v for k, v in kw.items() if not k.startswith("_")], _stream())


def both(t):
    """The values of `t` moved onto numbers exactly representable in bf16 AND in f16."""
    q = t.float().bfloat16().float()
    return torch.where(q.half().float() == q, q, torch.zeros_like(q))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def worst(got, r, e, u):
    """max err / tolerance of |got - r| <= u (|r| + e) + e."""
    err = (got.double() - r).abs()
    tol = u * (r.abs() + e) + e
    q = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max())


def lp_close(got, r, e, u, what):
    assert got.shape == r.shape, (got.shape, r.shape)
    q = worst(got, r, e, u)
    print("LPABI %s worst err/tol %.3f" % (what, q))
    assert q <= 1.0, "%s: an element is %.3f x its derived tolerance from the fp64 reference" % (what, q)


def up2(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3)


def _p(r):
    return r.ptr if r is not None else None


def run_twice(a, fn, kw, outs):
    """The call on the armed arena, its contract checked; again with the workspace-like operands refilled: the same bits."""
    M, L = _lib()
    assert call(L, fn, kw) == M.OK
    a.check()
    first = [o() for o in outs]
    a.rearm(ws_fill=1.5)
    assert call(L, fn, kw) == M.OK
    a.check()
    for f, o in zip(first, outs):
        assert same_bits(f, o()), "two calls on the same operands differ"
    return first


# ----------------------------------------------------------------------------------------------------------------------------
# References (fp64, CPU)
# ----------------------------------------------------------------------------------------------------------------------------
def epilogue_ref(acc, mag, n, scale, shift, glu, res, swap=False):
    """(value, fp32 error bound) of affine (+ GLU | + residual) on an accumulation `acc` of n products with sum |terms| = mag."""
    e = n * F32 * mag
    v = acc
    if scale is not None:
        s, t = scale.double()[None, :, None, None], shift.double()[None, :, None, None]
        v = acc * s + t
        e = e * s.abs() + 2 * F32 * ((acc * s).abs() + t.abs())
    if glu:
        co = v.shape[1] // 2
        a_, g_, ea, eg = v[:, :co], v[:, co:], e[:, :co], e[:, co:]
        if swap:
            a_, g_, ea, eg = g_, a_, eg, ea
        sg = torch.sigmoid(g_)
        v = a_ * sg
        e = sg * ea + a_.abs() * sg * (1 - sg) * eg + v.abs() * (g_.abs() + 8) * 2 * F32
    if res is not None:
        v = v + res.double()
        e = e + F32 * v.abs()
    return v, e


def conv3x3_ref(x, w, scale, shift, res, glu, up, variant=None, rows=4):
    """tgsr_lp_conv3x3_fwd / the upBlock in fp64.  variant: "tap" one tap dropped, "swap" value and gate halves swapped, "halo" the halo
    row above the second tile row (of `rows` rows) taken from the wrong tile, "phase" the two row phases of the up-sampled output swapped."""
    x, w = x.double(), w.double()
    if variant == "tap":
        w = w.clone()
        w[:, :, 0, 2] = 0
    xi = up2(x) if up else x
    acc = F.conv2d(xi, w, None, 1, 1)
    mag = F.conv2d(xi.abs(), w.abs(), None, 1, 1) if variant is None else torch.zeros_like(acc)     # a variant's bound is not used
    if variant == "halo":                            # the second tile row reads, for its top halo, what the first read: the zero border
        assert xi.shape[2] >= rows + 2
        x2 = xi[:, :, rows - 1:rows + 2].clone()
        x2[:, :, 0] = 0
        acc[:, :, rows] = F.conv2d(x2, w, None, 1, (0, 1))[:, :, 0]
    v, e = epilogue_ref(acc, mag, 9 * x.shape[1], scale, shift, glu, res, swap=variant == "swap")
    if variant == "phase":
        v = torch.stack((v[:, :, 1::2], v[:, :, 0::2]), 3).reshape(v.shape)
    return v, e


def tanh_ref(v, e, fast):
    """tanh and its bound: the derivative times e, the exponential's argument error where the epilogue's own exp-based form runs
    (1 - 2 / (exp(2v) + 1): (|v| + 1) 2^-22 on the exponential, damped by 1 - t^2), and 2^-22 for rcp and the subtraction."""
    t = torch.tanh(v)
    d = 1 - t * t
    return t, d * e + (2.0 ** -22 * (1 + v.abs()) * d if fast else 0) + 2.0 ** -22


def to3_ref(x, w, act, addend, alpha, amap, variant=None):
    """tgsr_lp_conv_to3_fwd / _map_fwd: out = act(conv) + a * addend.  variant: "tap", "notanh", "alpha" (alpha where the map applies)."""
    x, w = x.double(), w.double()
    K = w.shape[2]
    if variant == "tap":
        w = w.clone()
        w[:, :, 0, K - 1] = 0
    v, mag = F.conv2d(x, w, None, 1, K // 2), F.conv2d(x.abs(), w.abs(), None, 1, K // 2)
    e = 32 * K * K * F32 * mag
    if act == ACT_NONE:
        return v, e
    if act == ACT_TANH and variant != "notanh":
        v, e = tanh_ref(v, e, fast=False)
    if addend is None:
        return v, e
    a = amap.double()[None, None] if amap is not None and variant != "alpha" else torch.tensor(float(alpha), dtype=torch.float64)
    t = a * addend.double()
    return v + t, e + F32 * (2 * t.abs() + (v + t).abs())


def tile_partials_ref(h, w):
    """head_partial of tgsr_lp_upconv_glu_head_fwd from the stored feature image h [B][32][Ho][Wo]: per 8 x 64 tile the K x K head of
    the tile's own pixels on the (8 + 2P) x (64 + 2P) outputs they reach, [B][Ho/8][Wo/64][3][8 + 2P][64 + 2P]."""
    B, C, Ho, Wo = h.shape
    K = w.shape[2]
    P = K // 2
    t = h.double().reshape(B, C, Ho // 8, 8, Wo // 64, 64).permute(0, 2, 4, 1, 3, 5).reshape(-1, C, 8, 64)
    v, mag = F.conv2d(t, w.double(), None, 1, 2 * P), F.conv2d(t.abs(), w.double().abs(), None, 1, 2 * P)
    shape = (B, Ho // 8, Wo // 64, 3, 8 + 2 * P, 64 + 2 * P)
    return v.reshape(shape), (32 * K * K * F32 * mag).reshape(shape)


def fold_partials(p, H, W):
    """Sum of the <= 4 partials of every pixel: [B][H/8][W/64][3][8 + 2P][64 + 2P] -> [B][3][H][W] (and the same on |p|)."""
    B, ty, tx, _, NR, NX = p.shape
    P = (NR - 8) // 2
    out = torch.zeros(B, 3, H + 2 * P, W + 2 * P, dtype=torch.float64)
    for y in range(ty):
        for x in range(tx):
            out[:, :, 8 * y:8 * y + NR, 64 * x:64 * x + NX] += p[:, y, x].double()
    return out[:, :, P:P + H, P:P + W]


def mask_rows(B, Q, mode):
    """Which mask row pixel q of sample b reads: mode 0 the reference's mask.repeat order (b Q + q) % B, mode 1 its own."""
    if mode == 0:
        return (torch.arange(B)[:, None] * Q + torch.arange(Q)[None, :]) % B
    return torch.arange(B)[:, None].expand(B, Q)


def attention_ref(h, src, mask, mode, T, u):
    """tgsr_lp_word_attention_fwd in fp64 on the stored h [B][32][H][W] and the rounded projection src [B][32 i][32 t]:
    (c [B][32][H][W], its bound, P [B][T][H W], its bound).  c is the sum over t of src times the UNROUNDED softmax; that the kernel
    rounds its own fp32 softmax to the storage type first is part of the bound: |src| (u P + (1 + u) eP)."""
    B, _, H, W = h.shape
    Q = H * W
    hd, s = h.double().reshape(B, 32, Q), src.double()
    S = torch.einsum("bit,biq->btq", s, hd)
    eS = 32 * F32 * torch.einsum("bit,biq->btq", s.abs(), hd.abs())
    valid = torch.zeros(B, 32, Q, dtype=torch.bool)
    valid[:, :T] = True
    if mask is not None:
        valid[:, :T] &= ~mask[mask_rows(B, Q, mode)].permute(0, 2, 1)
    S = S.masked_fill(~valid, float("-inf"))
    mx = S.max(1, keepdim=True).values
    Pm = torch.softmax(S, 1)
    eSmax = torch.where(valid, eS, torch.zeros_like(eS)).max(1, keepdim=True).values
    gap = torch.where(valid, mx - S, torch.zeros_like(S))
    eP = Pm * (2 * eSmax + (gap + 40) * 2.0 ** -23)
    c = torch.einsum("bit,btq->biq", s, Pm)
    ec = torch.einsum("bit,btq->biq", s.abs(), u * Pm + (1 + u) * eP + 32 * F32 * Pm)
    return c.reshape(B, 32, H, W), ec.reshape(B, 32, H, W), Pm[:, :T], eP[:, :T]


# ----------------------------------------------------------------------------------------------------------------------------
# The packs, by the layouts include/tgsr_hip.h states
# ----------------------------------------------------------------------------------------------------------------------------
def conv3x3_pack_expected(w):
    Cout, Cin = w.shape[:2]
    dy, k16, dx, cb, l, j = torch.meshgrid(torch.arange(3), torch.arange(Cin // 16), torch.arange(3), torch.arange(Cout // 32),
                                           torch.arange(64), torch.arange(8), indexing="ij")
    return w[cb * 32 + (l & 31), k16 * 16 + 8 * (l >> 5) + j, dy, dx].reshape(-1)


def upconv_pack_expected(w):
    """fp32, in the order the header gives: rows first, then columns."""
    Cin = w.shape[1]
    rows = [[w[:, :, 0], w[:, :, 1] + w[:, :, 2]], [w[:, :, 0] + w[:, :, 1], w[:, :, 2]]]       # [a][dys] -> [Co][Ci][kx]
    out = torch.empty(Cin // 16, 2, 8, 2, 64, 8)
    l, j = torch.meshgrid(torch.arange(64), torch.arange(8), indexing="ij")
    for k16 in range(Cin // 16):
        ci = k16 * 16 + 8 * (l >> 5) + j
        for grp in range(2):
            for combo in range(8):
                a, b, dys = combo >> 2, (combo >> 1) & 1, combo & 1
                r = rows[a][dys]
                if grp == 0:
                    k = r[:, :, 0] if b == 0 else r[:, :, 2]
                else:
                    k = r[:, :, 1] + r[:, :, 2] if b == 0 else r[:, :, 0] + r[:, :, 1]
                for cb in range(2):
                    out[k16, grp, combo, cb] = k[cb * 32 + (l & 31), ci]
    return out.reshape(-1)


def to3_pack_expected(w):
    K = w.shape[2]
    dy, l, j = torch.meshgrid(torch.arange(K), torch.arange(64), torch.arange(8), indexing="ij")
    row, ci = l & 15, 8 * (l >> 4) + j
    c, dx = (row // K).clamp(max=2), row % K
    return torch.where(row < 3 * K, w[c, ci, dy, dx], torch.zeros(())).reshape(-1)


def att_frag_index():
    f, l, j = torch.meshgrid(torch.arange(4), torch.arange(64), torch.arange(8), indexing="ij")
    lr, lh = l % 32, l // 32
    ii = torch.where(f < 2, 16 * f + 8 * lh + j, lr)
    tt = torch.where(f < 2, lr, 16 * (f - 2) + 8 * (j // 4) + 4 * lh + (j % 4))
    return ii, tt


def att_pack_expected(src, mask, T, td):
    """att_pack as int16: src [nsets][B][32][32] fp32 -> fragments rounded once, then [B] uint32 mask words."""
    ii, tt = att_frag_index()
    frag = src.to(td)[:, :, ii, tt].reshape(-1).view(torch.int16)
    bits = torch.zeros(src.shape[1], dtype=torch.int64)
    if mask is not None:
        bits = (mask[:, :T].long() << torch.arange(T)).sum(1)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return torch.cat([frag, bits.view(torch.int16)])


PACKS = {"tgsr_lp_pack_conv3x3_weight": ("tgsr_lp_packed_conv3x3_elems", conv3x3_pack_expected),
         "tgsr_lp_pack_upconv_weight": ("tgsr_lp_packed_upconv_elems", upconv_pack_expected),
         "tgsr_lp_pack_to3_weight": (None, to3_pack_expected)}


def pack_elems(L, fn, d0, d1):
    return int(getattr(L, PACKS[fn][0])(d0, d1)) if PACKS[fn][0] else d1 * 512


def pack_dims(fn, w):
    return (w.shape[1], w.shape[2]) if fn == "tgsr_lp_pack_to3_weight" else (w.shape[0], w.shape[1])


def run_pack(fn, w, dtname):
    """The pack of `w` in an arena of its own: every element written and finite, nothing written past it."""
    M, L = _lib()
    code, td, _ = DTYPES[dtname]
    d0, d1 = pack_dims(fn, w)
    a = Arena(DEV)
    wr, pk = a.place_input(w), a.place_output16((pack_elems(L, fn, d0, d1),), td)
    kw = dict(dtype=code, w=wr.ptr, wpack=pk.ptr, d0=d0, d1=d1)
    (got,) = run_twice(a, fn, kw, [pk.read])
    return got


def fake_pack(n, td):
    return torch.arange(n, dtype=torch.int16).view(td)


# ----------------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------------
def _c(B, Cin, Cout, H, W, epi, up=0, aff=True, xcp=None, ocp=None, oco=0, rcp=None, rco=0):
    """tgsr_lp_conv3x3_fwd: H, W the OUTPUT size, epi "aff" | "glu" | "res"."""
    co = Cout // 2 if epi == "glu" else Cout
    return dict(kind="conv", B=B, Cin=Cin, Cout=Cout, H=H, W=W, epi=epi, up=up, aff=aff, xcp=xcp or Cin, ocp=ocp or co + oco, oco=oco,
                rcp=rcp or co + rco, rco=rco)


def _att(T, mask="none", attn=True, coff=32):
    """The fused / stand-alone attention of a case: mask "none" | "m0" | "m1"."""
    return dict(T=T, mask=mask, attn=attn, coff=coff)


def _u(B, Cin, H, W, hk=0, out=True, aff=True, xcp=None, ocp=None, oco=0, att=None):
    """The upBlock entries: H, W the LOW-resolution size; hk = 0 | 3 | 5 the fused head; out=False: the feature image is not written."""
    return dict(kind="up", B=B, Cin=Cin, H=H, W=W, hk=hk, out=out, aff=aff, xcp=xcp or Cin, ocp=ocp or max(64 if att else 32, 32 + oco),
                oco=oco, att=att)


def _s(B, C, H, W, ocp=None, oco=0, att=None):
    return dict(kind="stem", B=B, C=C, H=H, W=W, ocp=ocp or max(64 if att else C, C + oco), oco=oco, att=att)


def _t(B, H, W, K, act, addend=True, amap=False, xcp=32):
    return dict(kind="to3", B=B, H=H, W=W, K=K, act=act, addend=bool(addend and act), amap=amap, xcp=xcp)


def _a(B, H, W, T, mask="none", attn=True, second=False):
    """tgsr_lp_word_attention_fwd; second: c_code goes to a second image of c_cpitch 36 at c_coff 4."""
    return dict(kind="attn", B=B, H=H, W=W, att=_att(T, mask, attn, 4 if second else 32), second=second)


def _k(B, sizes, low=None, high=None, low_tanh=0, high_tanh=1, maps=None, via_map=False):
    """The combine: sizes [(H, W)] per scale; low / high: per scale whether the partial is given (default all); maps: per scale whether
    a weight map is given (None: amap == NULL); via_map: through tgsr_lp_head_combine_map."""
    n = len(sizes)
    return dict(kind="combine", B=B, sizes=sizes, low=low or [True] * n, high=high or [True] * n, low_tanh=low_tanh, high_tanh=high_tanh,
                maps=maps, via_map=via_map or maps is not None or not high_tanh)


def _x(B, T, nsets, width=None, cdf=48, tdim=32, ncf=10):
    return dict(kind="tail", B=B, T=T, nsets=nsets, width=width or T, cdf=cdf, tdim=tdim, ncf=ncf)


CONV, UP, UPHEAD, UPATT, COMBINE, COMBINEMAP, STEM, STEMATT, TO3, TO3MAP, ATTN, TAIL, RESBLOCKS = (
    "tgsr_lp_conv3x3_fwd", "tgsr_lp_upconv_glu_fwd", "tgsr_lp_upconv_glu_head_fwd", "tgsr_lp_upconv_glu_att_fwd", "tgsr_lp_head_combine",
    "tgsr_lp_head_combine_map", "tgsr_lp_stem_fwd", "tgsr_lp_stem_att_fwd", "tgsr_lp_conv_to3_fwd", "tgsr_lp_conv_to3_map_fwd",
    "tgsr_lp_word_attention_fwd", "tgsr_text_tail_lp_fwd", "tgsr_lp_resblocks_fwd")
FROM, TO, CONVERT, PACK3, PACKUP, PACKTO3 = ("tgsr_lp_from_nchw", "tgsr_lp_to_nchw", "tgsr_lp_convert", "tgsr_lp_pack_conv3x3_weight",
                                             "tgsr_lp_pack_upconv_weight", "tgsr_lp_pack_to3_weight")
_K3 = "lp_conv3x3_kernel<T,%d,%d,%s,%s,%d>"          # <T, CIN, COUT, EPI, UP, TR>
_EPI = {"aff": "kEpiAffine", "glu": "kEpiGlu", "res": "kEpiRes"}
_UPK = "lp_upconv_glu_kernel<T,%s>"                  # <T, CIN, HK[, ATT]>
_TO3 = "lp_to3_kernel<T,%d,%s>"                      # <T, K, ACT[, MAP]>
_ACT = {ACT_NONE: "TGSR_ACT_NONE", ACT_TANH: "TGSR_ACT_TANH_AXPY", ACT_IDENT: "TGSR_ACT_IDENT_AXPY"}
BIG = dict(B=64, H=32, W=64)                         # 64 * 4 * 2 = 512 tiles of 8 rows: the cheapest shape of the 8-row kernel


def conv_instance(c, rows):
    return _K3 % (c["Cin"], c["Cout"], _EPI[c["epi"]], "true" if c["up"] else "false", rows)


def _conv_rows():
    small = [  # one per (Cin, Cout, epilogue, upsample): one tile, a seam in each direction, B = 3, slices, identity affine between them
        (_c(1, 64, 128, 4, 32, "glu"), "one tile"),
        (_c(3, 64, 128, 8, 64, "glu", up=1), "a seam in each direction, B = 3"),
        (_c(2, 64, 128, 8, 64, "res", rcp=136, rco=8), "the residual from a third image at res_coff = 8"),
        (_c(1, 64, 128, 4, 32, "aff", aff=False, ocp=160, oco=32), "scale = shift = NULL; out_coff = 32 of a cpitch-160 image"),
        (_c(3, 64, 64, 8, 64, "glu", xcp=72), "x_cpitch = 72 with Cin = 64"),
        (_c(1, 64, 64, 8, 64, "glu", up=1, ocp=72, oco=32), "out_coff = 32 of a cpitch-72 image"),
        (_c(2, 64, 64, 12, 32, "res", aff=False, rcp=72, rco=8), "three tile rows; identity affine; res_coff = 8"),
        (_c(1, 64, 64, 4, 96, "aff", xcp=72), "three tile columns"),
        (_c(3, 32, 64, 8, 64, "glu", xcp=64), "x_cpitch = 64 with Cin = 32"),
        (_c(2, 32, 64, 8, 64, "glu", up=1, aff=False), "identity affine"),
        (_c(1, 32, 64, 4, 32, "res", rcp=72, rco=8), "one tile"),
        (_c(3, 32, 64, 8, 32, "aff", ocp=96, oco=32), "out_coff = 32 of a cpitch-96 image"),
        (_c(3, 32, 32, 8, 64, "res", xcp=64, rcp=40, rco=8, ocp=72, oco=32), "every slice at once"),
        (_c(1, 32, 32, 4, 32, "aff", aff=False), "one tile, identity affine"),
    ]
    rows = [(CONV, conv_instance(c, 4), "fewer than 512 tiles of 8 rows: " + why, c) for c, why in small]
    for c, _why in small:
        big = dict(c, **BIG)
        rows.append((CONV, conv_instance(c, 8), "B (H/8) (W/32) = 512 and H % 8 == 0: the 8-row tile", big))
    rows.append((CONV, conv_instance(small[-1][0], 4), "511 tiles of 8 rows: still the 4-row tile", _c(73, 32, 32, 56, 32, "aff")))
    return rows


TABLE = _conv_rows() + [
    # the upBlocks: one instance per (Cin, head); low-resolution 4 x 32 = one tile, 8 x 64 = 2 x 2 tiles (a pixel gets four partials)
    (UP, _UPK % "64,0", "Cin = 64", _u(3, 64, 8, 64, xcp=72, ocp=72, oco=32)),
    (UP, _UPK % "32,0", "Cin = 32; identity affine; x_cpitch = 64", _u(1, 32, 4, 32, aff=False, xcp=64)),
    (UPHEAD, _UPK % "64,3", "head_k = 3", _u(2, 64, 8, 64, hk=3)),
    (UPHEAD, _UPK % "64,3", "... out = NULL: the feature image is not written", _u(1, 64, 4, 32, hk=3, out=False)),
    (UPHEAD, _UPK % "32,3", "head_k = 3, Cin = 32", _u(1, 32, 4, 32, hk=3)),
    (UPHEAD, _UPK % "64,5", "head_k = 5, out = NULL", _u(1, 64, 8, 64, hk=5, out=False)),
    (UPHEAD, _UPK % "32,5", "head_k = 5, Cin = 32, B = 3, out_coff = 32", _u(3, 32, 4, 32, hk=5, ocp=72, oco=32)),
    (UPATT, _UPK % "64,0,true", "no head; T = 7, mask in mode 0 at B = 3: rows mix samples", _u(3, 64, 4, 32, att=_att(7, "m0"))),
    (UPATT, _UPK % "64,0,true", "... T = 1, no mask", _u(2, 64, 4, 32, att=_att(1))),
    (UPATT, _UPK % "64,0,true", "... T = 32, mask in mode 1, attn = NULL, a seam", _u(2, 64, 8, 64, att=_att(32, "m1", attn=False))),
    (UPATT, _UPK % "64,3,true", "head_k = 3; T = 7, mode 1", _u(2, 64, 8, 64, hk=3, att=_att(7, "m1"))),
    (COMBINE, "lp_head_combine_kernel", "one scale", _k(3, [(8, 64)])),
    (COMBINE, "lp_head_combine_kernel", "four scales of different sizes; low an input at one, no high at another; low_tanh",
     _k(2, [(8, 64), (16, 64), (8, 128), (16, 128)], low=[True, False, True, True], high=[True, True, False, True], low_tanh=1)),
    (COMBINEMAP, "lp_head_combine_map_kernel<true,true>", "high_tanh, a map at one scale only", _k(2, [(16, 128), (8, 64)], maps=[False, True])),
    (COMBINEMAP, "lp_head_combine_map_kernel<true,false>", "high_tanh, amap = NULL", _k(3, [(8, 64)], via_map=True)),
    (COMBINEMAP, "lp_head_combine_map_kernel<false,true>", "high_tanh = 0, maps", _k(2, [(8, 64), (16, 64)], high_tanh=0, maps=[True, True])),
    (COMBINEMAP, "lp_head_combine_map_kernel<false,false>", "high_tanh = 0, amap = NULL; low an input", _k(1, [(16, 128)], low=[False], high_tanh=0)),
    # the stems: any W for the non-attending form (the last column tile of W = 40 holds 8 pixels)
    (STEM, "lp_stem_kernel<T,false>", "C = 8", _s(2, 8, 5, 40)),
    (STEM, "lp_stem_kernel<T,false>", "C = 24, out_coff = 8", _s(1, 24, 5, 40, ocp=40, oco=8)),
    (STEM, "lp_stem_kernel<T,false>", "C = 32, B = 3", _s(3, 32, 5, 40)),
    (STEM, "lp_stem_kernel<T,false>", "C = 64: every thread of the workgroup computes", _s(1, 64, 5, 40)),
    (STEMATT, "lp_stem_kernel<T,true>", "T = 7, mode 0 at B = 3", _s(3, 32, 5, 32, att=_att(7, "m0"))),
    (STEMATT, "lp_stem_kernel<T,true>", "T = 1, no mask, two column tiles", _s(2, 32, 5, 64, att=_att(1))),
    (STEMATT, "lp_stem_kernel<T,true>", "T = 32, mode 1, attn = NULL", _s(2, 32, 5, 32, att=_att(32, "m1", attn=False))),
    # the stand-alone heads
    (TO3, _TO3 % (3, _ACT[0]), "one tile", _t(1, 8, 32, 3, ACT_NONE)),
    (TO3, _TO3 % (5, _ACT[0]), "a seam in each direction, B = 3, x_cpitch = 64", _t(3, 16, 64, 5, ACT_NONE, xcp=64)),
    (TO3, _TO3 % (3, _ACT[1]), "tanh + alpha * addend", _t(2, 16, 64, 3, ACT_TANH)),
    (TO3, _TO3 % (5, _ACT[1]), "addend = NULL under TANH_AXPY", _t(1, 8, 32, 5, ACT_TANH, addend=False)),
    (TO3MAP, _TO3 % (3, _ACT[1] + ",true"), "tanh, a map", _t(2, 8, 64, 3, ACT_TANH, amap=True)),
    (TO3MAP, _TO3 % (5, _ACT[1] + ",true"), "tanh, a map, a seam", _t(3, 16, 64, 5, ACT_TANH, amap=True)),
    (TO3MAP, _TO3 % (3, _ACT[2]), "identity, alpha", _t(1, 16, 32, 3, ACT_IDENT)),
    (TO3MAP, _TO3 % (5, _ACT[2]), "identity, alpha, B = 3", _t(3, 8, 32, 5, ACT_IDENT, xcp=64)),
    (TO3MAP, _TO3 % (3, _ACT[2] + ",true"), "identity, a map", _t(2, 16, 64, 3, ACT_IDENT, amap=True)),
    (TO3MAP, _TO3 % (5, _ACT[2] + ",true"), "identity, a map", _t(1, 8, 64, 5, ACT_IDENT, amap=True)),
    # the stand-alone attention
    (ATTN, "lp_word_attention_kernel<T>", "T = 7, mode 0 at B = 3", _a(3, 8, 32, 7, "m0")),
    (ATTN, "lp_word_attention_kernel<T>", "T = 1, no mask, odd H", _a(2, 5, 32, 1)),
    (ATTN, "lp_word_attention_kernel<T>", "T = 32, mode 1, attn = NULL", _a(2, 4, 64, 32, "m1", attn=False)),
    (ATTN, "lp_word_attention_kernel<T>", "c_img a second image, c_cpitch = 36, c_coff = 4", _a(3, 4, 32, 7, "m1", second=True)),
    (ATTN, "lp_word_attention_kernel<T>", "B = 257 in mode 0: mask rows past the 256 the LDS copy holds", _a(257, 4, 32, 5, "m0")),
    (TAIL, "text_tail_kernel", "T = 1, one set", _x(2, 1, 1, width=4)),
    (TAIL, "text_tail_kernel", "T = 32 (bit 31 of mbits), B = 17, four sets, width > T, aligned float4 rows (tdim = 64)", _x(17, 32, 4, width=35, tdim=64)),
    (FROM, "lp_from_nchw_kernel<T>", "odd sizes, a channel slice", dict(kind="from", B=3, C=5, H=5, W=7, cpitch=12, coff=4)),
    (TO, "lp_to_nchw_kernel<T>", "odd sizes, a channel slice", dict(kind="to", B=3, C=5, H=5, W=7, cpitch=12, coff=4)),
    (CONVERT, "lp_convert_kernel<F16,BF16>", "f16 -> bf16: one rounding", dict(kind="convert", n=8 * 1031, src="f16")),
    (CONVERT, "lp_convert_kernel<BF16,F16>", "bf16 -> f16: exact", dict(kind="convert", n=8 * 1031, src="bf16")),
    (PACK3, "lp_pack_conv3x3_kernel<T>", "64 -> 128", dict(kind="pack", fn=PACK3, shape=(128, 64, 3, 3))),
    (PACK3, "lp_pack_conv3x3_kernel<T>", "48 -> 96: no power of two", dict(kind="pack", fn=PACK3, shape=(96, 48, 3, 3))),
    (PACKUP, "lp_pack_upconv_kernel<T>", "Cin = 64", dict(kind="pack", fn=PACKUP, shape=(64, 64, 3, 3))),
    (PACKUP, "lp_pack_upconv_kernel<T>", "Cin = 32", dict(kind="pack", fn=PACKUP, shape=(64, 32, 3, 3))),
    (PACKTO3, "lp_pack_to3_kernel<T>", "K = 3: rows 9 .. 15 are zero", dict(kind="pack", fn=PACKTO3, shape=(3, 32, 3, 3))),
    (PACKTO3, "lp_pack_to3_kernel<T>", "K = 5: row 15 is zero", dict(kind="pack", fn=PACKTO3, shape=(3, 32, 5, 5))),
    (RESBLOCKS, "lp_resblocks_kernel<T,4>", "refusals only (refusals()): its tiles spin on a flag buffer the function owns across launches, and "
     "prefilling or disturbing that buffer - what every case here does to its operands - could make the kernel wait; its bit-identity to four "
     "separate launches is held by tests/test_hip_lp.py", None),
]


def _rows(*entries):
    return [r for r in TABLE if r[3] is not None and (not entries or r[0] in entries)]


def case_id(c):
    def att(a):
        return "" if a is None else "-T%d%s%s" % (a["T"], a["mask"], "" if a["attn"] else "-noattn")
    k = c["kind"]
    if k == "conv":
        return "%dto%d-%s%s-B%d-%dx%d-x%d-o%d+%d%s%s" % (c["Cin"], c["Cout"], c["epi"], "-up" if c["up"] else "", c["B"], c["H"], c["W"], c["xcp"],
                                                       c["ocp"], c["oco"], "" if c["aff"] else "-noaff", "-r%d+%d" % (c["rcp"], c["rco"]) if c["epi"] == "res" else "")
    if k == "up":
        return "up%d-hk%d-B%d-%dx%d-o%d+%d%s%s%s" % (c["Cin"], c["hk"], c["B"], c["H"], c["W"], c["ocp"], c["oco"], "" if c["out"] else "-noout",
                                                   "" if c["aff"] else "-noaff", att(c["att"]))
    if k == "stem":
        return "stem%d-B%d-%dx%d-o%d+%d%s" % (c["C"], c["B"], c["H"], c["W"], c["ocp"], c["oco"], att(c["att"]))
    if k == "to3":
        return "to3-K%d-act%d-B%d-%dx%d-x%d%s%s" % (c["K"], c["act"], c["B"], c["H"], c["W"], c["xcp"], "-add" if c["addend"] else "", "-map" if c["amap"] else "")
    if k == "attn":
        return "attn-B%d-%dx%d%s%s" % (c["B"], c["H"], c["W"], att(c["att"]), "-second" if c["second"] else "")
    if k == "combine":
        return "combine-B%d-%s-l%s-h%s-lt%d-ht%d-m%s%s" % (c["B"], "_".join("%dx%d" % s for s in c["sizes"]), "".join(str(int(v)) for v in c["low"]),
                                                         "".join(str(int(v)) for v in c["high"]), c["low_tanh"], c["high_tanh"],
                                                         "".join(str(int(v)) for v in c["maps"]) if c["maps"] else "none", "-viamap" if c["via_map"] else "")
    if k == "tail":
        return "tail-B%d-T%d-sets%d-w%d-tdim%d" % (c["B"], c["T"], c["nsets"], c["width"], c["tdim"])
    if k == "pack":
        return "%s-%s" % (c["fn"][8:], "x".join(str(s) for s in c["shape"]))
    if k == "convert":
        return "convert-from-%s" % c["src"]
    return "%s-B%d-C%d-%dx%d-cp%d+%d" % (k, c["B"], c["C"], c["H"], c["W"], c["cpitch"], c["coff"])


def row_id(r):
    return case_id(r[3])


# ----------------------------------------------------------------------------------------------------------------------------
# Inputs (once per case, shared by the two types and by tests/test_lp_abi_host.py)
# ----------------------------------------------------------------------------------------------------------------------------
def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def ckey(c):
    return (c["B"], c["Cin"], c["Cout"], c["H"], c["W"], c["epi"], c["up"], c["aff"])


@functools.lru_cache(maxsize=2)
def conv_inputs(key):
    B, Cin, Cout, H, W, epi, up, aff = key
    g = _gen(B, Cin, Cout, H, W, len(epi), up)
    Hi, Wi = (H // 2, W // 2) if up else (H, W)
    x = both(torch.randn(B, Cin, Hi, Wi, generator=g))
    w = both(torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5))
    scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
    co = Cout // 2 if epi == "glu" else Cout
    res = both(torch.randn(B, co, H, W, generator=g)) if epi == "res" else None
    return x, w, (scale if aff else None), (shift if aff else None), res


@functools.lru_cache(maxsize=2)
def conv_refs(key):
    x, w, scale, shift, res = conv_inputs(key)
    r, e = conv3x3_ref(x, w, scale, shift, res, key[5] == "glu", key[6])
    return r, e


def attention_inputs(B, T, mask, seed):
    """src [2 sets][B][32][32] (zero at words >= T, representable in both types) and the mask [B][T] (every row keeps a word)."""
    g = _gen(B, T, seed)
    src = both(torch.randn(2, B, 32, 32, generator=g) * 0.4)
    src[..., T:] = 0
    if mask == "none":
        return src, None
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 256:
        lens[256] = min(2, T)
    return src, torch.arange(T)[None, :] >= lens[:, None]


@functools.lru_cache(maxsize=8)
def up_inputs(B, Cin, H, W, hk, aff):
    """x, the 3x3 filter on the grid k / 256, |k| <= 16 (every pre-summed tap is then exact in both types: the sub-pixel form IS the
    direct one), the affine, and the head's filter."""
    g = _gen(B, Cin, H, W, 3)                         # not hk: the same upBlock with and without its head
    x = both(torch.randn(B, Cin, H, W, generator=g))
    w = torch.randint(-16, 17, (64, Cin, 3, 3), generator=g).float() / 256
    scale, shift = 0.5 + torch.rand(64, generator=g), 0.3 * torch.randn(64, generator=g)
    hw = both(torch.randn(3, 32, hk, hk, generator=_gen(hk, 29)) / (hk * 32 ** 0.5)) if hk else None
    return x, w, (scale if aff else None), (shift if aff else None), hw


@functools.lru_cache(maxsize=8)
def stem_inputs(B, C, H, W):
    g = _gen(B, C, H, W, 5)
    x = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    w = torch.randn(2 * C, 3, 3, 3, generator=g) / 5.0
    return x, w, 0.5 + torch.rand(2 * C, generator=g), 0.3 * torch.randn(2 * C, generator=g)


def stem_ref(x, w, scale, shift, variant=None):
    x, w = x.double(), w.double()
    if variant == "tap":
        w = w.clone()
        w[:, :, 0, 2] = 0
    acc, mag = F.conv2d(x, w, None, 1, 1), F.conv2d(x.abs(), w.abs(), None, 1, 1)
    return epilogue_ref(acc, mag, 27, scale, shift, True, None, swap=variant == "swap")


@functools.lru_cache(maxsize=8)
def to3_inputs(B, H, W, K, act, addend, amap):
    g = _gen(B, H, W, K, act, 11)
    x = both(torch.randn(B, 32, H, W, generator=g))
    w = both(torch.randn(3, 32, K, K, generator=g) / (K * 32 ** 0.5) * (3.0 if act == ACT_TANH else 1.0))
    add = torch.randn(B, 3, H, W, generator=g) if addend else None
    m = 0.3 + torch.rand(H, W, generator=g) if amap else None
    return x, w, add, m


def to3_key(c):
    return (c["B"], c["H"], c["W"], c["K"], c["act"], c["addend"], c["amap"])


def combine_inputs(c):
    g = _gen(c["B"], len(c["sizes"]), c["low_tanh"], c["high_tanh"], 13)
    out = []
    for k, (H, W) in enumerate(c["sizes"]):
        pl = torch.randn(c["B"], H // 8, W // 64, 3, 10, 66, generator=g) * 0.4 if c["low"][k] else None
        ph = torch.randn(c["B"], H // 8, W // 64, 3, 12, 68, generator=g) * 0.4 if c["high"][k] else None
        low = torch.randn(c["B"], 3, H, W, generator=g) if not c["low"][k] else None
        m = 0.3 + torch.rand(H, W, generator=g) if c["maps"] and c["maps"][k] else None
        out.append((pl, ph, low, m))
    return out


def combine_ref(c, variant=None):
    """[(low, e_low, high or None, e_high)] per scale.  variant: "partial" one of the four partials of the pixels at the tile corner left
    out, "alpha" alpha where a map applies, "notanh" the tanh of the high head dropped."""
    out = []
    for (pl, ph, low_in, m), (H, W) in zip(combine_inputs(c), c["sizes"]):
        if pl is not None:
            if variant == "partial" and pl.shape[1] * pl.shape[2] > 1:
                pl = pl.clone()
                pl[:, -1, -1, :, :2, :2] = 0
            low, e_low = fold_partials(pl, H, W), 3 * F32 * fold_partials(pl.abs(), H, W)
            if c["low_tanh"]:
                low, e_low = tanh_ref(low, e_low, fast=True)
        else:
            low, e_low = low_in.double(), torch.zeros(low_in.shape, dtype=torch.float64)
        high = e_high = None
        if ph is not None:
            if variant == "partial" and ph.shape[1] * ph.shape[2] > 1:
                ph = ph.clone()
                ph[:, -1, -1, :, :4, :4] = 0
            high, e_high = fold_partials(ph, H, W), 3 * F32 * fold_partials(ph.abs(), H, W)
            if c["high_tanh"] and variant != "notanh":
                high, e_high = tanh_ref(high, e_high, fast=True)
            a = m.double()[None, None] if m is not None and variant != "alpha" else torch.tensor(ALPHA, dtype=torch.float64)
            t = a * low
            high, e_high = high + t, e_high + a.abs() * e_low + F32 * (2 * t.abs() + (high + t).abs())
        out.append((low, e_low, high, e_high))
    return out


def tail_inputs(c):
    g = _gen(c["B"], c["T"], c["nsets"], 17)
    B, T = c["B"], c["T"]
    words = torch.randn(B, c["cdf"], T, generator=g)
    ws = [torch.randn(32, c["cdf"], generator=g) / c["cdf"] ** 0.5 for _ in range(c["nsets"])]
    sent = torch.randn(B, c["tdim"], generator=g)
    caw, cab = torch.randn(4 * c["ncf"], c["tdim"], generator=g) / 8, torch.randn(4 * c["ncf"], generator=g)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    cap = torch.zeros(B, c["width"], dtype=torch.int64)
    for b in range(B):
        cap[b, :int(lens[b])] = torch.randint(1, 40, (int(lens[b]),), generator=g)
    cap[:, T:] = 7                       # behind the T words the kernel reads: nothing it may take for padding
    return words, ws, sent, caw, cab, cap


# ----------------------------------------------------------------------------------------------------------------------------
# Placing the operands of an entry: (arena, regions, named arguments in the order of the C signature)
# ----------------------------------------------------------------------------------------------------------------------------
def place_conv(c, dtname, pack, written=True):
    code, td, _ = DTYPES[dtname]
    x, _w, scale, shift, res = conv_inputs(ckey(c))
    co = c["Cout"] // 2 if c["epi"] == "glu" else c["Cout"]
    a = Arena(DEV)
    r = {"x": a.place_lp(td, c["B"], x.shape[2], x.shape[3], c["xcp"], reads=[(0, x)]), "pack": a.place_input16(pack),
         "scale": a.place_input(scale) if scale is not None else None, "shift": a.place_input(shift) if shift is not None else None,
         "res": a.place_lp(td, c["B"], c["H"], c["W"], c["rcp"], reads=[(c["rco"], res)]) if res is not None else None,
         "out": a.place_lp(td, c["B"], c["H"], c["W"], c["ocp"], writes=[(c["oco"], co)], written=written)}
    kw = dict(dtype=code, x=r["x"].ptr, x_cpitch=c["xcp"], B=c["B"], Cin=c["Cin"], H=c["H"], W=c["W"], wpack=r["pack"].ptr, Cout=c["Cout"],
              scale=_p(r["scale"]), shift=_p(r["shift"]), residual=_p(r["res"]), res_cpitch=c["rcp"] if res is not None else 0,
              res_coff=c["rco"] if res is not None else 0, out=r["out"].ptr, out_cpitch=c["ocp"], out_coff=c["oco"],
              epilogue=1 if c["epi"] == "glu" else 0, upsample=c["up"])
    return a, r, kw


def _place_att(a, att, B, dtname, seed):
    """att_pack (two sets, the stage attends through set 1) and attn of a fused attention; the named arguments behind head_partial."""
    _code, td, _ = DTYPES[dtname]
    src, mask = attention_inputs(B, att["T"], att["mask"], seed)
    r = {"att_pack": a.place_input16(att_pack_expected(src, mask, att["T"], td))}
    return r, lambda: dict(att_pack=r["att_pack"].ptr, att_nsets=2, att_set=1, use_mask=int(mask is not None), mask_mode=int(att["mask"] == "m1"),
                   T=att["T"], c_coff=att["coff"]), src[1], mask


def place_up(c, dtname, pack, hpack, written=True, out=None, att=True):
    """out / att: overrides of the case's (the identities below call the same inputs without the head, the image or the attention)."""
    M, L = _lib()
    code, td, _ = DTYPES[dtname]
    x, _w, scale, shift, _hw = up_inputs(c["B"], c["Cin"], c["H"], c["W"], c["hk"], c["aff"])
    want_out = c["out"] if out is None else out
    att = c["att"] if att else None
    B, Ho, Wo = c["B"], 2 * c["H"], 2 * c["W"]
    a = Arena(DEV)
    writes = [(c["oco"], 32)] + ([(att["coff"], 32)] if att else [])
    r = {"x": a.place_lp(td, B, c["H"], c["W"], c["xcp"], reads=[(0, x)]), "pack": a.place_input16(pack),
         "scale": a.place_input(scale) if scale is not None else None, "shift": a.place_input(shift) if shift is not None else None,
         "out": a.place_lp(td, B, Ho, Wo, c["ocp"], writes=writes, written=written) if want_out else None,
         "hpack": a.place_input16(hpack) if c["hk"] else None,
         "hpart": a.place_output((int(L.tgsr_lp_head_partial_elems(B, Ho, Wo, c["hk"])),), written=written) if c["hk"] else None, "attn": None}
    if att:
        ra, kwa, src, mask = _place_att(a, att, B, dtname, 1)
        r.update(ra, src=src, mask=mask)
        if att["attn"]:
            r["attn"] = a.place_output((B, att["T"], Ho * Wo), written=written)
    kw = dict(dtype=code, x=r["x"].ptr, x_cpitch=c["xcp"], B=B, Cin=c["Cin"], H=c["H"], W=c["W"], wpack=r["pack"].ptr, Cout=64,
              scale=_p(r["scale"]), shift=_p(r["shift"]), out=_p(r["out"]), out_cpitch=c["ocp"], out_coff=c["oco"])
    fn = UP
    if c["hk"] or att:
        kw.update(head_wpack=_p(r["hpack"]), head_k=c["hk"], head_partial=_p(r["hpart"]))
        fn = UPHEAD
    if att:
        kw.update(kwa(), attn=_p(r["attn"]))
        fn = UPATT
    return a, r, kw, fn


def place_stem(c, dtname, written=True, att=True):
    code, td, _ = DTYPES[dtname]
    x, w, scale, shift = stem_inputs(c["B"], c["C"], c["H"], c["W"])
    att = c["att"] if att else None
    a = Arena(DEV)
    writes = [(c["oco"], c["C"])] + ([(att["coff"], 32)] if att else [])
    r = {"x": a.place_input(x), "w": a.place_input(w), "scale": a.place_input(scale), "shift": a.place_input(shift),
         "out": a.place_lp(td, c["B"], c["H"], c["W"], c["ocp"], writes=writes, written=written), "attn": None}
    if att:
        ra, kwa, src, mask = _place_att(a, att, c["B"], dtname, 2)
        r.update(ra, src=src, mask=mask)
        if att["attn"]:
            r["attn"] = a.place_output((c["B"], att["T"], c["H"] * c["W"]), written=written)
    kw = dict(dtype=code, x=r["x"].ptr, B=c["B"], H=c["H"], W=c["W"], w=r["w"].ptr, C=c["C"], scale=r["scale"].ptr, shift=r["shift"].ptr,
              out=r["out"].ptr, out_cpitch=c["ocp"], out_coff=c["oco"])
    fn = STEM
    if att:
        kw.update(kwa(), attn=_p(r["attn"]))
        fn = STEMATT
    return a, r, kw, fn


def place_to3(c, dtname, pack, written=True, via_map=None):
    code, td, _ = DTYPES[dtname]
    x, _w, add, m = to3_inputs(*to3_key(c))
    via_map = (c["amap"] or c["act"] == ACT_IDENT) if via_map is None else via_map
    a = Arena(DEV)
    r = {"x": a.place_lp(td, c["B"], c["H"], c["W"], c["xcp"], reads=[(0, x)]), "pack": a.place_input16(pack),
         "addend": a.place_input(add) if add is not None else None, "amap": a.place_input(m) if m is not None else None,
         "out": a.place_output((c["B"], 3, c["H"], c["W"]), written=written)}
    kw = dict(dtype=code, x=r["x"].ptr, x_cpitch=c["xcp"], B=c["B"], Cin=32, H=c["H"], W=c["W"], wpack=r["pack"].ptr, K=c["K"], act=c["act"],
              addend=_p(r["addend"]), alpha=ALPHA)
    if via_map:
        kw["amap"] = _p(r["amap"])
    kw["out"] = r["out"].ptr
    return a, r, kw, TO3MAP if via_map else TO3


def place_attn(c, dtname, h=None, src=None, mask=None, written=True):
    """The stand-alone attention; h / src / mask: another h (the stored output of a producer) and that producer's words."""
    code, td, _ = DTYPES[dtname]
    att, B, H, W = c["att"], c["B"], c["H"], c["W"]
    if h is None:
        h = both(torch.randn(B, 32, H, W, generator=_gen(B, H, W, 19)))
        s2, mask = attention_inputs(B, att["T"], att["mask"], 3)
        src = s2[1]
    a = Arena(DEV)
    r = {"src_r": a.place_input(src), "mask_r": a.place_input(mask.to(torch.uint8)) if mask is not None else None, "hval": h, "src": src,
         "mask": mask, "attn": a.place_output((B, att["T"], H * W), written=written) if att["attn"] else None}
    if c.get("second"):
        r["h"] = a.place_lp(td, B, H, W, 40, reads=[(0, h)])
        r["c"] = a.place_lp(td, B, H, W, 36, writes=[(att["coff"], 32)], written=written)
    else:
        r["h"] = r["c"] = a.place_lp(td, B, H, W, 64, reads=[(0, h)], writes=[(att["coff"], 32)], written=written)
    kw = dict(dtype=code, h=r["h"].ptr, h_cpitch=r["h"].cpitch, src=r["src_r"].ptr, mask=_p(r["mask_r"]), mask_mode=int(att["mask"] == "m1"), B=B,
              idf=32, T=att["T"], H=H, W=W, c_img=r["c"].ptr, c_cpitch=r["c"].cpitch, c_coff=att["coff"], attn=_p(r["attn"]))
    return a, r, kw, ATTN


def _ptrs(regions):
    arr = (ctypes.c_void_p * len(regions))(*[(None if r is None else r.address) for r in regions])
    return arr


def place_combine(c, written=True, via_map=None):
    via_map = c["via_map"] if via_map is None else via_map
    n, B = len(c["sizes"]), c["B"]
    a = Arena(DEV)
    r = {"pl": [], "ph": [], "low": [], "high": [], "amap": []}
    for (pl, ph, low, m), (H, W) in zip(combine_inputs(c), c["sizes"]):
        r["pl"].append(a.place_input(pl) if pl is not None else None)
        r["ph"].append(a.place_input(ph) if ph is not None else None)
        r["low"].append(a.place_input(low) if low is not None else a.place_output((B, 3, H, W), written=written))
        r["high"].append(a.place_output((B, 3, H, W), written=written) if ph is not None else None)
        r["amap"].append(a.place_input(m) if m is not None else None)
    a.buffer()
    kw = dict(nscales=n, B=B, H=(ctypes.c_int * n)(*[s[0] for s in c["sizes"]]), W=(ctypes.c_int * n)(*[s[1] for s in c["sizes"]]),
              partial_low=_ptrs(r["pl"]), partial_high=_ptrs(r["ph"]), low=_ptrs(r["low"]), high=_ptrs(r["high"]))
    if via_map:
        kw.update(amap=_ptrs(r["amap"]) if c["maps"] else None, low_tanh=c["low_tanh"], high_tanh=c["high_tanh"], alpha=ALPHA)
    else:
        kw.update(low_tanh=c["low_tanh"], alpha=ALPHA)
    return a, r, kw, COMBINEMAP if via_map else COMBINE


def place_tail(c, dtname, written=True, lp=True):
    M, L = _lib()
    code, td, _ = DTYPES[dtname]
    words, ws, sent, caw, cab, cap = tail_inputs(c)
    B, T, ns = c["B"], c["T"], c["nsets"]
    a = Arena(DEV)
    r = {"words": a.place_input(words), "ws": [a.place_input(w) for w in ws], "sent": a.place_input(sent), "caw": a.place_input(caw),
         "cab": a.place_input(cab), "cap": a.place_input(cap), "src": a.place_output((ns, B, 32, 32), written=written),
         "mu": a.place_output((B, c["ncf"]), written=written), "logvar": a.place_output((B, c["ncf"]), written=written),
         "mask": a.place_output_u8((B, T), written=written),
         "pack": a.place_output16((int(L.tgsr_lp_att_pack_bytes(ns, B)) // 2,), td, written=written, finite=False) if lp else None}
    a.buffer()
    kw = dict(words=r["words"].ptr, w_ctx=_ptrs(r["ws"]), nsets=ns, B=B, idf=32, cdf=c["cdf"], T=T, src_out=r["src"].ptr, sent_emb=r["sent"].ptr,
              ca_w=r["caw"].ptr, ca_b=r["cab"].ptr, tdim=c["tdim"], ncf=c["ncf"], mu=r["mu"].ptr, logvar=r["logvar"].ptr, captions=r["cap"].ptr,
              width=c["width"], mask=r["mask"].ptr)
    if lp:
        kw.update(lp_dtype=code, att_pack=r["pack"].ptr)
    return a, r, kw, TAIL if lp else "tgsr_text_tail_fwd"


# ----------------------------------------------------------------------------------------------------------------------------
# 1: every table row
# ----------------------------------------------------------------------------------------------------------------------------
def check_attention(r, c, att, h_got, dtname, what):
    """c_code and attn of a fused or stand-alone attention against the fp64 reference on the STORED h."""
    _code, _td, u = DTYPES[dtname]
    cr, ec, Pr, eP = attention_ref(h_got, r["src"], r["mask"], int(att["mask"] == "m1"), att["T"], u)
    c_got = r["c"].nchw(att["coff"], 32) if "c" in r else r["out"].nchw(att["coff"], 32)
    lp_close(c_got, cr, ec, u, what + " c_code")
    if att["attn"]:
        lp_close(r["attn"].read().reshape(Pr.shape), Pr, eP, 0.0, what + " attn")


def run_conv(c, dtname, instance):
    M, L = _lib()
    assert "%d>" % L.tgsr_lp_conv3x3_plan(c["B"], c["H"], c["W"]) == instance[-2:], "the planner takes another tile for this case"
    _x_, w, *_ = conv_inputs(ckey(c))
    pack = run_pack(PACK3, w, dtname)
    assert same_bits(pack.float(), conv3x3_pack_expected(w)), "the filter is representable: its pack holds it exactly"
    a, r, kw = place_conv(c, dtname, pack)
    co = c["Cout"] // 2 if c["epi"] == "glu" else c["Cout"]
    (got,) = run_twice(a, CONV, kw, [lambda: r["out"].nchw(c["oco"], co)])
    ref, e = conv_refs(ckey(c))
    lp_close(got, ref, e, DTYPES[dtname][2], "conv3x3 " + case_id(c) + " " + dtname)


def run_up(c, dtname, _instance):
    M, L = _lib()
    _code, _td, u = DTYPES[dtname]
    x, w, scale, shift, hw = up_inputs(c["B"], c["Cin"], c["H"], c["W"], c["hk"], c["aff"])
    pack = run_pack(PACKUP, w, dtname)
    hpack = run_pack(PACKTO3, hw, dtname) if c["hk"] else None
    a, r, kw, fn = place_up(c, dtname, pack, hpack)
    outs = ([lambda: r["out"].elements()] if r["out"] is not None else []) + ([r["hpart"].read] if c["hk"] else []) + (
        [r["attn"].read] if r["attn"] is not None else [])
    run_twice(a, fn, kw, outs)
    what = "upconv " + case_id(c) + " " + dtname
    if r["out"] is not None:
        h = r["out"].nchw(c["oco"], 32)
        ref, e = conv3x3_ref(x, w, scale, shift, None, True, True)
        lp_close(h, ref, e, u, what + " h")
    else:                                           # the image the head saw: the same call with the image written (identity 5 below)
        b, rb, kwb, fnb = place_up(c, dtname, pack, hpack, out=True)
        assert call(L, fnb, kwb) == M.OK
        b.check()
        h = rb["out"].nchw(c["oco"], 32)
        assert same_bits(rb["hpart"].read(), r["hpart"].read())
    if c["hk"]:
        pr, pe = tile_partials_ref(h, hw)
        lp_close(r["hpart"].read().reshape(pr.shape), pr, pe, 0.0, what + " head_partial")
    if c["att"]:
        check_attention(r, c, c["att"], h, dtname, what)


def run_stem(c, dtname, _instance):
    _code, _td, u = DTYPES[dtname]
    x, w, scale, shift = stem_inputs(c["B"], c["C"], c["H"], c["W"])
    a, r, kw, fn = place_stem(c, dtname)
    run_twice(a, fn, kw, [lambda: r["out"].elements()] + ([r["attn"].read] if r["attn"] is not None else []))
    h = r["out"].nchw(c["oco"], c["C"])
    ref, e = stem_ref(x, w, scale, shift)
    what = "stem " + case_id(c) + " " + dtname
    lp_close(h, ref, e, u, what + " h")
    if c["att"]:
        check_attention(r, c, c["att"], h, dtname, what)


def run_to3(c, dtname, _instance):
    x, w, add, m = to3_inputs(*to3_key(c))
    pack = run_pack(PACKTO3, w, dtname)
    a, r, kw, fn = place_to3(c, dtname, pack)
    (got,) = run_twice(a, fn, kw, [r["out"].read])
    ref, e = to3_ref(x, w, c["act"], add, ALPHA, m)
    lp_close(got, ref, e, 0.0, "to3 " + case_id(c) + " " + dtname)


def run_attn(c, dtname, _instance):
    a, r, kw, fn = place_attn(c, dtname)
    run_twice(a, fn, kw, [lambda: r["c"].elements()] + ([r["attn"].read] if r["attn"] is not None else []))
    check_attention(r, c, c["att"], r["hval"], dtname, "attention " + case_id(c) + " " + dtname)


def run_combine(c, _dtname, _instance):
    a, r, kw, fn = place_combine(c)
    outs = [x.read for x, given in zip(r["low"], c["low"]) if given] + [x.read for x in r["high"] if x is not None]
    run_twice(a, fn, kw, outs)
    for k, (low, e_low, high, e_high) in enumerate(combine_ref(c)):
        what = "combine %s scale %d" % (case_id(c), k)
        if c["low"][k]:
            lp_close(r["low"][k].read(), low, e_low, 0.0, what + " low")
        if high is not None:
            lp_close(r["high"][k].read(), high, e_high, 0.0, what + " high")


def run_tail(c, dtname, _instance):
    M, L = _lib()
    _code, td, _u = DTYPES[dtname]
    words, ws, _sent, _caw, _cab, cap = tail_inputs(c)
    a, r, kw, fn = place_tail(c, dtname)
    src, mu, lv, m8, pack = run_twice(a, fn, kw, [r["src"].read, r["mu"].read, r["logvar"].read, r["mask"].read, r["pack"].read])
    mask = cap[:, :c["T"]] == 0
    assert torch.equal(m8, mask.to(torch.uint8))
    assert same_bits(pack.view(torch.int16), att_pack_expected(src, mask, c["T"], td)), "att_pack is not the rounded src_out / the mask words"
    want = torch.stack([torch.einsum("ic,bct->bit", w.double(), words.double()) for w in ws])
    mag = torch.stack([torch.einsum("ic,bct->bit", w.double().abs(), words.double().abs()) for w in ws])
    lp_close(src[..., :c["T"]], want, c["cdf"] * F32 * mag, 0.0, "text tail src_out " + case_id(c))
    assert float(src[..., c["T"]:].abs().sum()) == 0.0


def run_from(c, dtname, _instance):
    code, td, _ = DTYPES[dtname]
    x = torch.randn(c["B"], c["C"], c["H"], c["W"], generator=_gen(1)) * 3
    a = Arena(DEV)
    xr, img = a.place_input(x), a.place_lp(td, c["B"], c["H"], c["W"], c["cpitch"], writes=[(c["coff"], c["C"])])
    kw = dict(dtype=code, x=xr.ptr, out=img.ptr, B=c["B"], C=c["C"], H=c["H"], W=c["W"], cpitch=c["cpitch"], coff=c["coff"])
    run_twice(a, FROM, kw, [img.elements])
    assert torch.equal(img.nchw(c["coff"], c["C"]), x.to(td).float())


def run_to(c, dtname, _instance):
    code, td, _ = DTYPES[dtname]
    x = both(torch.randn(c["B"], c["C"], c["H"], c["W"], generator=_gen(2)) * 3)
    a = Arena(DEV)
    img, out = a.place_lp(td, c["B"], c["H"], c["W"], c["cpitch"], reads=[(c["coff"], x)]), a.place_output(x.shape)
    kw = dict(dtype=code, x=img.ptr, out=out.ptr, B=c["B"], C=c["C"], H=c["H"], W=c["W"], cpitch=c["cpitch"], coff=c["coff"])
    (got,) = run_twice(a, TO, kw, [out.read])
    assert torch.equal(got, x)


def run_convert(c, _dtname, _instance):
    src_td, dst_td = (torch.float16, torch.bfloat16) if c["src"] == "f16" else (torch.bfloat16, torch.float16)
    x = torch.randn(c["n"], generator=_gen(3)) * 3
    x = x.to(src_td) if c["src"] == "f16" else both(x).to(src_td)
    a = Arena(DEV)
    s, d = a.place_input16(x), a.place_output16((c["n"],), dst_td)
    kw = dict(src_dtype=DTYPES[c["src"]][0], src=s.ptr, dst_dtype=3 - DTYPES[c["src"]][0], dst=d.ptr, n=c["n"])
    (got,) = run_twice(a, CONVERT, kw, [d.read])
    assert same_bits(got, x.float().to(dst_td))
    if c["src"] == "bf16":
        assert torch.equal(got.float(), x.float())


def run_packrow(c, dtname, _instance):
    _code, td, _ = DTYPES[dtname]
    w = torch.randn(*c["shape"], generator=_gen(*c["shape"])) / 3                     # NOT rounded: the pack rounds, once
    got = run_pack(c["fn"], w, dtname)
    assert same_bits(got, PACKS[c["fn"]][1](w).to(td)), "the pack is not the layout include/tgsr_hip.h states"


RUN = {"conv": run_conv, "up": run_up, "stem": run_stem, "to3": run_to3, "attn": run_attn, "combine": run_combine, "tail": run_tail,
       "from": run_from, "to": run_to, "convert": run_convert, "pack": run_packrow}
ONE_TYPE = ("combine", "convert")                 # rows without a storage type run once


def _row_params():
    out = []
    for r in _rows():
        for dt in (("bf16",) if r[3]["kind"] in ONE_TYPE else ("bf16", "f16")):
            out.append(pytest.param(r, dt, id="%s-%s-%s" % (r[0][5:], row_id(r), dt)))
    return out


@pytest.mark.parametrize("row,dtname", _row_params())
def test_table_row(row, dtname):
    _entry, instance, _cond, c = row
    RUN[c["kind"]](c, dtname, instance)


def test_size_functions():
    _M, L = _lib()
    assert L.tgsr_lp_packed_conv3x3_elems(128, 64) == 128 * 64 * 9 and L.tgsr_lp_packed_upconv_elems(64, 32) == 64 * 32 * 16
    assert L.tgsr_lp_head_partial_elems(3, 16, 128, 5) == 3 * 2 * 2 * 3 * 12 * 68 and L.tgsr_lp_head_partial_elems(1, 8, 64, 3) == 3 * 10 * 66
    assert L.tgsr_lp_att_pack_bytes(4, 17) == 4 * 17 * 4096 + 4 * 17
    assert L.tgsr_lp_resblocks_flag_elems(2, 8, 64) == 4 * 2 * 2 * 2 + 1 and L.tgsr_lp_resblocks_flag_elems(2, 6, 64) == 0
    assert [L.tgsr_lp_conv3x3_plan(*s) for s in ((64, 32, 64), (63, 32, 64), (73, 56, 32), (512, 12, 32), (1, 4, 32))] == [8, 4, 4, 4, 4]
    assert [L.tgsr_lp_conv3x3_plan(*s) for s in ((0, 4, 32), (1, 6, 32), (1, 4, 48))] == [E, U, U]


# ----------------------------------------------------------------------------------------------------------------------------
# 2: the identities the header states, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
BOTH = pytest.mark.parametrize("dtname", ["bf16", "f16"])


def _c_of(row):
    return row[3]


@BOTH
@pytest.mark.parametrize("row", _rows(UPATT, STEMATT), ids=row_id)
def test_fused_attention_equals_the_stand_alone_attention_on_the_stored_h(row, dtname):
    M, L = _lib()
    c = _c_of(row)
    att = c["att"]
    if c["kind"] == "up":
        x, w, _s_, _t_, hw = up_inputs(c["B"], c["Cin"], c["H"], c["W"], c["hk"], c["aff"])
        a, r, kw, fn = place_up(c, dtname, run_pack(PACKUP, w, dtname), run_pack(PACKTO3, hw, dtname) if c["hk"] else None)
        H, W, nch = 2 * c["H"], 2 * c["W"], 32
    else:
        a, r, kw, fn = place_stem(c, dtname)
        H, W, nch = c["H"], c["W"], c["C"]
    assert call(L, fn, kw) == M.OK
    a.check()
    h = r["out"].nchw(c["oco"], nch)
    b, rb, kwb, fnb = place_attn(dict(kind="attn", B=c["B"], H=H, W=W, att=att), dtname, h=h, src=r["src"], mask=r["mask"])
    assert call(L, fnb, kwb) == M.OK
    b.check()
    assert same_bits(rb["c"].nchw(att["coff"], 32), r["out"].nchw(att["coff"], 32)), "c_code"
    if att["attn"]:
        assert same_bits(rb["attn"].read(), r["attn"].read()), "attn"


@BOTH
@pytest.mark.parametrize("row", [r for r in _rows(TO3, TO3MAP) if not r[3]["amap"] and r[3]["act"] != ACT_IDENT], ids=row_id)
def test_conv_to3_map_without_a_map_equals_conv_to3(row, dtname):
    M, L = _lib()
    c = _c_of(row)
    pack = run_pack(PACKTO3, to3_inputs(*to3_key(c))[1], dtname)
    outs = []
    for via in (False, True):
        a, r, kw, fn = place_to3(c, dtname, pack, via_map=via)
        assert fn == (TO3MAP if via else TO3) and call(L, fn, kw) == M.OK
        a.check()
        outs.append(r["out"].read())
    assert same_bits(*outs)


@pytest.mark.parametrize("row", [r for r in _rows(COMBINE, COMBINEMAP) if not r[3]["maps"] and r[3]["high_tanh"]], ids=row_id)
def test_head_combine_map_without_a_map_equals_head_combine(row):
    M, L = _lib()
    c = _c_of(row)
    outs = []
    for via in (False, True):
        a, r, kw, fn = place_combine(c, via_map=via)
        assert fn == (COMBINEMAP if via else COMBINE) and call(L, fn, kw) == M.OK
        a.check()
        outs.append([x.read() for x, g in zip(r["low"], c["low"]) if g] + [x.read() for x in r["high"] if x is not None])
    assert len(outs[0]) == len(outs[1]) and all(same_bits(p, q) for p, q in zip(*outs))


@BOTH
@pytest.mark.parametrize("row", _rows(TAIL), ids=row_id)
def test_text_tail_lp_fp32_outputs_equal_text_tail(row, dtname):
    M, L = _lib()
    c = _c_of(row)
    outs = []
    for lp in (True, False):
        a, r, kw, fn = place_tail(c, dtname, lp=lp)
        assert call(L, fn, kw) == M.OK
        a.check()
        outs.append([r[k].read() for k in ("src", "mu", "logvar", "mask")])
    assert all(same_bits(p, q) for p, q in zip(*outs))


@BOTH
@pytest.mark.parametrize("row", [r for r in _rows(UPHEAD, UPATT) if r[3]["hk"] and r[3]["out"]], ids=row_id)
def test_upblock_feature_image_with_a_head_equals_the_one_without(row, dtname):
    M, L = _lib()
    c = _c_of(row)
    x, w, _s_, _t_, hw = up_inputs(c["B"], c["Cin"], c["H"], c["W"], c["hk"], c["aff"])
    pack, hpack = run_pack(PACKUP, w, dtname), run_pack(PACKTO3, hw, dtname)
    imgs = []
    for plain in (False, True):
        a, r, kw, fn = place_up(dict(c, hk=0) if plain else c, dtname, pack, None if plain else hpack, att=False)
        assert fn == (UP if plain else UPHEAD) and call(L, fn, kw) == M.OK
        a.check()
        imgs.append(r["out"].nchw(c["oco"], 32))
    assert same_bits(*imgs)


# ----------------------------------------------------------------------------------------------------------------------------
# 3: refusals - the documented code in front of the first launch, the whole arena untouched
# ----------------------------------------------------------------------------------------------------------------------------
def _off(name, nbytes):
    """The operand `name` moved `nbytes` off its alignment."""
    return lambda kw: ctypes.c_void_p(kw[name].value + nbytes)


def _arr(name, index, value):
    """The host pointer array `name` with one entry replaced (None, or a region's address plus an offset)."""
    def make(kw):
        vals = list(kw[name])
        vals[index] = value(vals[index]) if callable(value) else value
        return (ctypes.c_void_p * len(vals))(*vals)
    return make


def _ints(name, index, value):
    def make(kw):
        vals = list(kw[name])
        vals[index] = value
        return (ctypes.c_int * len(vals))(*vals)
    return make


GIB = 5263448                    # (4 + 2) (32 + 2) GIB 2 >= 2^31: a channel pitch of the base cases' 4 x 32 image beyond the 2-GiB guard
R_CONV = _c(1, 32, 32, 4, 32, "res", rcp=40, rco=8, ocp=72, oco=32, xcp=32)
R_UP = _u(1, 64, 4, 32, hk=3, ocp=72, oco=0, att=_att(5, "m1"))
R_STEM = _s(1, 32, 4, 32, ocp=72, att=_att(5, "m1"))
R_TO3 = _t(1, 8, 32, 3, ACT_TANH, amap=True)
R_ATTN = _a(2, 4, 32, 5, "m1")
R_COMBINE = _k(1, [(8, 64), (8, 64)], maps=[True, True])
R_TAIL = _x(2, 5, 2, width=6, tdim=64)


def _base(fn, dtname):
    """(arena, named arguments) of a valid call of `fn` on its smallest case, every output placed as one that must stay untouched."""
    _code, td, _ = DTYPES[dtname]
    if fn == CONV:
        a, _r, kw = place_conv(R_CONV, dtname, fake_pack(32 * 32 * 9, td), written=False)
    elif fn in (UP, UPHEAD, UPATT):
        c = dict(R_UP, hk=0 if fn == UP else 3, att=R_UP["att"] if fn == UPATT else None)
        a, _r, kw, got = place_up(c, dtname, fake_pack(64 * 64 * 16, td), fake_pack(3 * 512, td) if c["hk"] else None, written=False)
        assert got == fn
    elif fn in (STEM, STEMATT):
        a, _r, kw, got = place_stem(dict(R_STEM, att=R_STEM["att"] if fn == STEMATT else None), dtname, written=False)
        assert got == fn
    elif fn in (TO3, TO3MAP):
        a, _r, kw, got = place_to3(dict(R_TO3, amap=fn == TO3MAP), dtname, fake_pack(3 * 512, td), written=False)
        assert got == fn
    elif fn == ATTN:
        a, _r, kw, _ = place_attn(R_ATTN, dtname, written=False)
    elif fn in (COMBINE, COMBINEMAP):
        a, _r, kw, got = place_combine(dict(R_COMBINE, maps=R_COMBINE["maps"] if fn == COMBINEMAP else None), written=False, via_map=fn == COMBINEMAP)
        assert got == fn
    elif fn == TAIL:
        a, _r, kw, _ = place_tail(R_TAIL, dtname, written=False)
    elif fn in (FROM, TO):
        a = Arena(DEV)
        x = torch.ones(1, 4, 2, 2)
        if fn == FROM:
            xr, img = a.place_input(x), a.place_lp(td, 1, 2, 2, 8, writes=[(4, 4)], written=False)
            kw = dict(dtype=DTYPES[dtname][0], x=xr.ptr, out=img.ptr, B=1, C=4, H=2, W=2, cpitch=8, coff=4)
        else:
            img, out = a.place_lp(td, 1, 2, 2, 8, reads=[(4, x)]), a.place_output(x.shape, written=False)
            kw = dict(dtype=DTYPES[dtname][0], x=img.ptr, out=out.ptr, B=1, C=4, H=2, W=2, cpitch=8, coff=4)
    elif fn == CONVERT:
        a = Arena(DEV)
        s, d = a.place_input16(torch.ones(16, dtype=torch.float16)), a.place_output16((16,), torch.bfloat16, written=False)
        kw = dict(src_dtype=2, src=s.ptr, dst_dtype=1, dst=d.ptr, n=16)
    elif fn in PACKS:
        shape = {PACK3: (32, 16, 3, 3), PACKUP: (64, 32, 3, 3), PACKTO3: (3, 32, 3, 3)}[fn]
        a = Arena(DEV)
        d0, d1 = pack_dims(fn, torch.empty(shape))
        wr, pk = a.place_input(torch.ones(shape)), a.place_output16((9 * 64 * 64 * 2,), td, written=False)
        kw = dict(dtype=DTYPES[dtname][0], w=wr.ptr, wpack=pk.ptr, d0=d0, d1=d1)
    else:
        assert fn == RESBLOCKS
        a = Arena(DEV)
        x = both(torch.randn(1, 64, 4, 32, generator=_gen(23)))
        imgs = [a.place_lp(td, 1, 4, 32, 64, reads=[(0, x)])] + [a.place_lp(td, 1, 4, 32, 64, writes=[(0, 64)], written=False) for _ in range(3)]
        packs = [a.place_input16(fake_pack(co * 64 * 9, td)) for co in (128, 64, 128, 64)]
        aff = [a.place_input(torch.ones(co)) for co in (128, 64, 128, 64)]
        flags = a.place_output((4 * 1 * 1 * 1 + 1,), written=False, dtype=torch.int32)
        a.buffer()
        kw = dict(dtype=DTYPES[dtname][0], x=imgs[0].ptr, x_cpitch=64, B=1, H=4, W=32, wpack=_ptrs(packs), scale=_ptrs(aff), shift=_ptrs(aff),
                  tmp=imgs[1].ptr, tmp_cpitch=64, a_out=imgs[2].ptr, a_cpitch=64, b_out=imgs[3].ptr, b_cpitch=64, flags=flags.ptr)
    return a, kw


def _null(*names):
    return [("null_" + n, E, {n: None}) for n in names]


def _below_one(*names):
    return [("no_" + n, E, {n: 0}) for n in names]


_ATT_FUSE = [("null_att_pack", E, dict(att_pack=None)), ("no_set", E, dict(att_nsets=0)), ("att_set_negative", E, dict(att_set=-1)),
             ("att_set_beyond_nsets", E, dict(att_set=2)), ("att_pack_off_8_bytes", E, dict(att_pack=_off("att_pack", 8))),
             ("mask_mode_2", E, dict(mask_mode=2)), ("mask_mode_negative", E, dict(mask_mode=-1)),
             ("no_word", U, dict(T=0)), ("words_33", U, dict(T=33)), ("c_coff_negative", U, dict(out_coff=32, c_coff=-8)), ("c_coff_not_x4", U, dict(c_coff=34)),
             ("c_coff_beyond_pitch", U, dict(c_coff=48)), ("c_code_over_h", U, dict(c_coff=16)), ("c_code_over_h_from_below", U, dict(out_coff=8, c_coff=0))]
_UPCOMMON = _null("x", "wpack") + _below_one("B", "H", "W") + [
    ("scale_without_shift", E, dict(shift=None)), ("shift_without_scale", E, dict(scale=None)), ("unknown_dtype", E, dict(dtype=3)),
    ("cout_128", U, dict(Cout=128)), ("cin_48", U, dict(Cin=48)), ("w_not_x32", U, dict(W=48)), ("h_not_x4", U, dict(H=6)),
    ("x_cpitch_below_cin", U, dict(x_cpitch=56)), ("x_cpitch_not_x8", U, dict(x_cpitch=68)), ("x_off_8_bytes", U, dict(x=_off("x", 8))),
    ("wpack_off_8_bytes", U, dict(wpack=_off("wpack", 8))), ("out_cpitch_not_x8", U, dict(out_cpitch=68)), ("out_coff_negative", U, dict(out_coff=-8)),
    ("out_coff_not_x8", U, dict(out_coff=4)), ("out_coff_beyond_pitch", U, dict(out_coff=48)), ("out_off_8_bytes", U, dict(out=_off("out", 8))),
    ("out_2gib", U, dict(out_cpitch=GIB))]
_UPHEADS = [("head_wpack_off_8_bytes", U, dict(head_wpack=_off("head_wpack", 8))), ("null_head_wpack", E, dict(head_wpack=None)),
            ("head_k_4", E, dict(head_k=4)), ("head_k_7", E, dict(head_k=7))]
_STEMCOMMON = _null("x", "w", "scale", "shift", "out") + _below_one("B", "H", "W") + [
    ("c_below_8", E, dict(C=4)), ("c_not_x8", U, dict(C=12)), ("c_above_64", U, dict(C=72, out_cpitch=144)), ("out_cpitch_not_x8", U, dict(out_cpitch=76)),
    ("out_coff_negative", U, dict(out_coff=-8)), ("out_coff_not_x8", U, dict(out_coff=4)), ("out_coff_beyond_pitch", U, dict(out_coff=48)),
    ("out_off_8_bytes", U, dict(out=_off("out", 8))), ("unknown_dtype", E, dict(dtype=0))]
_TO3COMMON = _null("x", "wpack", "out") + _below_one("B", "H", "W") + [
    ("cin_64", U, dict(Cin=64)), ("kernel_4", U, dict(K=4)), ("kernel_7", U, dict(K=7)), ("w_not_x32", U, dict(W=48)), ("h_not_x8", U, dict(H=12)),
    ("x_cpitch_below_32", U, dict(x_cpitch=24)), ("x_cpitch_not_x8", U, dict(x_cpitch=36)), ("x_off_8_bytes", U, dict(x=_off("x", 8))),
    ("wpack_off_8_bytes", U, dict(wpack=_off("wpack", 8))), ("unknown_dtype", E, dict(dtype=3))]
_COMBINECOMMON = [("no_scale", E, dict(nscales=0)), ("five_scales", E, dict(nscales=5))] + _below_one("B") + _null(
    "H", "W", "partial_low", "partial_high", "low", "high") + [
    ("h_below_8", U, dict(H=_ints("H", 1, 4))), ("w_below_64", U, dict(W=_ints("W", 0, 32))), ("h_not_x8", U, dict(H=_ints("H", 0, 12))),
    ("w_not_x64", U, dict(W=_ints("W", 1, 96))), ("null_low_of_a_scale", E, dict(low=_arr("low", 1, None))),
    ("partial_high_without_high", E, dict(high=_arr("high", 0, None))), ("low_off_8_bytes", U, dict(low=_arr("low", 0, lambda v: v + 8))),
    ("high_off_4_bytes", U, dict(high=_arr("high", 1, lambda v: v + 4))), ("too_many_pixels", U, dict(B=2 ** 30))]
_PACKCOMMON = _null("w", "wpack") + [("unknown_dtype", E, dict(dtype=3))]
_TAILNULLS = _null("words", "w_ctx", "src_out", "sent_emb", "ca_w", "ca_b", "mu", "logvar", "captions", "mask", "att_pack")
_RB = ["x", "tmp", "a_out", "b_out"]
REFUSALS = {
    FROM: _null("x", "out") + _below_one("B", "C", "H", "W") + [("coff_negative", E, dict(coff=-4, cpitch=16)), ("coff_beyond_pitch", E, dict(coff=6)),
                                                             ("unknown_dtype", E, dict(dtype=0))],
    TO: _null("x", "out") + _below_one("B", "C", "H", "W") + [("coff_negative", E, dict(coff=-4, cpitch=16)), ("coff_beyond_pitch", E, dict(coff=6)),
                                                           ("unknown_dtype", E, dict(dtype=3))],
    CONVERT: _null("src", "dst") + [("fewer_than_8", E, dict(n=0)), ("n_not_x8", E, dict(n=12)), ("same_type", E, dict(dst_dtype=2)),
                                    ("unknown_type", E, dict(src_dtype=3)), ("src_off_8_bytes", E, dict(src=_off("src", 8))),
                                    ("dst_off_8_bytes", E, dict(dst=_off("dst", 8)))],
    PACK3: _PACKCOMMON + _below_one("d0", "d1") + [("cout_not_x32", U, dict(d0=48)), ("cin_not_x16", U, dict(d1=24))],
    PACKUP: _PACKCOMMON + [("cout_128", U, dict(d0=128)), ("cin_48", U, dict(d1=48)), ("cin_16", U, dict(d1=16))],
    PACKTO3: _PACKCOMMON + [("cin_64", U, dict(d0=64)), ("kernel_4", U, dict(d1=4)), ("kernel_1", U, dict(d1=1))],
    CONV: _null("x", "wpack", "out") + _below_one("B", "H", "W") + [
        ("scale_without_shift", E, dict(shift=None)), ("shift_without_scale", E, dict(scale=None)), ("unknown_epilogue", E, dict(epilogue=2)),
        ("glu_with_residual", E, dict(epilogue=1)), ("unknown_dtype", E, dict(dtype=3)), ("w_not_x32", U, dict(W=48)), ("h_not_x4", U, dict(H=6)),
        ("x_cpitch_below_cin", U, dict(x_cpitch=24)), ("x_cpitch_not_x8", U, dict(x_cpitch=36)), ("out_cpitch_not_x8", U, dict(out_cpitch=76)),
        ("out_coff_negative", U, dict(out_coff=-8)), ("out_coff_not_x8", U, dict(out_coff=36)), ("out_coff_beyond_pitch", U, dict(out_coff=48)),
        ("res_cpitch_not_x8", U, dict(res_cpitch=44)), ("res_coff_negative", U, dict(res_coff=-8)), ("res_coff_not_x8", U, dict(res_coff=4)),
        ("res_coff_beyond_pitch", U, dict(res_coff=16)), ("x_off_8_bytes", U, dict(x=_off("x", 8))), ("wpack_off_8_bytes", U, dict(wpack=_off("wpack", 8))),
        ("out_off_8_bytes", U, dict(out=_off("out", 8))), ("residual_off_8_bytes", U, dict(residual=_off("residual", 8))),
        ("x_2gib", U, dict(x_cpitch=GIB)), ("out_2gib", U, dict(out_cpitch=GIB)), ("res_2gib", U, dict(res_cpitch=GIB)),
        ("cin_16", U, dict(Cin=16)), ("cin_64_cout_32", U, dict(Cin=64, x_cpitch=64)), ("cout_96", U, dict(Cout=96, out_cpitch=160, res_cpitch=112)),
        ("glu_cout_32", U, dict(epilogue=1, residual=None)), ("upsample_without_glu", U, dict(upsample=1))],
    UP: _UPCOMMON + _null("out"),
    UPHEAD: _UPCOMMON + _UPHEADS + _null("head_partial"),
    UPATT: _UPCOMMON + _UPHEADS[:1] + _ATT_FUSE + [("no_image", U, dict(out=None)), ("cin_32", U, dict(Cin=32)), ("head_k_5", U, dict(head_k=5)),
                                                   ("neither_image_nor_head", E, dict(out=None, head_partial=None))],
    COMBINE: _COMBINECOMMON,
    COMBINEMAP: _COMBINECOMMON + [("amap_off_8_bytes", U, dict(amap=_arr("amap", 1, lambda v: v + 8)))],
    STEM: _STEMCOMMON,
    STEMATT: _STEMCOMMON + [t for t in _ATT_FUSE if t[0] != "c_code_over_h_from_below"] + [
        ("c_code_over_h_from_below", U, dict(out_coff=32, c_coff=28)), ("c_24", U, dict(C=24)), ("w_not_x32", U, dict(W=40))],
    TO3: _TO3COMMON + [("act_ident_axpy", E, dict(act=2)), ("unknown_act", E, dict(act=3))],
    TO3MAP: _TO3COMMON + [("unknown_act", E, dict(act=3)), ("map_with_act_none", E, dict(act=0))],
    ATTN: _null("h", "src", "c_img") + _below_one("B", "T", "H", "W") + [
        ("mask_mode_2", E, dict(mask_mode=2)), ("mask_mode_negative", E, dict(mask_mode=-1)), ("unknown_dtype", E, dict(dtype=3)),
        ("idf_64", U, dict(idf=64)), ("words_33", U, dict(T=33)), ("w_not_x32", U, dict(W=48)), ("h_cpitch_below_32", U, dict(h_cpitch=24)),
        ("h_cpitch_not_x8", U, dict(h_cpitch=68)), ("c_cpitch_not_x4", U, dict(c_cpitch=66)), ("c_coff_negative", U, dict(c_coff=-4)),
        ("c_coff_not_x4", U, dict(c_coff=30)), ("c_coff_beyond_pitch", U, dict(c_coff=36)), ("h_off_8_bytes", U, dict(h=_off("h", 8), c_img=_off("c_img", 8))),
        ("c_img_off_4_bytes", U, dict(c_img=_off("c_img", 4))), ("c_code_over_h", U, dict(c_coff=0)), ("c_code_over_h_partly", U, dict(c_coff=28))],
    TAIL: _TAILNULLS + _below_one("nsets", "B", "cdf", "T", "tdim", "ncf") + [
        ("width_below_t", E, dict(width=4)), ("five_sets", U, dict(nsets=5)), ("words_33", U, dict(T=33, width=33)), ("idf_16", U, dict(idf=16)),
        ("idf_48", U, dict(idf=48)), ("idf_64_with_a_pack", U, dict(idf=64)), ("tdim_not_x16", U, dict(tdim=24)),
        ("sent_emb_off_8_bytes", U, dict(sent_emb=_off("sent_emb", 8))), ("ca_w_off_4_bytes", U, dict(ca_w=_off("ca_w", 4))),
        ("null_w_ctx_of_a_set", E, dict(w_ctx=_arr("w_ctx", 1, None))), ("unknown_lp_dtype", U, dict(lp_dtype=0)),
        ("att_pack_off_8_bytes", U, dict(att_pack=_off("att_pack", 8)))],
    RESBLOCKS: _null("x", "wpack", "scale", "shift", "tmp", "a_out", "b_out", "flags") + _below_one("B", "H", "W") + [
        ("unknown_dtype", E, dict(dtype=3)), ("w_not_x32", U, dict(W=48)), ("h_not_x4", U, dict(H=6))] + [
        ("%s_cpitch_below_64" % n, U, {n + "_cpitch" if n != "a_out" and n != "b_out" else n[0] + "_cpitch": 56}) for n in _RB] + [
        ("%s_cpitch_not_x8" % n, U, {n + "_cpitch" if n != "a_out" and n != "b_out" else n[0] + "_cpitch": 68}) for n in _RB] + [
        ("%s_off_8_bytes" % n, U, {n: _off(n, 8)}) for n in _RB] + [
        ("null_wpack_of_a_layer", E, dict(wpack=_arr("wpack", 2, None))), ("wpack_of_a_layer_off_8_bytes", E, dict(wpack=_arr("wpack", 1, lambda v: v + 8))),
        ("scale_without_shift_of_a_layer", E, dict(shift=_arr("shift", 3, None))), ("tmp_is_x", E, dict(tmp=lambda kw: kw["x"])),
        ("tmp_is_a_out", E, dict(tmp=lambda kw: kw["a_out"])), ("tmp_is_b_out", E, dict(tmp=lambda kw: kw["b_out"])),
        ("a_out_is_x", E, dict(a_out=lambda kw: kw["x"])), ("a_out_is_b_out", E, dict(a_out=lambda kw: kw["b_out"])), ("image_2gib", U, dict(b_cpitch=GIB))],
}


def refusals():
    """[(name, call, expected code)]: call(dtname) -> (the code the entry gave, the arena it was given)."""
    out = []
    for fn, specs in REFUSALS.items():
        for tag, code, over in specs:
            def run(dtname, fn=fn, over=over):
                _M, L = _lib()
                a, kw = _base(fn, dtname)
                new = {k: (v(kw) if callable(v) else v) for k, v in over.items()}
                assert set(new) <= set(kw), "an argument the entry does not take"
                kw.update(new)
                return call(L, fn, kw), a
            out.append(("%s-%s" % (fn[5:], tag), run, code))
    return out


@pytest.mark.parametrize("name", [n for n, _run, _code in refusals()])
def test_refusal(name):
    (run, code), = [(r, c) for n, r, c in refusals() if n == name]
    for dtname in DTYPES:
        rc, a = run(dtname)
        assert rc == code, "%s (%s) gave %d, not %d" % (name, dtname, rc, code)
        a.check()                                               # every operand, every guard band: untouched
