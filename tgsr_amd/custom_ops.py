"""`torch.ops.tgsr.*`: the HIP entry points as PyTorch-ROCm custom operators (BASELINE.json north_star: "driven from
Python through PyTorch-ROCm custom ops over a thin C-ABI").

Each op is a schema in the `tgsr` namespace whose CUDA(=HIP) kernel is the ctypes call into libtgsr_hip.so
(`tgsr_amd.ops`), plus a fake (meta) kernel for shape propagation and - for the two differentiable ones below - an
autograd formula registered with `torch.library.register_autograd` whose backward is itself a `tgsr::` op.  The drop-in
modules (`tgsr_amd.util`) call these operators, not the ctypes wrappers directly.

Registered through `torch.library.Library.define / impl` rather than the `@custom_op` decorator: measured on this
torch build the decorator's Python wrapper costs ~11 us per call against ~2 us for a Library-registered op, and one SR
forward issues ~60 of them (0.7 ms of host time per 1.7 ms step otherwise).

Functional ops return fresh tensors; the `*_out` variants write into a caller-provided channel-slice view (how the
reference's torch.cat((h_code, c_code), 1), util.py:771/817, disappears) and are declared as mutating that argument.
"""
from typing import Optional

import torch

from . import lp, ops

_lib = torch.library.Library("tgsr", "DEF")
_T = torch.Tensor


def _refuse_cpu(name):
    def kernel(*args, **kwargs):
        raise ops.TgsrError("torch.ops.tgsr.%s got CPU tensors: tgsr_amd ops run only on HIP tensors; there is no CPU fallback" % name)
    return kernel


def _define(schema, fn, fake=None):
    name = schema.split("(")[0]
    _lib.define(schema)
    _lib.impl(name, fn, "CUDA")
    _lib.impl(name, _refuse_cpu(name), "CPU")        # a loud refusal (the same TgsrError the ctypes wrappers raise), not a fallback
    if fake is not None:
        torch.library.register_fake("tgsr::" + name, fake, lib=_lib)
    return getattr(torch.ops.tgsr, name).default


def _co(cout, glu):
    return cout // 2 if glu else cout


# ------------------------------------------------------------------------------------------------ conv3x3, every kernel form
# One operator family per row of ops.FORMS: `op` (functional), `op`_out (into a channel-slice view), `op`_stats where the form has
# the BatchNorm-statistics epilogue, `op_plain` (the un-gated up-sampling convolution of training) and `pack_op`.
def _pack_fake(form, w, dgrad):
    return w.new_empty(ops.packed_elems(form, w.shape[1], w.shape[0]) if dgrad else ops.packed_elems(form, w.shape[0], w.shape[1]))


def _define_form(f):
    form, g = f.name, globals()
    pack = "upack" if "wino" in form else "wpack"          # the schema's name for the Winograd-transformed / the re-ordered weights
    run = ops._conv3x3
    if f.up:           # upBlock forms: gated, the affine required, no residual
        sig = "Tensor x, Tensor %s, int cout, Tensor scale, Tensor shift" % pack
        fn = lambda x, p, cout, s, t: run(form, x, p, cout, s, t, True, True, None, None)                          # noqa: E731
        fn_out = lambda x, p, cout, s, t, out: (run(form, x, p, cout, s, t, True, True, None, out), None)[1]      # noqa: E731
        fake = lambda x, p, cout, s, t: x.new_empty(x.shape[0], cout // 2, 2 * x.shape[2], 2 * x.shape[3])        # noqa: E731
    elif f.tail == "epi,up":
        sig = "Tensor x, Tensor %s, int cout, Tensor? scale, Tensor? shift, bool glu, bool upsample, Tensor? residual" % pack
        fn = lambda x, p, cout, s, t, glu, up, res: run(form, x, p, cout, s, t, glu, up, res, None)               # noqa: E731
        fn_out = lambda x, p, cout, s, t, glu, up, res, out: (run(form, x, p, cout, s, t, glu, up, res, out), None)[1]   # noqa: E731
        fake = lambda x, p, cout, s, t, glu, up, res: x.new_empty(x.shape[0], _co(cout, glu), x.shape[2] * (2 if up else 1),   # noqa: E731
                                                                  x.shape[3] * (2 if up else 1))
    else:
        sig = "Tensor x, Tensor %s, int cout, Tensor? scale, Tensor? shift, bool glu, Tensor? residual" % pack
        fn = lambda x, p, cout, s, t, glu, res: run(form, x, p, cout, s, t, glu, False, res, None)                # noqa: E731
        fn_out = lambda x, p, cout, s, t, glu, res, out: (run(form, x, p, cout, s, t, glu, False, res, out), None)[1]    # noqa: E731
        fake = lambda x, p, cout, s, t, glu, res: x.new_empty(x.shape[0], _co(cout, glu), x.shape[2], x.shape[3])  # noqa: E731
    g[f.op] = _define("%s(%s) -> Tensor" % (f.op, sig), fn, fake)
    g[f.op + "_out"] = _define("%s_out(%s, Tensor(a!) out) -> ()" % (f.op, sig), fn_out, lambda *a: None)
    if f.op_plain is not None:
        g[f.op_plain] = _define("%s(Tensor x, Tensor %s, int cout, Tensor? scale, Tensor? shift, bool glu) -> Tensor" % (f.op_plain, pack),
                                lambda x, p, cout, s, t, glu: run(form, x, p, cout, s, t, glu, True, None, None),
                                lambda x, p, cout, s, t, glu: x.new_empty(x.shape[0], _co(cout, glu), 2 * x.shape[2], 2 * x.shape[3]))
    if f.stats is not None:
        g[f.op + "_stats"] = _define(
            "%s_stats(Tensor x, Tensor %s, int cout) -> (Tensor, Tensor)" % (f.op, pack),
            lambda x, p, cout: run(form, x, p, cout, None, None, False, False, None, None, True),
            lambda x, p, cout: (x.new_empty(x.shape[0], cout, x.shape[2], x.shape[3]),
                                x.new_empty(cout, ops.stats_nslots(form, x.shape[0], x.shape[2], x.shape[3], cout), 2)))
    # the pack operator's schema names the flags the form's pack has: a data-gradient pack (`dgrad`), the gate grouping (`glu`)
    if f.pack_op is None:
        return
    if f.pack_arg == "k":
        g[f.pack_op] = _define("%s(Tensor w, bool dgrad) -> Tensor" % f.pack_op, lambda w, d: ops.pack_weight(form, w, False, d),
                               lambda w, d: _pack_fake(form, w, d))
    elif f.pack_dgrad is not None:
        g[f.pack_op] = _define("%s(Tensor w, bool glu, bool dgrad) -> Tensor" % f.pack_op, lambda w, gl, d: ops.pack_weight(form, w, gl, d),
                               lambda w, gl, d: _pack_fake(form, w, d))
    else:
        g[f.pack_op] = _define("%s(Tensor w, bool glu) -> Tensor" % f.pack_op, lambda w, gl: ops.pack_weight(form, w, gl),
                               lambda w, gl: _pack_fake(form, w, False))


for _f in ops.FORMS.values():
    _define_form(_f)


def _caller(f):
    """`f`'s operators behind ONE signature, for the callers that hold ops.conv3x3_form's answer: into `out` (a channel-slice view)
    where one is given.  Built once per form; the operators are looked up in this module by name at each call."""
    g, op, op_out, op_plain = globals(), f.op, f.op + "_out", f.op_plain
    if f.up:
        def call(x, pack, cout, scale, shift, glu=False, upsample=True, residual=None, out=None):
            assert residual is None
            if not glu:
                return g[op_plain](x, pack, cout, scale, shift, False)
            if out is None:
                return g[op](x, pack, cout, scale, shift)
            g[op_out](x, pack, cout, scale, shift, out)
            return out
    elif f.tail == "epi,up":
        def call(x, pack, cout, scale, shift, glu=False, upsample=False, residual=None, out=None):
            if out is None:
                return g[op](x, pack, cout, scale, shift, glu, upsample, residual)
            g[op_out](x, pack, cout, scale, shift, glu, upsample, residual, out)
            return out
    else:
        def call(x, pack, cout, scale, shift, glu=False, upsample=False, residual=None, out=None):
            if out is None:
                return g[op](x, pack, cout, scale, shift, glu, residual)
            g[op_out](x, pack, cout, scale, shift, glu, residual, out)
            return out
    return call


# form -> f(x, pack, cout, scale, shift, glu, upsample, residual, out): the layer on that kernel form
CONV3X3 = {f.name: _caller(f) for f in ops.FORMS.values()}


_STATS_OP = {f.name: f.op + "_stats" for f in ops.FORMS.values() if f.stats is not None}


def conv3x3_stats(form, x, pack, cout):
    """`form`'s raw convolution with BatchNorm's partial sums in its epilogue: (raw, stat_partial)."""
    return globals()[_STATS_OP[form]](x, pack, cout)


# ------------------------------------------------------------------------------------------------ word attention
def _word_attention(h, words, w_ctx, mask, correct_mask, src):
    return ops.word_attention(h, words, w_ctx, mask, correct_mask, src=src)


def _word_attention_fake(h, words, w_ctx, mask, correct_mask, src):
    return torch.empty_like(h), h.new_empty(h.shape[0], words.shape[2], h.shape[2], h.shape[3])


def _word_attention_out(h, words, w_ctx, mask, correct_mask, src, out):
    return ops.word_attention(h, words, w_ctx, mask, correct_mask, out=out, src=src)[1]


word_attention = _define("word_attention(Tensor h, Tensor words, Tensor w_ctx, Tensor? mask, bool correct_mask, "
                         "Tensor? src) -> (Tensor, Tensor)", _word_attention, _word_attention_fake)
word_attention_out = _define("word_attention_out(Tensor h, Tensor words, Tensor w_ctx, Tensor? mask, bool correct_mask, "
                             "Tensor? src, Tensor(a!) out) -> Tensor", _word_attention_out,
                             lambda h, words, w_ctx, mask, cm, src, out:
                             h.new_empty(h.shape[0], words.shape[2], h.shape[2], h.shape[3]))


word_project = _define("word_project(Tensor words, Tensor[] w_ctxs) -> Tensor[]", lambda words, ws: ops.word_project(words, list(ws)),
                       lambda words, ws: list(words.new_empty(len(ws), words.shape[0], ws[0].shape[0], 32).unbind(0)))


# ------------------------------------------------------------------------------------------------ image heads (differentiable)
def _conv_to3(x, w, tanh_axpy, addend, alpha):
    return ops.conv_to3(x, w, tanh_axpy=tanh_axpy, addend=addend, alpha=alpha)


def _conv_to3_bwd(dy, out, addend, alpha, x, w, tanh_axpy, need_dx, need_dw):
    """(dx, dw) of conv_to3; a gradient that is not needed comes back as an empty tensor."""
    dx, dw = ops.conv_to3_bwd(dy, out, addend, alpha, x, w, tanh_axpy, need_dx, need_dw)
    return (dx if dx is not None else x.new_empty(0)), (dw if dw is not None else x.new_empty(0))


conv_to3 = _define("conv_to3(Tensor x, Tensor w, bool tanh_axpy, Tensor? addend, float alpha) -> Tensor", _conv_to3,
                   lambda x, w, tanh_axpy, addend, alpha: x.new_empty(x.shape[0], 3, x.shape[2], x.shape[3]))
conv_to3_bwd = _define("conv_to3_bwd(Tensor dy, Tensor? out, Tensor? addend, float alpha, Tensor x, Tensor w, bool tanh_axpy, "
                       "bool need_dx, bool need_dw) -> (Tensor, Tensor)", _conv_to3_bwd,
                       lambda dy, out, addend, alpha, x, w, t, ndx, ndw:
                       (torch.empty_like(x) if ndx else x.new_empty(0), torch.empty_like(w) if ndw else x.new_empty(0)))


def _conv_to3_setup(ctx, inputs, output):
    x, w, tanh_axpy, addend, alpha = inputs
    ctx.save_for_backward(x, w, output if tanh_axpy else None, addend)
    ctx.tanh_axpy, ctx.alpha = tanh_axpy, alpha


def _conv_to3_backward(ctx, dy):
    x, w, out, addend = ctx.saved_tensors
    ndx, ndw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    dx = dw = None
    if ndx or ndw:
        dx, dw = conv_to3_bwd(dy, out, addend, ctx.alpha, x, w, ctx.tanh_axpy, ndx, ndw)
    dadd = dy * ctx.alpha if (addend is not None and ctx.needs_input_grad[3]) else None
    return (dx if ndx else None), (dw if ndw else None), None, dadd, None


torch.library.register_autograd("tgsr::conv_to3", _conv_to3_backward, setup_context=_conv_to3_setup, lib=_lib)


# ------------------------------------------------------------------------------------------------ downBlock conv (differentiable)
conv4x4s2 = _define("conv4x4s2(Tensor x, Tensor w, bool leaky) -> Tensor",
                    lambda x, w, leaky: ops.conv4x4s2(x, w, leaky=leaky),
                    lambda x, w, leaky: x.new_empty(x.shape[0], w.shape[0], x.shape[2] // 2, x.shape[3] // 2))
conv4x4s2_dgrad = _define("conv4x4s2_dgrad(Tensor dy, Tensor w, int H, int W) -> Tensor",
                          lambda dy, w, H, W: ops.conv4x4s2_dgrad(dy, w, H, W),
                          lambda dy, w, H, W: dy.new_empty(dy.shape[0], w.shape[1], H, W))
conv4x4s2_wgrad = _define("conv4x4s2_wgrad(Tensor dy, Tensor x) -> Tensor",
                          lambda dy, x: ops.conv4x4s2_wgrad(dy, x),
                          lambda dy, x: dy.new_empty(dy.shape[1], x.shape[1], 4, 4))
leaky_relu_bwd = _define("leaky_relu_bwd(Tensor dy, Tensor y) -> Tensor", lambda dy, y: ops.leaky_relu_bwd(dy, y),
                         lambda dy, y: torch.empty_like(dy))


def _conv4x4s2_setup(ctx, inputs, output):
    x, w, leaky = inputs
    ctx.save_for_backward(x, w, output if leaky else None)


def _conv4x4s2_backward(ctx, dy):
    x, w, out = ctx.saved_tensors
    g = dy.contiguous() if out is None else leaky_relu_bwd(dy.contiguous(), out)
    dx = conv4x4s2_dgrad(g, w, x.shape[2], x.shape[3]) if ctx.needs_input_grad[0] else None
    dw = conv4x4s2_wgrad(g, x.contiguous()) if ctx.needs_input_grad[1] else None
    return dx, dw, None


torch.library.register_autograd("tgsr::conv4x4s2", _conv4x4s2_backward, setup_context=_conv4x4s2_setup, lib=_lib)


# ------------------------------------------------------------------------------------------------ stand-alone GLU (differentiable)
glu = _define("glu(Tensor x) -> Tensor", lambda x: ops.glu(x),
              lambda x: x.new_empty((x.shape[0], x.shape[1] // 2) + tuple(x.shape[2:])))
glu_bwd = _define("glu_bwd(Tensor dy, Tensor x) -> Tensor", lambda dy, x: ops.glu_bwd(dy, x), lambda dy, x: torch.empty_like(x))
torch.library.register_autograd("tgsr::glu", lambda ctx, dy: glu_bwd(dy, ctx.saved_tensors[0]),
                                setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0]), lib=_lib)


# ================================================================================================ training primitives
# The blocks of tgsr_amd.autograd (ConvBnAct, ResBlockFn, ConvBnLeaky) are formulas over these operators; gradient
# tensors that must land in a given place (a slot of the flat gradient bucket, parallel.grad_slot) are mutable arguments.
def _bn_train_fwd(raw, gamma, beta, eps, momentum, running_mean, running_var, act, residual, nbt):
    return ops.bn_train_fwd(raw, gamma, beta, eps, momentum, running_mean, running_var, act, residual, nbt)


bn_train_fwd = _define("bn_train_fwd(Tensor raw, Tensor gamma, Tensor beta, float eps, float momentum, Tensor(a!)? running_mean, "
                       "Tensor(b!)? running_var, int act, Tensor? residual, Tensor(c!)? num_batches_tracked) -> (Tensor, Tensor)",
                       _bn_train_fwd,
                       lambda raw, g, b, eps, mom, rm, rv, act, res, nbt:
                       (raw.new_empty(raw.shape[0], raw.shape[1] // 2 if act == 1 else raw.shape[1], raw.shape[2], raw.shape[3]),
                        raw.new_empty(4, raw.shape[1])))
bn_train_fwd_from_stats = _define(
    "bn_train_fwd_from_stats(Tensor raw, Tensor gamma, Tensor beta, float eps, float momentum, Tensor(a!)? running_mean, "
    "Tensor(b!)? running_var, int act, Tensor? residual, Tensor(c!)? num_batches_tracked, Tensor stat_partial) -> (Tensor, Tensor)",
    lambda raw, g, b, eps, mom, rm, rv, act, res, nbt, sp: ops.bn_train_fwd(raw, g, b, eps, mom, rm, rv, act, res, nbt, stat_partial=sp),
    lambda raw, g, b, eps, mom, rm, rv, act, res, nbt, sp:
    (raw.new_empty(raw.shape[0], raw.shape[1] // 2 if act == 1 else raw.shape[1], raw.shape[2], raw.shape[3]),
     raw.new_empty(4, raw.shape[1])))
bn_train_fwd_out = _define("bn_train_fwd_out(Tensor raw, Tensor gamma, Tensor beta, float eps, float momentum, "
                           "Tensor(a!)? running_mean, Tensor(b!)? running_var, int act, Tensor(c!)? num_batches_tracked, "
                           "Tensor(d!) out, Tensor(e!) stats) -> ()",
                           lambda raw, g, b, eps, mom, rm, rv, act, nbt, out, stats:
                           (ops.bn_train_fwd(raw, g, b, eps, mom, rm, rv, act, None, nbt, out=out, stats=stats), None)[1],
                           lambda *a: None)
bn_train_bwd = _define("bn_train_bwd(Tensor dout, Tensor raw, Tensor stats, int act, Tensor(a!) dgamma, Tensor(b!) dbeta, "
                       "Tensor(c!)? draw) -> Tensor",
                       lambda dout, raw, stats, act, dg, db, draw: ops.bn_train_bwd(dout, raw, stats, act, dg, db, draw)[0]
                       if draw is None else (ops.bn_train_bwd(dout, raw, stats, act, dg, db, draw), raw.new_empty(0))[1],
                       lambda dout, raw, stats, act, dg, db, draw: torch.empty_like(raw) if draw is None else raw.new_empty(0))
conv3x3_wgrad = _define("conv3x3_wgrad(Tensor draw, Tensor x, bool upsample, bool winograd, Tensor(a!) dw) -> ()",
                        lambda draw, x, up, wino, dw: (ops.conv3x3_wgrad(draw, x, up, wino, out=dw), None)[1], lambda *a: None)
sumpool2x2 = _define("sumpool2x2(Tensor x) -> Tensor", lambda x: ops.sumpool2x2(x),
                     lambda x: x.new_empty(x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2))
conv3x3_gemm = _define("conv3x3_gemm(Tensor x, Tensor w) -> Tensor", lambda x, w: ops.conv3x3_gemm(x, w),
                       lambda x, w: x.new_empty(x.shape[0], w.shape[0], x.shape[2], x.shape[3]))
conv3x3_gemm_dgrad = _define("conv3x3_gemm_dgrad(Tensor dy, Tensor w) -> Tensor", lambda dy, w: ops.conv3x3_gemm_dgrad(dy, w),
                             lambda dy, w: dy.new_empty(dy.shape[0], w.shape[1], dy.shape[2], dy.shape[3]))
conv3x3_gemm_wgrad_out = _define("conv3x3_gemm_wgrad_out(Tensor dy, Tensor x, Tensor(a!) dw) -> ()",
                                 lambda dy, x, dw: (ops.conv3x3_gemm_wgrad(dy, x, out=dw), None)[1], lambda *a: None)
conv4x4s2_wgrad_out = _define("conv4x4s2_wgrad_out(Tensor dy, Tensor x, Tensor(a!) dw) -> ()",
                              lambda dy, x, dw: (ops.conv4x4s2_wgrad(dy, x, out=dw), None)[1], lambda *a: None)


# ------------------------------------------------------------------------------------------------ word attention backward
word_attention_bwd = _define("word_attention_bwd(Tensor h, Tensor src, Tensor? mask, bool correct_mask, int T, Tensor dc) -> "
                             "(Tensor, Tensor)",
                             lambda h, src, mask, cm, T, dc: ops.word_attention_bwd(h, src, mask, cm, T, dc),
                             lambda h, src, mask, cm, T, dc: (torch.empty_like(h), h.new_empty(h.shape[0], h.shape[1], T)))


# ------------------------------------------------------------------------------------------------ logit heads (row dot)
rowdot = _define("rowdot(Tensor x, Tensor w, Tensor? bias) -> Tensor", lambda x, w, b: ops.rowdot(x, w, b),
                 lambda x, w, b: x.new_empty(x.shape[0]))


def _rowdot_bwd(dy, x, w, need_dx, need_dw):
    dx, dw = ops.rowdot_bwd(dy, x, w, need_dx, need_dw)
    return (dx if dx is not None else x.new_empty(0)), (dw if dw is not None else x.new_empty(0))


rowdot_bwd = _define("rowdot_bwd(Tensor dy, Tensor x, Tensor w, bool need_dx, bool need_dw) -> (Tensor, Tensor)", _rowdot_bwd,
                     lambda dy, x, w, ndx, ndw: (torch.empty_like(x) if ndx else x.new_empty(0),
                                                 x.new_empty(x.shape[1]) if ndw else x.new_empty(0)))


def _rowdot_backward(ctx, dy):
    x, w = ctx.saved_tensors
    ndx, ndw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    dx = dw = None
    if ndx or ndw:
        dx, dw = rowdot_bwd(dy, x, w, ndx, ndw)
    return (dx if ndx else None), (dw.reshape(w.shape) if ndw else None), (dy.sum().reshape(1) if ctx.needs_input_grad[2] else None)


torch.library.register_autograd("tgsr::rowdot", _rowdot_backward,
                                setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0], inputs[1]), lib=_lib)


# ------------------------------------------------------------------------------------------------ GEMM heads (differentiable)
linear = _define("linear(Tensor x, Tensor w, Tensor? bias) -> Tensor", lambda x, w, b: ops.linear(x, w, b),
                 lambda x, w, b: x.new_empty(x.shape[0], w.shape[0]))
conv1x1 = _define("conv1x1(Tensor x, Tensor w) -> Tensor", lambda x, w: ops.conv1x1(x, w),
                  lambda x, w: x.new_empty(x.shape[0], w.shape[0], x.shape[2], x.shape[3]))


def _gemm_nt(a, b):
    """a [M,K] @ b[N,K]^T on the HIP GEMM kernel."""
    return linear(a.contiguous(), b.contiguous(), None)


def _linear_backward(ctx, dy):
    x, w = ctx.saved_tensors
    dy = dy.contiguous()
    dx = _gemm_nt(dy, w.detach().t()) if ctx.needs_input_grad[0] else None          # [B,N] @ W [N,K]
    dw = _gemm_nt(dy.t(), x.detach().t()) if ctx.needs_input_grad[1] else None      # dy^T x
    return dx, dw, (dy.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None)


def _linear_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.has_bias = inputs[2] is not None


torch.library.register_autograd("tgsr::linear", _linear_backward, setup_context=_linear_setup, lib=_lib)


def _conv1x1_backward(ctx, dy):
    x, w = ctx.saved_tensors
    Cout, Cin = w.shape[0], w.shape[1]
    dy = dy.contiguous()
    dx = dw = None
    if ctx.needs_input_grad[0]:                                    # (the frozen trunk's features need none)
        dx = conv1x1(dy, w.detach().reshape(Cout, Cin).t().contiguous())
    if ctx.needs_input_grad[1]:
        dw = ops.conv1x1_wgrad(dy, x.detach())                     # the implicit-GEMM kernel where the shape qualifies
        if dw is None:
            dy2 = dy.permute(1, 0, 2, 3).reshape(Cout, -1)         # [Cout, B*S]
            x2 = x.detach().permute(1, 0, 2, 3).reshape(Cin, -1)   # [Cin,  B*S]
            dw = _gemm_nt(dy2, x2)
        dw = dw.reshape(w.shape)
    return dx, dw


torch.library.register_autograd("tgsr::conv1x1", _conv1x1_backward,
                                setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0], inputs[1]), lib=_lib)


# ------------------------------------------------------------------------------------------------ text encoder
bilstm_table = _define("bilstm_table(Tensor captions, int[] cap_lens, Tensor table, Tensor w_hh) -> (Tensor, Tensor)",
                       lambda c, lens, table, w_hh: ops.bilstm_table(c, list(lens), table, w_hh),
                       lambda c, lens, table, w_hh: (table.new_empty(c.shape[0], 2 * w_hh.shape[2], max(lens)),
                                                     table.new_empty(c.shape[0], 2 * w_hh.shape[2])))
# lengths read from a device int32 tensor: no argument of the launch depends on their values (hipGraph replay on new batches)
bilstm_table_static = _define("bilstm_table_static(Tensor captions, Tensor cap_lens, Tensor table, Tensor w_hh) -> (Tensor, Tensor)",
                              lambda c, lens, table, w_hh: ops.bilstm_table(c, lens, table, w_hh),
                              lambda c, lens, table, w_hh: (table.new_empty(c.shape[0], 2 * w_hh.shape[2], c.shape[1]),
                                                            table.new_empty(c.shape[0], 2 * w_hh.shape[2])))
# the GRU branch of RNN_ENCODER (util.py:207-211), eval mode
gru_gate_table = _define("gru_gate_table(Tensor emb, Tensor w_ih, Tensor b_ih, Tensor b_hh) -> (Tensor, Tensor)",
                         lambda e, w, bi, bh: ops.gru_gate_table(e, w, bi, bh),
                         lambda e, w, bi, bh: (e.new_empty(e.shape[0], 2, w.shape[1]), e.new_empty(2, w.shape[1] // 3)))
bigru_table = _define("bigru_table(Tensor captions, int[] cap_lens, Tensor table, Tensor w_hh, Tensor b_hn) -> (Tensor, Tensor)",
                      lambda c, lens, table, w_hh, b_hn: ops.bigru_table(c, list(lens), table, w_hh, b_hn),
                      lambda c, lens, table, w_hh, b_hn: (table.new_empty(c.shape[0], 2 * w_hh.shape[2], max(lens)),
                                                          table.new_empty(c.shape[0], 2 * w_hh.shape[2])))
bigru_table_static = _define("bigru_table_static(Tensor captions, Tensor cap_lens, Tensor table, Tensor w_hh, Tensor b_hn) -> "
                             "(Tensor, Tensor)",
                             lambda c, lens, table, w_hh, b_hn: ops.bigru_table(c, lens, table, w_hh, b_hn),
                             lambda c, lens, table, w_hh, b_hn: (table.new_empty(c.shape[0], 2 * w_hh.shape[2], c.shape[1]),
                                                                 table.new_empty(c.shape[0], 2 * w_hh.shape[2])))
lstm_gate_table = _define("lstm_gate_table(Tensor emb, Tensor w_ih, Tensor b_ih, Tensor b_hh) -> Tensor",
                          lambda e, w, bi, bh: ops.lstm_gate_table(e, w, bi, bh),
                          lambda e, w, bi, bh: e.new_empty(e.shape[0], 2, w.shape[1]))
bilstm_train = _define("bilstm_train(Tensor x, Tensor w_ih, Tensor w_hh, Tensor b_ih, Tensor b_hh, int[] cap_lens) -> "
                       "(Tensor, Tensor, Tensor)",
                       lambda x, wi, wh, bi, bh, lens: ops.bilstm_train_fwd(x, list(lens), wi, wh, bi, bh),
                       lambda x, wi, wh, bi, bh, lens: (x.new_empty(x.shape[0], 2 * wh.shape[2], x.shape[1]),
                                                        x.new_empty(x.shape[0], 2 * wh.shape[2]),
                                                        x.new_empty(x.shape[0], x.shape[1], 2, 5, wh.shape[2])))
bilstm_bwd = _define("bilstm_bwd(int[] cap_lens, Tensor w_hh, Tensor acts, Tensor words, Tensor d_words, Tensor? d_sent) -> "
                     "(Tensor, Tensor, Tensor)",
                     lambda lens, wh, acts, words, dw, ds: ops.bilstm_bwd(list(lens), wh, acts, words, dw, ds),
                     lambda lens, wh, acts, words, dw, ds: (acts.new_empty(acts.shape[0], acts.shape[1], 2, 4 * acts.shape[4]),
                                                            acts.new_empty(acts.shape[0], acts.shape[1], 2, acts.shape[4]),
                                                            acts.new_empty(2, 4 * acts.shape[4])))
bigru_train = _define("bigru_train(Tensor x, Tensor w_ih, Tensor w_hh, Tensor b_ih, Tensor b_hh, int[] cap_lens) -> "
                      "(Tensor, Tensor, Tensor)",
                      lambda x, wi, wh, bi, bh, lens: ops.bigru_train_fwd(x, list(lens), wi, wh, bi, bh),
                      lambda x, wi, wh, bi, bh, lens: (x.new_empty(x.shape[0], 2 * wh.shape[2], x.shape[1]),
                                                       x.new_empty(x.shape[0], 2 * wh.shape[2]),
                                                       x.new_empty(x.shape[0], x.shape[1], 2, 4, wh.shape[2])))
bigru_bwd = _define("bigru_bwd(int[] cap_lens, Tensor w_hh, Tensor acts, Tensor words, Tensor d_words, Tensor? d_sent) -> "
                    "(Tensor, Tensor, Tensor, Tensor)",
                    lambda lens, wh, acts, words, dw, ds: ops.bigru_bwd(list(lens), wh, acts, words, dw, ds),
                    lambda lens, wh, acts, words, dw, ds: (acts.new_empty(acts.shape[0], acts.shape[1], 2, 3 * acts.shape[4]),
                                                           acts.new_empty(acts.shape[0], acts.shape[1], 2, 3 * acts.shape[4]),
                                                           acts.new_empty(acts.shape[0], acts.shape[1], 2, acts.shape[4]),
                                                           acts.new_empty(2, 2, 3 * acts.shape[4])))


# ------------------------------------------------------------------------------------------------ DAMSM
damsm_words = _define("damsm_words(Tensor img_features, Tensor words_emb, int[] cap_lens, float gamma1, float gamma2) -> "
                      "(Tensor, Tensor)",
                      lambda f, w, lens, g1, g2: ops.damsm_words_similarity(f, w, list(lens), g1, g2, need_att=True),
                      lambda f, w, lens, g1, g2: (f.new_empty(f.shape[0], f.shape[0]),
                                                  f.new_empty(f.shape[0], w.shape[2], f.shape[2], f.shape[3])))
damsm_words_bwd = _define("damsm_words_bwd(Tensor img_features, Tensor words_emb, int[] cap_lens, float gamma1, float gamma2, "
                          "Tensor grad_sim) -> (Tensor, Tensor)",
                          lambda f, w, lens, g1, g2, gs: ops.damsm_words_bwd(f, w, list(lens), g1, g2, gs),
                          lambda f, w, lens, g1, g2, gs: (torch.empty_like(f), torch.empty_like(w)))
func_attention = _define("func_attention(Tensor query, Tensor context, float gamma1) -> (Tensor, Tensor)",
                         lambda q, c, g1: ops.func_attention(q, c, g1),
                         lambda q, c, g1: (torch.empty_like(q), q.new_empty(q.shape[0], q.shape[2], c.shape[2], c.shape[3])))
# text-image retrieval (tgsr_amd.retrieval reads them; evaluation only, no autograd formula): similarities of N images against candidate
# captions out of a pool of M (`cand` int [N, K], -1 = an empty slot; None = every caption), and the rank of a target column per row
damsm_gallery = _define("damsm_gallery(Tensor img_features, Tensor words_emb, int[] cap_lens, float gamma1, float gamma2, "
                        "Tensor? cand=None) -> Tensor",
                        lambda f, w, lens, g1, g2, cand=None: ops.damsm_gallery(f, w, list(lens), g1, g2, cand),
                        lambda f, w, lens, g1, g2, cand=None: f.new_empty(f.shape[0], w.shape[0] if cand is None else cand.shape[1]))
sent_gallery = _define("sent_gallery(Tensor cnn_code, Tensor rnn_code, float eps, float gamma3, Tensor? cand=None) -> Tensor",
                       lambda x, y, eps, g3, cand=None: ops.sent_gallery(x, y, eps, g3, cand),
                       lambda x, y, eps, g3, cand=None: x.new_empty(x.shape[0], y.shape[0] if cand is None else cand.shape[1]))
retrieval_ranks = _define("retrieval_ranks(Tensor sim, Tensor target) -> Tensor", lambda sim, t: ops.retrieval_ranks(sim, t),
                          lambda sim, t: sim.new_empty(sim.shape[0], dtype=torch.int32))
# distribution distances (tgsr_amd.featdist reads them; evaluation only, no autograd formula): the fp64 moments of a feature batch added
# into `sum` [D] / `outer` [D, D] (its block-upper part), and the three kernel sums of KID for S subsets (`ix`, `iy` int [S, m]) -> [S, 3]
feat_moments_add = _define("feat_moments_add(Tensor x, Tensor(a!) sum, Tensor(b!) outer) -> ()",
                           lambda x, s, o: ops.feat_moments_add(x, s, o), lambda x, s, o: None)
poly_mmd_sums = _define("poly_mmd_sums(Tensor x, Tensor y, Tensor ix, Tensor iy) -> Tensor",
                        lambda x, y, ix, iy: ops.poly_mmd_sums(x, y, ix, iy),
                        lambda x, y, ix, iy: x.new_empty((ix.shape[0], 3), dtype=torch.float64))


# attention panels (tgsr_amd.attnviz reads it): (panel, conf, order, maps) - one tile per caption word, the word's attention map
# expanded by the fp64 operators Mh / Mw and pasted over the image; `maps` is an empty tensor without with_maps
def _attn_panels_fake(images, att, cap_lens, Mh, Mw, u, alpha, K, by_conf, with_maps):
    B, T, h, w = att.shape
    u8 = dict(dtype=torch.uint8)
    return (att.new_empty((B, u * h, K * (u * w + 2), 3), **u8), att.new_empty((B, T), dtype=torch.float64),
            att.new_empty((B, T), dtype=torch.int32), att.new_empty((B, T, u * h, u * w) if with_maps else (0,), **u8))


attn_panels = _define("attn_panels(Tensor images, Tensor att, int[] cap_lens, Tensor Mh, Tensor Mw, int u, int alpha, int K, "
                      "bool by_conf, bool with_maps) -> (Tensor, Tensor, Tensor, Tensor)",
                      lambda im, att, lens, Mh, Mw, u, alpha, K, by_conf, with_maps:
                      ops.attn_panels(im, att, list(lens), Mh, Mw, u, alpha, K, by_conf, with_maps),
                      _attn_panels_fake)


# ------------------------------------------------------------------------------------------------ CA_NET (inference)
def _ca_net(sent_emb, w, b, ncf, eps):
    c, mu, logvar = ops.ca_net(sent_emb, w, b, ncf, eps)
    return (c if c is not None else mu.new_empty(0)), mu, logvar


ca_net = _define("ca_net(Tensor sent_emb, Tensor w, Tensor b, int ncf, Tensor? eps) -> (Tensor, Tensor, Tensor)", _ca_net,
                 lambda s_, w, b, ncf, eps: (s_.new_empty(s_.shape[0], ncf) if eps is not None else s_.new_empty(0),
                                             s_.new_empty(s_.shape[0], ncf), s_.new_empty(s_.shape[0], ncf)))
text_tail = _define("text_tail(Tensor words, Tensor[] w_ctxs, Tensor sent_emb, Tensor ca_w, Tensor ca_b, int ncf, Tensor captions) "
                    "-> (Tensor, Tensor, Tensor, Tensor)",
                    lambda words, ws, sent, cw, cb, ncf, cap: ops.text_tail(words, list(ws), sent, cw, cb, ncf, cap),
                    lambda words, ws, sent, cw, cb, ncf, cap:
                    (words.new_empty(len(ws), words.shape[0], ws[0].shape[0], 32), words.new_empty(words.shape[0], ncf),
                     words.new_empty(words.shape[0], ncf),
                     words.new_empty(words.shape[0], words.shape[2], dtype=torch.uint8)))
# ... and, for the reduced-precision generators, the `att_pack` their attention-fused kernels read (bool bf16: else f16)
text_tail_lp = _define("text_tail_lp(Tensor words, Tensor[] w_ctxs, Tensor sent_emb, Tensor ca_w, Tensor ca_b, int ncf, "
                       "Tensor captions, bool bf16) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
                       lambda words, ws, sent, cw, cb, ncf, cap, bf16:
                       ops.text_tail(words, list(ws), sent, cw, cb, ncf, cap,
                                     lp_dtype=torch.bfloat16 if bf16 else torch.float16),
                       lambda words, ws, sent, cw, cb, ncf, cap, bf16:
                       (words.new_empty(len(ws), words.shape[0], ws[0].shape[0], 32), words.new_empty(words.shape[0], ncf),
                        words.new_empty(words.shape[0], ncf),
                        words.new_empty(words.shape[0], words.shape[2], dtype=torch.uint8),
                        words.new_empty(len(ws) * words.shape[0] * 4096 + 4 * words.shape[0], dtype=torch.uint8)))
axpy_images = _define("axpy_images(Tensor[] ts, Tensor[] ss, float alpha) -> Tensor[]",
                      lambda ts, ss, alpha: ops.axpy_images(list(ts), list(ss), alpha), lambda ts, ss, alpha: [torch.empty_like(t) for t in ts])
# the last low-frequency head and every `+ a * SRb` in one launch (inference; ops.conv_to3_finish)
conv_to3_finish = _define("conv_to3_finish(Tensor x, Tensor w, Tensor[] ts, Tensor[] ss, float alpha) -> (Tensor, Tensor[])",
                          lambda x, w, ts, ss, alpha: ops.conv_to3_finish(x, w, list(ts), list(ss), alpha),
                          lambda x, w, ts, ss, alpha: (x.new_empty(x.shape[0], 3, x.shape[2], x.shape[3]),
                                                       [torch.empty_like(t) for t in ts]))
# ------------------------------------------------------------------------------------------------ CNN_ENCODER's frozen trunk
gconv_pack = _define("gconv_pack(Tensor w, Tensor? scale, bool dgrad) -> Tensor", lambda w, sc, dg: ops.gconv_pack(w, sc, dg),
                     lambda w, sc, dg: w.new_empty((w.shape[1], w.shape[0] * w.shape[2] * w.shape[3]) if dg else
                                                   (w.shape[0], w.shape[1] * w.shape[2] * w.shape[3])))
gconv = _define("gconv(bool dgrad, Tensor A, Tensor S, int s_coff, int s_ch, Tensor(a!) out, int o_coff, int kh, int kw, int stride, "
                "int padh, int padw, Tensor? bias, bool relu, bool accumulate, Tensor(b!)? ws, Tensor? mask) -> ()",
                lambda dg, A, S, sc, sch, out, oc, kh, kw, st, ph, pw, bias, relu, acc, ws, mask:
                ops.gconv(dg, A, S, sc, sch, out, oc, kh, kw, st, ph, pw, bias, relu, acc, ws, mask), lambda *a: None)
# training mode (batch-statistics BatchNorm): the raw convolution + its statistics partials, then BN + ReLU in place on the slice
gconv_stats = _define("gconv_stats(Tensor A, Tensor S, int s_coff, int s_ch, Tensor(a!) out, int o_coff, int kh, int kw, int stride, "
                      "int padh, int padw, Tensor(b!)? ws, Tensor(c!) stat_partial) -> ()",
                      lambda A, S, sc, sch, out, oc, kh, kw, st, ph, pw, ws, part:
                      (ops.gconv_stats(A, S, sc, sch, out, oc, kh, kw, st, ph, pw, ws, part), None)[1], lambda *a: None)
bn_train_relu_slice_from_stats = _define(
    "bn_train_relu_slice_from_stats(Tensor(a!) y, int coff, Tensor gamma, Tensor beta, float eps, float momentum, "
    "Tensor(b!)? running_mean, Tensor(c!)? running_var, Tensor(d!)? num_batches_tracked, Tensor stat_partial, int slot_px, "
    "Tensor(e!) stats) -> ()",
    lambda y, coff, g, b, eps, mom, rm, rv, nbt, part, spx, stats:
    (ops.bn_train_relu_slice_from_stats(y, coff, g, b, eps, mom, rm, rv, nbt, part, spx, stats), None)[1], lambda *a: None)
maxpool3s2 = _define("maxpool3s2(Tensor x, Tensor(a!) out, int o_coff) -> ()", lambda x, out, oc: ops.maxpool3s2(x, out, oc),
                     lambda *a: None)
maxpool3s2_bwd = _define("maxpool3s2_bwd(Tensor x, Tensor dy, int dy_coff, Tensor(a!) dx, bool accumulate, Tensor? mask) -> ()",
                         lambda x, dy, dc, dx, acc, mask: ops.maxpool3s2_bwd(x, dy, dc, dx, acc, mask), lambda *a: None)
# the VGG16 trunk's pool and the LPIPS tail (tgsr_lpips.hip; tgsr_amd/lpips.py walks them)
maxpool2s2 = _define("maxpool2s2(Tensor x, Tensor(a!) out, int o_coff) -> ()", lambda x, out, oc: ops.maxpool2s2(x, out, oc),
                     lambda *a: None)
maxpool2s2_bwd = _define("maxpool2s2_bwd(Tensor x, Tensor dy, int dy_coff, Tensor(a!) dx, bool accumulate, Tensor? mask) -> ()",
                         lambda x, dy, dc, dx, acc, mask: ops.maxpool2s2_bwd(x, dy, dc, dx, acc, mask), lambda *a: None)
lpips_layer = _define("lpips_layer(Tensor f0, Tensor f1, Tensor w) -> Tensor", lambda f0, f1, w: ops.lpips_layer(f0, f1, w),
                      lambda f0, f1, w: f0.new_empty(f0.shape[0], ops.lpips_nslots(f0.shape[1], f0.shape[2] * f0.shape[3]),
                                                     dtype=torch.float64))
lpips_finish = _define("lpips_finish(Tensor[] partials, int[] hws) -> (Tensor, Tensor)",
                       lambda ps, hws: ops.lpips_finish(list(ps), list(hws)),
                       lambda ps, hws: (ps[0].new_empty(len(ps), ps[0].shape[0], dtype=torch.float32),
                                        ps[0].new_empty(ps[0].shape[0], dtype=torch.float32)))
lpips_layer_bwd = _define("lpips_layer_bwd(Tensor g, Tensor f0, Tensor f1, Tensor w, Tensor(a!) df0, bool accumulate, Tensor? mask) -> ()",
                          lambda g, f0, f1, w, df0, acc, mask: ops.lpips_layer_bwd(g, f0, f1, w, df0, acc, mask), lambda *a: None)
avgpool3 = _define("avgpool3(Tensor x, Tensor(a!) out, bool accumulate, Tensor? mask) -> ()",
                   lambda x, out, acc, mask: ops.avgpool3(x, out, acc, mask), lambda *a: None)
plane_mean = _define("plane_mean(Tensor x) -> Tensor", lambda x: ops.plane_mean(x), lambda x: x.new_empty(x.shape[0], x.shape[1]))
plane_mean_bwd = _define("plane_mean_bwd(Tensor dy, int H, int W) -> Tensor", lambda dy, H, W: ops.plane_mean_bwd(dy, H, W),
                         lambda dy, H, W: dy.new_empty(dy.shape[0], dy.shape[1], H, W))
relu_mask_ = _define("relu_mask_(Tensor(a!) dy, Tensor y, int coff, int ch) -> ()", lambda dy, y, c, ch: ops.relu_mask_(dy, y, c, ch),
                     lambda *a: None)
bilinear = _define("bilinear(Tensor x, int OH, int OW) -> Tensor", lambda x, OH, OW: ops.bilinear(x, OH, OW),
                   lambda x, OH, OW: x.new_empty(x.shape[0], x.shape[1], OH, OW))
sum_stack = _define("sum_stack(Tensor stack, int n, Tensor(a!) out) -> ()", lambda st, n, out: ops.sum_stack(st, n, out), lambda *a: None)
interleave2x2_ = _define("interleave2x2_(Tensor t00, Tensor t01, Tensor t10, Tensor t11, Tensor(a!) dx, bool accumulate, Tensor? mask) -> ()",
                         lambda a, b, c, d, dx, acc, m: ops.interleave2x2((a, b, c, d), dx, acc, m), lambda *a: None)
bilinear_bwd = _define("bilinear_bwd(Tensor dy, int H, int W) -> Tensor", lambda dy, H, W: ops.bilinear_bwd(dy, H, W),
                       lambda dy, H, W: dy.new_empty(dy.shape[0], dy.shape[1], H, W))
adam_flat_ = _define("adam_flat_(Tensor(a!) param, Tensor grad, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor(d!) state, float lr, "
                     "float beta1, float beta2, float eps, float weight_decay, bool advance) -> ()",
                     lambda p, g, m, v, st, lr, b1, b2, eps, wd, adv: ops.adam_flat(p, g, m, v, st, lr, b1, b2, eps, wd, adv),
                     lambda *a: None)
weighted_bce = _define("weighted_bce(Tensor a, Tensor? b, Tensor target, Tensor weight) -> Tensor",
                       lambda a, b, t, w: ops.weighted_bce(a, b, t, w), lambda a, b, t, w: a.new_empty(()))


def _weighted_bce_bwd(dy, a, b, t, w):
    da, db = ops.weighted_bce_bwd(dy, a, b, t, w)
    return da, (db if db is not None else a.new_empty(0))


weighted_bce_bwd = _define("weighted_bce_bwd(Tensor dy, Tensor a, Tensor? b, Tensor target, Tensor weight) -> (Tensor, Tensor)",
                           _weighted_bce_bwd, lambda dy, a, b, t, w: (torch.empty_like(a), torch.empty_like(b) if b is not None else a.new_empty(0)))


def _weighted_bce_backward(ctx, dy):
    a, b, t, w = ctx.saved_tensors if ctx.has_b else (ctx.saved_tensors[0], None, ctx.saved_tensors[1], ctx.saved_tensors[2])
    da, db = weighted_bce_bwd(dy.contiguous(), a, b, t, w)
    return (da if ctx.needs_input_grad[0] else None), (db if ctx.has_b and ctx.needs_input_grad[1] else None), None, None


def _weighted_bce_setup(ctx, inputs, output):
    a, b, t, w = inputs
    ctx.has_b = b is not None
    if b is not None:
        ctx.save_for_backward(a, b, t, w)
    else:
        ctx.save_for_backward(a, t, w)


torch.library.register_autograd("tgsr::weighted_bce", _weighted_bce_backward, setup_context=_weighted_bce_setup, lib=_lib)
axpy_map = _define("axpy_map(Tensor t, Tensor s, Tensor amap) -> Tensor", lambda t, s, a: ops.axpy_map(t, s, a),
                   lambda t, s, a: torch.empty_like(t))


def _axpy_map_bwd(dy, s, amap, need_ds, need_da):
    ds, da = ops.axpy_map_bwd(dy, s, amap, need_ds, need_da)
    return (ds if ds is not None else dy.new_empty(0)), (da if da is not None else dy.new_empty(0))


axpy_map_bwd = _define("axpy_map_bwd(Tensor dy, Tensor s, Tensor amap, bool need_ds, bool need_da) -> (Tensor, Tensor)", _axpy_map_bwd,
                       lambda dy, s, a, nds, nda: (torch.empty_like(dy) if nds else dy.new_empty(0),
                                                   torch.empty_like(a) if nda else dy.new_empty(0)))


def _axpy_map_backward(ctx, dy):
    s, amap = ctx.saved_tensors
    nds, nda = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
    ds = da = None
    if nds or nda:
        ds, da = axpy_map_bwd(dy.contiguous(), s, amap, nds, nda)
    return (dy if ctx.needs_input_grad[0] else None), (ds if nds else None), (da if nda else None)


torch.library.register_autograd("tgsr::axpy_map", _axpy_map_backward,
                                setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[1], inputs[2]), lib=_lib)
affine_act = _define("affine_act(Tensor raw, Tensor scale, Tensor shift, int act) -> Tensor",
                     lambda raw, sc, sh, act: ops.affine_act(raw, sc, sh, act), lambda raw, sc, sh, act: torch.empty_like(raw))
affine_act_bwd = _define("affine_act_bwd(Tensor dy, Tensor? out, Tensor scale, int act) -> Tensor",
                         lambda dy, out, sc, act: ops.affine_act_bwd(dy, out, sc, act), lambda dy, out, sc, act: torch.empty_like(dy))
multi_copy = _define("multi_copy(Tensor(a!)[] dsts, Tensor[] srcs) -> ()",
                     lambda dsts, srcs: ops.multi_copy(list(dsts), list(srcs)), lambda dsts, srcs: None)
to_uint8 = _define("to_uint8(Tensor img) -> Tensor", lambda x: ops.to_uint8(x), lambda x: torch.empty_like(x, dtype=torch.uint8))
# image quality against ground truth (tgsr_amd.metrics reads them): float64 [B, 3] = (SSE RGB, SSE Y, sum of SSIM-on-Y windows)
sr_metrics = _define("sr_metrics(Tensor sr, Tensor hr, int shave=0) -> Tensor", lambda sr, hr, shave=0: ops.sr_metrics(sr, hr, shave),
                     lambda sr, hr, shave=0: sr.new_empty(sr.shape[0], 3, dtype=torch.float64))
rgb_to_y = _define("rgb_to_y(Tensor rgb) -> Tensor", lambda rgb: ops.rgb_to_y(rgb),
                   lambda rgb: rgb.new_empty(rgb.shape[0], rgb.shape[2], rgb.shape[3], dtype=torch.uint8))


# no-reference image quality (tgsr_amd.niqe reads it): (feats float64 [B, nblk, 36], sharp float64 [B, nblk]) over the 96 x 96 blocks
def _niqe_features_fake(img, shave=0):
    nblk = ((img.shape[2] - 2 * shave) // ops.NIQE_BLOCK) * ((img.shape[3] - 2 * shave) // ops.NIQE_BLOCK)
    return (img.new_empty((img.shape[0], nblk, 36), dtype=torch.float64), img.new_empty((img.shape[0], nblk), dtype=torch.float64))


niqe_features = _define("niqe_features(Tensor img, int shave=0) -> (Tensor, Tensor)", lambda img, shave=0: ops.niqe_features(img, shave),
                        _niqe_features_fake)

# the objectives that read the generator's word-attention maps (miscc.losses.weight_MSE / words_reweight_loss): cap_lens is an int32
# DEVICE tensor; weight_mse returns (term [], wmax [B, h, w], widx uint8 [B, h, w], wlast [B, 1, H, W] or [0]); autograd.WeightMSE
# is the differentiable form over weight_mse / weight_mse_bwd (absent gradients come back as [0])
attn_confidence = _define("attn_confidence(Tensor att, Tensor cap_lens) -> Tensor", lambda att, lens: ops.attn_confidence(att, lens),
                          lambda att, lens: att.new_empty(att.shape[0], att.shape[1]))
weight_mse = _define("weight_mse(Tensor fake, Tensor label, Tensor att, bool want_wlast) -> (Tensor, Tensor, Tensor, Tensor)",
                     lambda fake, label, att, wl: ops.weight_mse(fake, label, att, wl),
                     lambda fake, label, att, wl: (
                         fake.new_empty(()), att.new_empty(att.shape[0], att.shape[2], att.shape[3]),
                         att.new_empty(att.shape[0], att.shape[2], att.shape[3], dtype=torch.uint8),
                         fake.new_empty((fake.shape[0], 1, fake.shape[2], fake.shape[3]) if wl else (0,))))


def _weight_mse_bwd(grad, fake, label, wmax, widx, T, need_fake, need_label, need_att):
    return tuple(t if t is not None else fake.new_empty(0)
                 for t in ops.weight_mse_bwd(grad, fake, label, wmax, widx, T, need_fake, need_label, need_att))


weight_mse_bwd = _define("weight_mse_bwd(Tensor grad, Tensor fake, Tensor label, Tensor wmax, Tensor widx, int T, bool need_fake, "
                         "bool need_label, bool need_att) -> (Tensor, Tensor, Tensor)", _weight_mse_bwd,
                         lambda grad, fake, label, wmax, widx, T, nf, nl, na: (
                             torch.empty_like(fake, memory_format=torch.contiguous_format) if nf else fake.new_empty(0),
                             torch.empty_like(fake, memory_format=torch.contiguous_format) if nl else fake.new_empty(0),
                             fake.new_empty((wmax.shape[0], T, wmax.shape[1], wmax.shape[2]) if na else (0,))))

# the cycle-consistency objective (miscc.losses.CycleMSE): all scales of a pyramid in one forward and one backward launch.  cycle_mse
# returns (loss [], terms [n], diff [n, B, C, h, w]); cycle_mse_bwd takes the sizes (H_0, W_0, H_1, W_1, ...) and one flag per scale and
# returns n + 1 tensors - d_sr[0..n-1], d_lr - absent gradients as [0]; autograd.CycleMSE is the differentiable form
cycle_mse = _define("cycle_mse(Tensor[] sr, Tensor lr) -> (Tensor, Tensor, Tensor)", lambda sr, lr: ops.cycle_mse(sr, lr),
                    lambda sr, lr: (lr.new_empty(()), lr.new_empty(len(sr)), lr.new_empty((len(sr),) + tuple(lr.shape))))


def _cycle_mse_bwd(grad, diff, sizes, need_sr, need_lr):
    d_sr, d_lr = ops.cycle_mse_bwd(grad, diff, sizes, need_sr, need_lr)
    return [t if t is not None else diff.new_empty(0) for t in d_sr + [d_lr]]


def _cycle_mse_bwd_fake(grad, diff, sizes, need_sr, need_lr):
    _n, B, C, h, w = diff.shape
    out = [diff.new_empty((B, C, sizes[2 * i], sizes[2 * i + 1]) if need else (0,)) for i, need in enumerate(need_sr)]
    return out + [diff.new_empty((B, C, h, w) if need_lr else (0,))]


cycle_mse_bwd = _define("cycle_mse_bwd(Tensor grad, Tensor diff, int[] sizes, bool[] need_sr, bool need_lr) -> Tensor[]",
                        _cycle_mse_bwd, _cycle_mse_bwd_fake)


# whole images by overlapping tiles (SRPipeline.upscale): `table` is the host int32 [Tb, 6] window table, `table_dev` its device copy
def _tile_gather(img, img2, table, table_dev, th, tw):
    lr, lrb = ops.tile_gather(img, table, th, tw, img2=img2, table_dev=table_dev)
    return lr, (lrb if lrb is not None else lr.new_empty(0))


tile_gather = _define("tile_gather(Tensor img, Tensor? img2, Tensor table, Tensor table_dev, int th, int tw) -> (Tensor, Tensor)",
                      _tile_gather,
                      lambda img, img2, table, table_dev, th, tw: (
                          img.new_empty(table.shape[0], 3, th, tw, dtype=torch.float32),
                          img.new_empty((table.shape[0], 3, th, tw) if img2 is not None else (0,), dtype=torch.float32)))
tile_stitch = _define("tile_stitch(Tensor[] tiles, Tensor(a!)[] outs, Tensor table, Tensor table_dev, int H, int W, int th, int tw) -> ()",
                      lambda tiles, outs, table, table_dev, H, W, th, tw:
                      ops.tile_stitch(list(tiles), list(outs), table, H, W, th, tw, table_dev=table_dev),
                      lambda *a: None)


# geometric self-ensemble (x8; SRPipeline.upscale(ensemble=8), self_ensemble): the variant batch of every window of N images, and
# the mean of its outputs mapped back.  srcs_t: empty when srcs hold all eight variants, else the transposed group of every output
def _d8_shape(img, table, th, tw, k0, nk):
    hh, ww = (tw, th) if k0 == 4 else (th, tw)
    return (img.shape[0], table.shape[0], nk, 3, hh, ww)


def _d8_gather(img, img2, table, table_dev, th, tw, k0, nk):
    lr, lrb = ops.d8_gather(img, table, th, tw, k0, nk, img2=img2, table_dev=table_dev)
    return lr, (lrb if lrb is not None else lr.new_empty(0))


d8_gather = _define("d8_gather(Tensor img, Tensor? img2, Tensor table, Tensor table_dev, int th, int tw, int k0, int nk) "
                    "-> (Tensor, Tensor)", _d8_gather,
                    lambda img, img2, table, table_dev, th, tw, k0, nk: (
                        img.new_empty(_d8_shape(img, table, th, tw, k0, nk), dtype=torch.float32),
                        img.new_empty(_d8_shape(img, table, th, tw, k0, nk) if img2 is not None else (0,), dtype=torch.float32)))
d8_merge = _define("d8_merge(Tensor[] srcs, Tensor[] srcs_t, Tensor(a!)[] outs, Tensor table, Tensor table_dev, int H, int W, int th, "
                   "int tw) -> ()",
                   lambda srcs, srcs_t, outs, table, table_dev, H, W, th, tw:
                   ops.d8_merge(list(srcs), list(outs), table, H, W, th, tw, srcs_t=list(srcs_t) if len(srcs_t) else None,
                                table_dev=table_dev),
                   lambda *a: None)


# ================================================================================================ reduced-precision path
# (lp images are mutable arguments: every kernel writes a channel slice of a caller-owned zero-bordered image)
lp_conv3x3 = _define("lp_conv3x3(Tensor x, Tensor wpack, int cin, int cout, Tensor? scale, Tensor? shift, bool glu, bool upsample, "
                     "Tensor? residual, int res_coff, Tensor(a!) out, int out_coff) -> ()",
                     lambda x, wp, cin, cout, s, t, glu, up, res, rco, out, oco:
                     (lp.conv3x3(x, wp, cin, cout, s, t, glu=glu, upsample=up, residual=res, res_coff=rco, out=out, out_coff=oco),
                      None)[1], lambda *a: None)
lp_resblocks = _define("lp_resblocks(Tensor x, Tensor[] wpacks, Tensor[] scales, Tensor[] shifts, Tensor(a!) tmp, Tensor(b!) a, "
                       "Tensor(c!) b, Tensor(d!) flags) -> ()",
                       lambda x, wp, sc, sh, tmp, a, b, flags: (lp.resblocks(x, list(wp), list(sc), list(sh), tmp, a, b, flags), None)[1],
                       lambda *a: None)
# the producers of h may also attend to the words for the pixels they have just computed (GlobalAttention.py:87-130 at
# util.py:768-771 / 814-817): att_pack = text_tail_lp's fifth output, index = which projection the stage attends through
_ATT_SCHEMA = ", Tensor att_pack, int nsets, int index, int T, bool use_mask, bool correct_mask, int c_coff, Tensor(%s!)? attn"


def _define_lp_upconv(name, head, att):
    """The upBlock by sub-pixel decomposition [+ the partial sums of its image head] [+ the next stage's word attention] (the
    last eight arguments: lp.AttFuse's)."""
    schema = name + "(Tensor x, Tensor wpack, int cin, int cout, Tensor? scale, Tensor? shift, "
    if head:      # without the attention `out` may be absent: the feature image is then not written
        schema += "Tensor head_wpack, int K, Tensor(a!) partial, Tensor(b!)%s out, int out_coff" % ("" if att else "?")
    else:
        schema += "Tensor(a!) out, int out_coff"

    def fn(x, wp, cin, cout, s, t, *rest):
        a = lp.AttFuse(*rest[-8:]) if att else None
        if head:
            hw, K, part, out, oco = rest[:5]
            lp.upconv_glu_head(x, wp, cin, cout, s, t, hw, K, partial=part, out=out, out_coff=oco, write_out=out is not None, att=a)
        else:
            lp.upconv_glu(x, wp, cin, cout, s, t, out=rest[0], out_coff=rest[1], att=a)
    return _define(schema + (_ATT_SCHEMA % ("c" if head else "b") if att else "") + ") -> ()", fn, lambda *a: None)


def _define_lp_stem(name, att):
    def fn(x, w, s, t, out, oco, *a):
        lp.stem(x, w, s, t, out=out, out_coff=oco, att=lp.AttFuse(*a) if att else None)
    return _define(name + "(Tensor x, Tensor w, Tensor scale, Tensor shift, Tensor(a!) out, int out_coff" +
                   (_ATT_SCHEMA % "b" if att else "") + ") -> ()", fn, lambda *a: None)


lp_upconv_glu = _define_lp_upconv("lp_upconv_glu", False, False)
lp_upconv_glu_head = _define_lp_upconv("lp_upconv_glu_head", True, False)
lp_upconv_glu_att = _define_lp_upconv("lp_upconv_glu_att", False, True)
lp_upconv_glu_head_att = _define_lp_upconv("lp_upconv_glu_head_att", True, True)
lp_stem = _define_lp_stem("lp_stem", False)
lp_stem_att = _define_lp_stem("lp_stem_att", True)
lp_convert = _define("lp_convert(Tensor src, Tensor(a!) out) -> ()", lambda src, out: (lp.convert(src, out), None)[1],
                     lambda *a: None)
_to3_fake = lambda x, *a: x.new_empty(x.shape[0], 3, x.shape[1] - 2, x.shape[2] - 2, dtype=torch.float32)      # noqa: E731
lp_conv_to3 = _define("lp_conv_to3(Tensor x, Tensor wpack, int K, bool tanh_axpy, Tensor? addend, float alpha) -> Tensor",
                      lambda x, wp, K, act, add, alpha: lp.conv_to3(x, wp, K, tanh_axpy=act, addend=add, alpha=alpha), _to3_fake)
# NetG_highweight's other forms (weightmap x useAct, model.py:212-298): the weight map a_k in place of alpha, tanh or the identity
lp_conv_to3_map = _define("lp_conv_to3_map(Tensor x, Tensor wpack, int K, bool tanh, Tensor? addend, float alpha, Tensor? amap) "
                          "-> Tensor",
                          lambda x, wp, K, th, add, alpha, amap: lp.conv_to3_map(x, wp, K, tanh=th, addend=add, alpha=alpha, amap=amap),
                          _to3_fake)
lp_word_attention = _define("lp_word_attention(Tensor(a!) h_img, Tensor src, Tensor? mask, int T, bool correct_mask, int c_coff) -> Tensor",
                            lambda h, src, mask, T, cm, cco: lp.word_attention(h, src, mask, T, correct_mask=cm, c_coff=cco),
                            lambda h, src, mask, T, cm, cco: h.new_empty(h.shape[0], T, h.shape[1] - 2, h.shape[2] - 2, dtype=torch.float32))


def _lp_head_combine(sizes_h, sizes_w, partial_low, partial_high, low, high, low_tanh, alpha, amap=(), high_tanh=True):
    n = len(sizes_h)
    none = lambda t: None if (t is None or t.numel() == 0) else t          # noqa: E731  (an empty tensor stands for "absent")
    lp.head_combine(low[0].shape[0], list(zip(sizes_h, sizes_w)), [none(t) for t in partial_low[:n]],
                    [none(t) for t in partial_high[:n]], list(low[:n]), [none(t) for t in high[:n]], low_tanh, alpha,
                    amap=[none(t) for t in amap[:n]] if len(amap) else None, high_tanh=high_tanh)


lp_head_combine = _define("lp_head_combine(int[] H, int[] W, Tensor[] partial_low, Tensor[] partial_high, Tensor(a!)[] low, "
                          "Tensor(b!)[] high, bool low_tanh, float alpha) -> ()", _lp_head_combine, lambda *a: None)
# + the per-scale weight maps and / or tanh-free high heads of NetG_highweight's other forms
lp_head_combine_map = _define("lp_head_combine_map(int[] H, int[] W, Tensor[] partial_low, Tensor[] partial_high, "
                              "Tensor(a!)[] low, Tensor(b!)[] high, Tensor[] amap, bool low_tanh, bool high_tanh, float alpha) -> ()",
                              lambda H, W, pl, ph, lo, hi, amap, low_tanh, high_tanh, alpha:
                              _lp_head_combine(H, W, pl, ph, lo, hi, low_tanh, alpha, amap, high_tanh), lambda *a: None)
