"""Tensor-level wrappers over the C ABI (include/tgsr_hip.h): validate, allocate outputs with torch, launch on
torch's current HIP stream.  PyTorch is plumbing here (device memory + streams); the arithmetic is in
libtgsr_hip.so.  No function in this file computes on the CPU or through eager torch ops.
"""
import collections
import ctypes
import functools
import os
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import TgsrError, check

BN_EPS = 1e-5

# Per-launch measurement hook (bench.py): when `profile` is a list, every conv / attention launch is bracketed
# with HIP events on the launch stream and appended as (kernel, algorithmic flops, algorithmic bytes, e0, e1).
profile = None


def _ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current HIP stream of the current device as a void*.  The raw-handle query costs < 1 us; going through
    torch.cuda.current_stream() costs ~5 us, i.e. 0.25 ms of host time per forward at ~50 launches."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _rows4(stats: torch.Tensor):
    """Pointers of the four rows of a [4, C] fp32 tensor (mean, invstd, scale, shift).  Address arithmetic where the tensor is
    dense - four `stats[i]` views cost ~3 us of host time per call, on ~150 BatchNorm calls of a host-bound train step."""
    if stats.dim() == 2 and stats.shape[0] == 4 and stats.is_contiguous() and stats.dtype == torch.float32:
        base, step = stats.data_ptr(), stats.shape[1] * 4
        return (ctypes.c_void_p(base), ctypes.c_void_p(base + step), ctypes.c_void_p(base + 2 * step), ctypes.c_void_p(base + 3 * step))
    return _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3])


def _need_hip(*ts):
    """Every tensor on ONE HIP device, and that device the current one: the kernels launch on the current device's
    stream (`_stream()`), so a tensor living elsewhere would be read through a foreign pointer on the wrong queue."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise TgsrError("tgsr_amd ops run only on HIP tensors (got a %s tensor); there is no CPU fallback"
                            % t.device.type)
        if dev is None:
            dev = t.device.index
        elif t.device.index != dev:
            raise TgsrError("tgsr_amd op got tensors on different devices (cuda:%d and cuda:%d)" % (dev, t.device.index))
    if dev is not None and dev != torch.cuda.current_device():
        raise TgsrError("tensors live on cuda:%d but the current device is cuda:%d: run the call under "
                        "`with torch.cuda.device(%d):` (SRPipeline / the trainers do)" % (dev, torch.cuda.current_device(), dev))


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TgsrError("%s must be float32, got %s" % (name, t.dtype))
    return t


def _nchw_bstride(t: torch.Tensor, name: str) -> Tuple[torch.Tensor, int]:
    """Accept [B,C,H,W] with a dense (C,H,W) block and ANY batch stride (channel-slice views); else copy."""
    B, C, H, W = t.shape
    if t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W:
        return t, t.stride(0) if B > 1 else C * H * W
    t = t.contiguous()
    return t, C * H * W


# ----------------------------------------------------------------------------------------- the conv3x3 kernel forms
# Everything the host side knows about a kernel form the fp32 generator's 3x3 convolutions run on is one row here; the
# launcher (_conv3x3), the packer (pack_weight), the router (conv3x3_form) and the operator definitions of custom_ops.py read it.
#   what        the public wrapper below that launches it (named in error messages);  op: its torch.ops.tgsr operator (`op`_out
#               writes into a view;  op_plain: the un-gated operator of training;  pack_op: the pack operator)
#   fwd         C entry point;  fwd_plain: the entry without the gate where that is another function;  tail: what the entry takes
#               after (out, batch stride): "epi,up" / "epi" (those two also take a residual in front of out), "glu" or ""
#   stats, nslots   the raw convolution whose epilogue leaves BatchNorm's partial sums, and its slot count (training)
#   pack, pack_dgrad, elems   the pack of a [Cout,Cin,3,3] weight, of its data-gradient conv, and the packed size;  pack_arg: what
#               they take after (Cout, Cin): "k" the kernel size (all three), "glu" the gate flag (pack only), "" nothing
#   up          the nearest x2 up-sampling is part of the kernel;  gate_only: it has the GLU epilogue only
#   kernel      the name it reports to `profile`
#   shape(cin, cout, H, W)   the shapes the kernel takes (H x W of the input)
#   align       out / residual must start on this many bytes with batch strides that keep every image there; 0: the kernel takes
#               any address.  (x: 16 bytes for the Winograd forms, any address for direct and upconv.  csrc/tgsr_conv_plan.h holds the
#               library's table of the same requirements; tests/test_infer_abi_host.py ties the two.)
Form = collections.namedtuple("Form", "name what op op_plain pack_op fwd fwd_plain tail stats nslots pack pack_dgrad elems pack_arg "
                                      "up gate_only kernel shape align")


def _wino4_shape(cin, cout, H, W):
    return cout % 64 == 0 and cin % 4 == 0 and W % 64 == 0 and H % 8 == 0            # whole workgroup tiles


def _wino4_form(cin: int) -> str:
    """Which of the two F(4x4) forms a layer that goes there takes: the register-fed one where the layer has an even number of
    4-channel stages, else the LDS-fed one."""
    return "wino4w" if cin % 8 == 0 else "wino4"


FORMS = {f.name: f for f in (
    Form("direct", "conv3x3_fused", "conv3x3_fused", None, "pack_conv3x3_weight", "tgsr_conv3x3_fwd", None, "epi,up", None, None,
         "tgsr_pack_conv_weight", "tgsr_pack_conv_weight_dgrad", "tgsr_packed_weight_elems", "k",
         False, False, "conv3x3_mfma_kernel", lambda cin, cout, H, W: True, 0),
    Form("wino", "conv3x3_wino", "conv3x3_wino", None, "pack_wino_weight", "tgsr_wino_conv3x3_fwd", None, "epi",
         "tgsr_wino_conv3x3_stats_fwd", "tgsr_wino_stats_nslots",
         "tgsr_pack_wino_weight", "tgsr_pack_wino_weight_dgrad", "tgsr_packed_wino_weight_elems", "glu",
         False, False, "wino_conv3x3_kernel", lambda cin, cout, H, W: cout % 32 == 0 and cin % 4 == 0 and W % 4 == 0, 8),
    # F(4x4, 3x3), LDS-fed
    Form("wino4", "conv3x3_wino4", "conv3x3_wino4", None, "pack_wino4_weight", "tgsr_wino4_conv3x3_fwd", None, "epi",
         "tgsr_wino4_conv3x3_stats_fwd", "tgsr_wino4_stats_nslots",
         "tgsr_pack_wino4_weight", "tgsr_pack_wino4_weight_dgrad", "tgsr_packed_wino4_weight_elems", "glu",
         False, False, "wino4_conv3x3_kernel", _wino4_shape, 16),
    # F(4x4, 3x3), register-fed: 128-row groups where Cout % 128 == 0, else 64-row groups in 4-wave workgroups; its pack has the size
    # of wino4's in another order
    Form("wino4w", "conv3x3_wino4", "conv3x3_wino4w", None, "pack_wino4w_weight", "tgsr_wino4_wide_conv3x3_fwd", None, "epi",
         "tgsr_wino4_wide_conv3x3_stats_fwd", "tgsr_wino4_wide_stats_nslots",
         "tgsr_pack_wino4_wide_weight", "tgsr_pack_wino4_wide_weight_dgrad", "tgsr_packed_wino4_weight_elems", "glu",
         False, False, "wino4w_conv3x3_kernel", lambda cin, cout, H, W: _wino4_shape(cin, cout, H, W) and _wino4_form(cin) == "wino4w", 16),
    # the upBlock forms: sub-pixel (four 2x2 convs on the pre-upsample tensor), Winograd F(2x2) and F(4x4) on the up-sampled grid
    # (upconv's 8 bytes are the library's requirement, stated for whoever places `out`; conv3x3_form does not route on it: an `out` off
    # 8 bytes there is the wrapper's error, as it always was)
    Form("upconv", "upconv3x3_glu", "upconv3x3_glu", None, None, "tgsr_upconv3x3_glu_fwd", None, "", None, None,
         "tgsr_pack_upconv_weight", None, "tgsr_packed_upconv_weight_elems", "",
         True, True, "upconv_glu_mfma_kernel", lambda cin, cout, H, W: cout % 64 == 0, 8),
    Form("upwino", "upwino_glu", "upwino_glu", "upwino", "pack_upwino_weight", "tgsr_upwino_glu_fwd", "tgsr_upwino_fwd", "", None, None,
         "tgsr_pack_upwino_weight", None, "tgsr_packed_upwino_weight_elems", "glu",
         True, False, "upwino_glu_kernel", lambda cin, cout, H, W: cout % 64 == 0 and cin % 4 == 0 and W % 4 == 0, 8),
    Form("upwino4", "upwino4_glu", "upwino4_glu", None, "pack_upwino4_weight", "tgsr_upwino4_fwd", None, "glu", None, None,
         "tgsr_pack_upwino4_weight", None, "tgsr_packed_upwino4_weight_elems", "glu",
         True, False, "upwino4_kernel",                        # an even number of 4-channel stages, whole 4 x 64 OUTPUT tiles
         lambda cin, cout, H, W: cout % 64 == 0 and cin % 8 == 0 and (2 * W) % 64 == 0 and (2 * H) % 4 == 0, 16),
)}


# ----------------------------------------------------------------------------------------- weight prep
@functools.lru_cache(maxsize=None)
def packed_elems(form: str, cout: int, cin: int) -> int:
    """Floats in form `form`'s pack of a [cout, cin, 3, 3] weight (the library's own count)."""
    f = FORMS[form]
    fn = getattr(_lib.lib(), f.elems)
    return int(fn(cout, cin, 3) if f.pack_arg == "k" else fn(cout, cin))


def _bad_pack(what: str, form: str, pack: torch.Tensor, cout: int, cin: int):
    """The kernels walk the packed filter by (Cout, Cin of the INPUT): a pack made for another channel count (its size is not
    packed_elems) would be read past its end.  torch raises a shape error for the same mistake (weight [Cout, Cin', 3, 3] on a
    Cin-channel input); so does this."""
    raise TgsrError("%s: the packed weight holds %d values, not the %d of a [%d, %d, 3, 3] filter - the input has %d "
                    "channels, the weight was packed for another count" % (what, pack.numel(), packed_elems(form, cout, cin),
                                                                          cout, cin, cin))


def _pack_out(out, n, dev):
    """A pack's destination: fresh, or the caller's persistent buffer (autograd.PackCache re-packs in place)."""
    if out is None:
        return torch.empty(n, dtype=torch.float32, device=dev)
    if out.numel() != n or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise TgsrError("pack: out %s %s does not hold %d floats" % (tuple(out.shape), out.dtype, n))
    return out


def pack_weight(form: str, w: torch.Tensor, glu: bool = False, dgrad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pack of `w` [Cout,Cin,3,3] for kernel form `form` (a key of FORMS).  `glu` must match the epilogue the pack is used
    with (the Winograd packs group value channels with their gate channels).  `dgrad`: w is the forward conv's weight and the
    pack is of its data-gradient conv (in/out swapped, taps flipped: the pack kernels read it so - no flip/transpose copies)."""
    f = FORMS[form]
    _need_hip(w)
    w = _f32(w.detach(), "weight").contiguous()
    Cout, Cin, K, K2 = w.shape
    assert K == 3 and K2 == 3
    name = f.pack
    if dgrad:
        assert not glu
        if f.pack_dgrad is None:
            raise TgsrError("pack_weight: the %s form has no data-gradient pack" % form)
        Cout, Cin, name = Cin, Cout, f.pack_dgrad
    fn = getattr(_lib.lib(), name)
    out = _pack_out(out, packed_elems(form, Cout, Cin), w.device)
    if f.pack_arg == "k":
        rc = fn(_p(w), _p(out), Cout, Cin, 3, _stream())
    elif f.pack_arg == "glu" and not dgrad:
        rc = fn(_p(w), _p(out), Cout, Cin, 1 if glu else 0, _stream())
    else:
        rc = fn(_p(w), _p(out), Cout, Cin, _stream())
    check(rc, name)
    return out


def pack_conv3x3_weight(w: torch.Tensor, dgrad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,3,3] -> the [ceil(Cin/4)][9][4][Cout] stream order of tgsr_conv3x3_fwd.  `dgrad`: see pack_weight."""
    return pack_weight("direct", w, False, dgrad, out)


def pack_wino_weight(w: torch.Tensor, glu: bool = False, dgrad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,3,3] -> Winograd F(2x2,3x3) transformed weights [ceil(Cin/8)][Cout/64][16 pos][8][64].  `glu`, `dgrad`: see
    pack_weight."""
    return pack_weight("wino", w, glu, dgrad, out)


def pack_wino4_weight(w: torch.Tensor, glu: bool = False, dgrad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,3,3] -> Winograd F(4x4,3x3) transformed weights [Cin/4][Cout/64][9 quads][4 ci][64 rows][4] (U = G g G^T in
    double, rounded once).  `glu`, `dgrad`: see pack_weight."""
    return pack_weight("wino4", w, glu, dgrad, out)


def pack_wino4w_weight(w: torch.Tensor, glu: bool = False, dgrad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pack of the register-fed F(4x4,3x3) kernel: per-wave fragment order [Cin/4][groups][8 | 4 blocks][9 quads][64 lanes][4]
    (128-row groups where Cout % 128 == 0, else 64-row groups) - not interchangeable with pack_wino4_weight's.  `glu`, `dgrad`: see pack_weight."""
    return pack_weight("wino4w", w, glu, dgrad, out)


def pack_upconv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] -> [ceil(Cin/4)][4 phases][4 taps][4][Cout] with the sub-pixel tap sums (tgsr_upconv3x3_glu_fwd)."""
    return pack_weight("upconv", w)


def pack_upwino_weight(w: torch.Tensor, glu: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,3,3] -> the 9 tap-sum positions of the up-sample-aware Winograd form (tgsr_upwino_glu_fwd; glu=False:
    the layout of tgsr_upwino_fwd)."""
    return pack_weight("upwino", w, glu, False, out)


def pack_upwino4_weight(w: torch.Tensor, glu: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout,Cin,3,3] -> the 25 live positions of the up-sample-aware F(4x4,3x3) form (tgsr_upwino4_fwd), the -1/3 factors of
    the fifth transformed row / column folded in; computed in double, rounded once."""
    return pack_weight("upwino4", w, glu, False, out)


def bn_fold(weight, bias, running_mean, running_var, eps: float = BN_EPS):
    """BatchNorm2d(eval) -> (scale, shift) per channel."""
    _need_hip(weight, bias, running_mean, running_var)
    C = weight.numel()
    ts = [_f32(t.detach(), "bn tensor").contiguous() for t in (weight, bias, running_mean, running_var)]
    scale = torch.empty(C, dtype=torch.float32, device=weight.device)
    shift = torch.empty_like(scale)
    check(_lib.lib().tgsr_bn_fold(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), eps, _p(scale), _p(shift), C, _stream()),
          "tgsr_bn_fold")
    return scale, shift


# ----------------------------------------------------------------------------------------- routing
WINO4_MIN_PIXELS = 64 * 64        # per image; profiles/HISTORY.md 3.1e: the error study that keeps F(4x4) off the 32 x 32 layers
WINO4_MIN_PIXELS_64 = 128 * 128   # pixels per image from which layers with 64-channel groups only may use F(4x4) too
# The up-sample-aware F(4x4) form must keep +-1 among its interpolation points (its 25-of-36 structure depends on them,
# tgsr_upwino4.hip), so it does not get the better-conditioned points of tgsr_winograd4.hip: its OWN error is 1.9-2.2x the CPU
# fp32 op's on the same input (tests/test_hip_parity_margin.py, profiles/HISTORY.md 3.1g).  It therefore serves only upBlocks whose output is
# the generator's finest feature map (>= 256 x 256: nothing but an image head reads it); an upBlock in mid-network feeds the
# 128^2 stages that amplify whatever error they are handed.
UPWINO4_MIN_OUT_PIXELS = 256 * 256
WINO4_MIN_WORKGROUPS = 256        # below a full round of its (large) workgroup tiles F(2x2)'s four times smaller ones win


class _Routing:
    """Which layers go to the F(4x4) kernels.  Read from the environment ONCE, at import (the eager host path asks per layer and
    per forward); tests and tools/ change the attributes of `ops.ROUTING` instead.
      TGSR_WINO4=0                every layer stays on F(2x2)
      TGSR_WINO4_MIN_WG=<n>       the work rule's threshold (n = 32 gives the batch-2 golden case the routing of batch 16)
      TGSR_WINO4_PIN_BATCH=<b>    decide the work rule as if the batch were b: the same kernels - bit-identical images per
                                  sample - whatever the batch size (reproducibility knob; default: the real batch)
    diagnostics (tools/diag_precision_classes.py): min_cin / min_pixels / upwino4_min_cin switch layer classes off."""

    def __init__(self, env=os.environ):
        self.wino4 = env.get("TGSR_WINO4", "1") != "0"
        self.min_workgroups = int(env.get("TGSR_WINO4_MIN_WG", WINO4_MIN_WORKGROUPS))
        self.pin_batch = int(env.get("TGSR_WINO4_PIN_BATCH", "0"))
        self.min_cin = int(env.get("TGSR_WINO4_MIN_CIN", "0"))
        self.min_pixels = int(env.get("TGSR_WINO4_MIN_PIXELS", "0"))
        self.upwino4_min_cin = int(env.get("TGSR_UPWINO4_MIN_CIN", "0"))

    def reset(self, env=os.environ):
        self.__init__(env)
        return self


ROUTING = _Routing()


def wino4_wanted(cin: int, cout: int, H: int, W: int, B: int = 16) -> bool:
    """Does a conv3x3 layer go to the F(4x4, 3x3) kernels?  Three rules.
    Shape: Cout % 64, Cin % 4, W % 64, H % 8 (whole workgroup tiles).
    Numerics (profiles/HISTORY.md 3.1e / 3.1g; tests/test_hip_parity.py::test_fp32_parity_margin_*): layers of >= 128 x 128
    pixels; at 64 x 64 .. 128 x 128 only the convolutions with 128-channel groups; nothing below 64 x 64 (the early, small layers
    are the ones whose error the rest of the network amplifies).
    Work: >= 256 workgroups of the form the layer takes (`_wino4_form`) - register-fed: 4 x 64 pixels x 128 rows, or x 64 rows
    where Cout % 128 != 0; else the LDS-fed form, 8 x 64 x 64 (measured at batch 4 .. 32: each routed layer faster than on
    F(2x2), each unrouted one slower; the batch-2 golden case stays on F(2x2) except for the last upBlocks).
    `ROUTING` holds the switches (environment, read at import)."""
    R = ROUTING
    if not R.wino4:
        return False
    if not (_wino4_shape(cin, cout, H, W) and H * W >= WINO4_MIN_PIXELS):
        return False
    if cin < R.min_cin or H * W < R.min_pixels:          # diagnostics
        return False
    if H * W < WINO4_MIN_PIXELS_64 and cout % 128 != 0:
        return False
    if R.pin_batch:
        B = R.pin_batch
    if _wino4_form(cin) == "wino4w":
        nwg = B * (H // 4) * (W // 64) * (cout // (128 if cout % 128 == 0 else 64))
    else:
        nwg = B * (H // 8) * (W // 64) * (cout // 64)
    return nwg >= R.min_workgroups


def upwino4_wanted(cin: int, cout: int, H: int, W: int, B: int = 16) -> bool:
    """Does an upBlock (low-resolution input H x W) go to the F(4x4) form of the up-sample-aware kernel?  Shape support
    (Cout % 64, Cin % 8: an even number of 4-channel stages, whole 4 x 64 OUTPUT tiles), a numerics floor on the OUTPUT
    (>= 256 x 256 pixels: the generator's last upBlock, read by an image head only - see UPWINO4_MIN_OUT_PIXELS) and at least 256
    of its 4-wave workgroups.  `ROUTING.wino4 = False` (TGSR_WINO4=0) keeps the F(2x2) form."""
    R = ROUTING
    if not R.wino4:
        return False
    Ho, Wo = 2 * H, 2 * W
    if cin < R.upwino4_min_cin:                            # diagnostics: which upBlocks cost what
        return False
    if not (FORMS["upwino4"].shape(cin, cout, H, W) and Ho * Wo >= UPWINO4_MIN_OUT_PIXELS):
        return False
    if R.pin_batch:
        B = R.pin_batch
    return B * (Ho // 4) * (Wo // 64) * (cout // 64) >= R.min_workgroups


def _aligned(t, nbytes: int) -> bool:
    """`t` (None: nothing to ask) starts on an `nbytes` boundary and its batch stride keeps every image on one."""
    return t is None or (t.data_ptr() % nbytes == 0 and (t.shape[0] == 1 or t.stride(0) % (nbytes // 4) == 0))


def _dense(t) -> bool:
    return t is None or (t.stride(3) == 1 and t.stride(2) == t.shape[3] and t.stride(1) == t.shape[2] * t.shape[3])


def conv3x3_form(x, cout: int, upsample: bool = False, glu: bool = False, out=None, residual=None, winograd: bool = True,
                 training: bool = False) -> str:
    """Which kernel form (a key of FORMS) a conv3x3 layer takes - THE routing decision; the eval-mode blocks of util.py and the
    training blocks of autograd.py all ask here.  Host arithmetic on shapes, strides and addresses (x / out / residual need
    `shape`, `stride()`, `data_ptr()` only); the library is not touched.
      winograd   util.WINOGRAD (TGSR_WINOGRAD=0: the direct kernel, and the sub-pixel form for upBlocks)
      training   the caller is autograd.py: BatchNorm's batch statistics sit between the convolution and the gate, so `glu` is
                 False there and the gated one-launch upBlock forms (upconv, upwino4) are not available.
    In order of preference.  Without up-sampling: F(4x4) where wino4_wanted routes the layer and every tensor is a dense NCHW block
    on 16 bytes; F(2x2) where the kernel takes the shape and pays - always with 64-channel groups, with 32-channel groups (Cout %
    64 != 0: 8-row workgroup tiles) only when the image gives >= 256 workgroups (measured at B=16: 32->32 @128^2 40 vs 71 us, @64^2
    16 vs 20 us, @32^2 16 vs 13 us); else the direct kernel.  With it: an eval-mode upBlock (`glu`) with whole 64-channel groups is
    ONE launch - Winograd on the up-sampled grid with the up-sampling folded into the input transform (upwino: 9 of 16 positions
    survive, 2.25 multiplies per output), its F(4x4) form (25 of 36: 1.56) where upwino4_wanted routes the layer, and the
    sub-pixel form (upconv: 4 multiplies) for what Winograd does not take; training has the un-gated upwino entry; everything
    else up-samples inside the direct kernel."""
    if x.dim() != 4:
        return "direct"       # whose wrapper refuses it
    B, cin, H, W = x.shape
    if upsample:
        f = FORMS["upwino"]
        wino = winograd and f.shape(cin, cout, H, W) and _aligned(x, 16) and _aligned(out, f.align)
        if training:
            return "upwino" if wino else "direct"
        if not (glu and FORMS["upconv"].shape(cin, cout, H, W)):
            return "direct"
        if not wino:
            return "upconv"
        return "upwino4" if upwino4_wanted(cin, cout, H, W, B) and _aligned(out, FORMS["upwino4"].align) else "upwino"
    if not winograd:
        return "direct"
    if (wino4_wanted(cin, cout, H, W, B) and _aligned(x, 16) and _dense(x) and _aligned(out, 16) and _dense(out) and
            _aligned(residual, 16) and _dense(residual)):
        return _wino4_form(cin)
    if training:
        residual = None       # what autograd.py adds in a data-gradient conv's epilogue is a gradient it has just allocated: not asked
    f = FORMS["wino"]
    if (f.shape(cin, cout, H, W) and _aligned(x, 16) and _aligned(out, f.align) and _aligned(residual, f.align) and
            (cout % 64 == 0 or B * ((W + 31) // 32) * ((H + 7) // 8) >= 256)):
        return "wino"
    return "direct"


# ----------------------------------------------------------------------------------------- convolutions
def _what(f, stats: bool) -> str:
    """The public wrapper a launch came through, for an error message."""
    return f.what + "_stats" if stats else f.what


def _conv3x3(form: str, x, pack, cout: int, scale, shift, glu: bool, upsample: bool, residual, out, stats: bool = False):
    """Validate, allocate (or check `out`), launch and bracket for `profile`: every conv3x3 form goes through here.  `stats`:
    the form's raw convolution with BatchNorm's partial sums in the epilogue; returns (out, stat_partial [cout, nslots, 2])."""
    f = FORMS[form]
    if f.gate_only and not glu:
        raise TgsrError("%s: the %s form has the GLU epilogue only" % (_what(f, stats), form))
    _need_hip(x, pack, scale, shift, residual, out)
    x, xbs = _nchw_bstride(_f32(x, "x"), "x")
    B, Cin, H, W = x.shape
    if pack.numel() != packed_elems(form, cout, Cin):
        _bad_pack(_what(f, stats), form, pack, cout, Cin)
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    co = cout // 2 if glu else cout
    L = _lib.lib()
    part = None
    if stats:
        nslots = getattr(L, f.nslots)(B, H, W, cout)
        if nslots < 1:
            raise TgsrError("%s: unsupported shape %s -> %d channels" % (_what(f, stats), tuple(x.shape), cout))
        part = torch.empty(cout, nslots, 2, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(B, co, Ho, Wo, dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, co, Ho, Wo) or out.stride(3) != 1 or out.stride(2) != Wo or out.stride(1) != Ho * Wo:
        raise TgsrError("%s: bad `out` shape/strides %s %s" % (_what(f, stats), tuple(out.shape), out.stride()))
    obs = out.stride(0) if B > 1 else co * Ho * Wo
    rbs = 0
    if residual is not None:
        if (glu and form == "direct") or not f.tail.startswith("epi"):
            raise TgsrError("%s: residual with GLU is not a reference pattern" % _what(f, stats))
        residual, rbs = _nchw_bstride(_f32(residual, "residual"), "residual")
        if tuple(residual.shape) != (B, co, Ho, Wo):
            raise TgsrError("%s: residual shape %s" % (_what(f, stats), tuple(residual.shape)))
    e0 = _ev() if profile is not None else None
    name = f.stats if stats else (f.fwd if glu or f.fwd_plain is None else f.fwd_plain)
    fn = getattr(L, name)
    if stats:
        rc = fn(_p(x), xbs, B, Cin, H, W, _p(pack), cout, _p(out), obs, _p(part), _stream())
    elif f.tail == "epi":
        rc = fn(_p(x), xbs, B, Cin, H, W, _p(pack), cout, _p(scale), _p(shift), _p(residual), rbs, _p(out), obs,
                _lib.EPI_AFFINE_GLU if glu else _lib.EPI_AFFINE, _stream())
    elif f.tail == "epi,up":
        rc = fn(_p(x), xbs, B, Cin, H, W, _p(pack), cout, _p(scale), _p(shift), _p(residual), rbs, _p(out), obs,
                _lib.EPI_AFFINE_GLU if glu else _lib.EPI_AFFINE, 1 if upsample else 0, _stream())
    elif f.tail == "glu":
        rc = fn(_p(x), xbs, B, Cin, H, W, _p(pack), cout, _p(scale), _p(shift), _p(out), obs, 1 if glu else 0, _stream())
    else:
        rc = fn(_p(x), xbs, B, Cin, H, W, _p(pack), cout, _p(scale), _p(shift), _p(out), obs, _stream())
    check(rc, name)
    if profile is not None:
        nbytes = 4 * (B * Cin * H * W + B * co * Ho * Wo * (2 if residual is not None else 1) + cout * Cin * 9)
        profile.append((f.kernel, 2.0 * B * Ho * Wo * cout * Cin * 9, nbytes, e0, _ev()))
    return (out, part) if stats else out


def conv3x3_fused(x: torch.Tensor, wpack: torch.Tensor, cout: int, scale: Optional[torch.Tensor],
                  shift: Optional[torch.Tensor], glu: bool = False, upsample: bool = False,
                  residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv3x3 [+nearest x2 in front] + per-channel affine + (GLU | residual add) in one launch.
    `out` may be a channel-slice view of a wider buffer (dense C,H,W block, any batch stride)."""
    return _conv3x3("direct", x, wpack, cout, scale, shift, glu, upsample, residual, out)


def conv3x3_wino(x: torch.Tensor, upack: torch.Tensor, cout: int, scale, shift, glu: bool = False,
                 residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv3x3 + affine + (GLU | residual) by Winograd F(2x2,3x3) (same contract as conv3x3_fused, no upsample)."""
    return _conv3x3("wino", x, upack, cout, scale, shift, glu, False, residual, out)


def conv3x3_wino4(x: torch.Tensor, upack: torch.Tensor, cout: int, scale, shift, glu: bool = False,
                  residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, wide: bool = False) -> torch.Tensor:
    """conv3x3 + affine + (GLU | residual) by Winograd F(4x4,3x3) (same contract as conv3x3_wino; 16-byte aligned tensors).
    `wide`: the register-fed form (Cin a multiple of 8), upack from pack_wino4w_weight."""
    return _conv3x3("wino4w" if wide else "wino4", x, upack, cout, scale, shift, glu, False, residual, out)


def stats_nslots(form: str, B: int, H: int, W: int, cout: int) -> int:
    """Partial-sum pairs per channel the `stats` entry of `form` writes for this shape (0: unsupported)."""
    return int(getattr(_lib.lib(), FORMS[form].nslots)(int(B), int(H), int(W), int(cout)))


def wino_stats_nslots(B: int, H: int, W: int, cout: int) -> int:
    """stats_nslots of conv3x3_wino_stats."""
    return stats_nslots("wino", B, H, W, cout)


def wino4_stats_nslots(B: int, H: int, W: int, cout: int, wide: bool = False) -> int:
    """stats_nslots of conv3x3_wino4_stats."""
    return stats_nslots("wino4w" if wide else "wino4", B, H, W, cout)


def conv3x3_wino_stats(x: torch.Tensor, upack: torch.Tensor, cout: int):
    """The raw Winograd convolution (no affine, no residual) whose epilogue also leaves BatchNorm's batch statistics as
    partial sums: returns (out [B,cout,H,W], stat_partial [cout, nslots, 2]) for bn_train_fwd(..., stat_partial=...)."""
    return _conv3x3("wino", x, upack, cout, None, None, False, False, None, None, stats=True)


def conv3x3_wino4_stats(x: torch.Tensor, upack: torch.Tensor, cout: int, wide: bool = False):
    """conv3x3_wino_stats on the F(4x4, 3x3) kernels: (out [B,cout,H,W], stat_partial [cout, nslots, 2]).  `wide`: the
    register-fed form (upack from pack_wino4w_weight)."""
    return _conv3x3("wino4w" if wide else "wino4", x, upack, cout, None, None, False, False, None, None, stats=True)


def upconv3x3_glu(x: torch.Tensor, wpack_up: torch.Tensor, cout: int, scale, shift,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """upBlock in one launch by sub-pixel decomposition (4 x 2x2 convs on the pre-upsample tensor)."""
    return _conv3x3("upconv", x, wpack_up, cout, scale, shift, True, True, None, out)


def upwino_glu(x: torch.Tensor, upack: torch.Tensor, cout: int, scale, shift,
               out: Optional[torch.Tensor] = None, glu: bool = True) -> torch.Tensor:
    """upBlock in one launch by Winograd on the up-sampled grid (9 products per 2x2 outputs); contract of upconv3x3_glu.
    glu=False: Upsample -> conv3x3 -> affine without the gate (out [B,cout,2H,2W]; scale/shift may be None)."""
    return _conv3x3("upwino", x, upack, cout, scale, shift, glu, True, None, out)


def upwino4_glu(x: torch.Tensor, upack: torch.Tensor, cout: int, scale, shift,
                out: Optional[torch.Tensor] = None, glu: bool = True) -> torch.Tensor:
    """upBlock in one launch by F(4x4,3x3) on the up-sampled grid (25 products per 4x4 outputs); contract of upwino_glu with
    16-byte aligned tensors."""
    return _conv3x3("upwino4", x, upack, cout, scale, shift, glu, True, None, out)


def conv_to3(x: torch.Tensor, w: torch.Tensor, tanh_axpy: bool = False, addend: Optional[torch.Tensor] = None,
             alpha: float = 0.0) -> torch.Tensor:
    """KxK (3|5) conv to 3 channels; tanh_axpy: tanh(conv) + alpha * addend."""
    _need_hip(x, w, addend)
    x, xbs = _nchw_bstride(_f32(x, "x"), "x")
    w = _f32(w.detach(), "w").contiguous()
    B, Cin, H, W = x.shape
    if w.shape[0] != 3 or w.shape[1] != Cin or w.shape[2] != w.shape[3]:
        raise TgsrError("conv_to3: weight shape %s" % (tuple(w.shape),))
    if addend is not None:
        addend = _f32(addend, "addend").contiguous()
        if tuple(addend.shape) != (B, 3, H, W):
            raise TgsrError("conv_to3: addend shape %s" % (tuple(addend.shape),))
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
    e0 = _ev() if profile is not None else None
    rc = _lib.lib().tgsr_conv_to3_fwd(_p(x), xbs, B, Cin, H, W, _p(w), int(w.shape[2]),
                                      _lib.ACT_TANH_AXPY if tanh_axpy else _lib.ACT_NONE, _p(addend), float(alpha),
                                      _p(out), _stream())
    check(rc, "tgsr_conv_to3_fwd")
    if profile is not None:
        K = int(w.shape[2])
        nbytes = 4 * (B * Cin * H * W + B * 3 * H * W * (2 if addend is not None else 1))
        profile.append(("conv_to3_kernel", 2.0 * B * H * W * 3 * Cin * K * K, nbytes, e0, _ev()))
    return out


def conv_to3_finish(x: torch.Tensor, w: torch.Tensor, ts, ss, alpha: float):
    """(img, fine): the closing launch of the fp32 inference step (tgsr_conv_to3_finish_fwd).  img = conv_to3(x, w), the last
    low-frequency head; fine[k] = ts[k] + alpha * ss[k] for the smaller scales (len(ss) == len(ts) - 1) and
    fine[-1] = ts[-1] + alpha * img - what axpy_images(ts, ss + [img], alpha) returns, bit for bit, without its launch and
    without reading img back.  Only shapes of the streaming head with 16-byte copies (TgsrError otherwise)."""
    import ctypes
    ts, ss = list(ts), list(ss)
    n = len(ts)
    if n < 1 or n > 3 or len(ss) != n - 1:
        raise TgsrError("conv_to3_finish: %d / %d images (1..3 scales, one low-frequency image fewer)" % (n, len(ss)))
    _need_hip(x, w, *ts, *ss)
    x, xbs = _nchw_bstride(_f32(x, "x"), "x")
    w = _f32(w.detach(), "w").contiguous()
    B, Cin, H, W = x.shape
    if w.shape[0] != 3 or w.shape[1] != Cin or w.shape[2] != w.shape[3]:
        raise TgsrError("conv_to3_finish: weight shape %s" % (tuple(w.shape),))
    ts = [_f32(t, "t").contiguous() for t in ts]
    ss = [_f32(s_, "s").contiguous() for s_ in ss]
    if tuple(ts[-1].shape) != (B, 3, H, W):
        raise TgsrError("conv_to3_finish: last scale %s against a %s head" % (tuple(ts[-1].shape), (B, 3, H, W)))
    for t, s_ in zip(ts, ss):
        if t.shape != s_.shape:
            raise TgsrError("conv_to3_finish: %s + alpha * %s" % (tuple(t.shape), tuple(s_.shape)))
    img = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
    fine = [torch.empty_like(t) for t in ts]
    tp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    sp = (ctypes.c_void_p * n)(*([s_.data_ptr() for s_ in ss] + [None]))
    fp = (ctypes.c_void_p * n)(*[o.data_ptr() for o in fine])
    ne = (ctypes.c_int64 * n)(*[t.numel() for t in ts])
    e0 = _ev() if profile is not None else None
    rc = _lib.lib().tgsr_conv_to3_finish_fwd(_p(x), xbs, B, Cin, H, W, _p(w), int(w.shape[2]), _p(img), n, fp, tp, sp, ne,
                                             float(alpha), _stream())
    check(rc, "tgsr_conv_to3_finish_fwd")
    if profile is not None:
        K = int(w.shape[2])
        nbytes = 4 * (B * Cin * H * W + B * 3 * H * W) + 4 * sum(3 * t.numel() for t in ts) - 4 * ts[-1].numel()
        profile.append(("conv_to3_kernel", 2.0 * B * H * W * 3 * Cin * K * K, nbytes, e0, _ev()))
    return img, fine


# ----------------------------------------------------------------------------------------- attention
_MASK_CACHE = [None, None, None]   # (tensor id/version key, source (kept alive), uint8 copy)


def _mask_u8(mask: torch.Tensor) -> torch.Tensor:
    """bool -> uint8 once per mask tensor (the three generator stages share one mask)."""
    if mask.dtype == torch.uint8 and mask.is_contiguous():
        return mask
    if mask.dtype == torch.bool and mask.is_contiguous():
        return mask.view(torch.uint8)                    # torch.bool storage is one byte 0 / 1: no cast kernel
    key = (mask.data_ptr(), mask._version, tuple(mask.shape), mask.dtype)
    if _MASK_CACHE[0] != key or _MASK_CACHE[1] is not mask:
        _MASK_CACHE[0], _MASK_CACHE[1], _MASK_CACHE[2] = key, mask, mask.to(torch.uint8).contiguous()
    return _MASK_CACHE[2]


def word_project(words: torch.Tensor, w_ctxs) -> list:
    """The conv1x1 of GlobalAttentionGeneral (GlobalAttention.py:100-102) for up to 4 weight sets over the same words in
    one launch: words [B,cdf,T], w_ctxs = list of [idf,cdf(,1,1)] -> list of src [B,idf,32] (zero padded words),
    to be handed to word_attention(src=...)."""
    import ctypes
    _need_hip(words, *w_ctxs)
    words = _f32(words, "words").contiguous()
    B, cdf, T = words.shape
    n = len(w_ctxs)
    idf = w_ctxs[0].shape[0]
    ws = [_f32(w.detach(), "w_ctx").reshape(idf, cdf).contiguous() for w in w_ctxs]
    out = torch.empty(n, B, idf, 32, dtype=torch.float32, device=words.device)
    ptrs = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    check(_lib.lib().tgsr_word_project_fwd(_p(words), ptrs, n, B, idf, cdf, T, _p(out), _stream()),
          "tgsr_word_project_fwd")
    return [out[i] for i in range(n)]


def word_attention(h: torch.Tensor, words: torch.Tensor, w_ctx: torch.Tensor, mask: Optional[torch.Tensor],
                   correct_mask: bool = False, out: Optional[torch.Tensor] = None, need_attn: bool = True,
                   src: Optional[torch.Tensor] = None):
    """GlobalAttentionGeneral.forward: h [B,idf,ih,iw], words [B,cdf,T], w_ctx [idf,cdf(,1,1)], mask bool [B,T].
    Returns (c_code [B,idf,ih,iw], attn [B,T,ih,iw]).  `src` = this layer's word_project output (skips the projection)."""
    _need_hip(h, words, w_ctx, mask, out)
    h, hbs = _nchw_bstride(_f32(h, "h"), "h")
    B, idf, ih, iw = h.shape
    words = _f32(words, "words").contiguous()
    cdf, T = words.shape[1], words.shape[2]
    w2 = _f32(w_ctx.detach(), "w_ctx").reshape(idf, cdf).contiguous()
    m8 = None
    if mask is not None:
        if tuple(mask.shape) != (B, T):
            raise TgsrError("word_attention: mask shape %s, expected %s" % (tuple(mask.shape), (B, T)))
        m8 = _mask_u8(mask)
    Q = ih * iw
    if out is None:
        out = torch.empty(B, idf, ih, iw, dtype=torch.float32, device=h.device)
    if tuple(out.shape) != (B, idf, ih, iw) or out.stride(3) != 1 or out.stride(2) != iw or out.stride(1) != Q:
        raise TgsrError("word_attention: bad `out`")
    cbs = out.stride(0) if B > 1 else idf * Q
    attn = torch.empty(B, T, ih, iw, dtype=torch.float32, device=h.device) if need_attn else None
    if src is not None:
        if tuple(src.shape) != (B, idf, 32) or not src.is_contiguous():
            raise TgsrError("word_attention: bad `src` %s" % (tuple(src.shape),))
        ws, wp, w2p = src, None, None
    else:
        ws, wp, w2p = torch.empty(B * idf * 32, dtype=torch.float32, device=h.device), _p(words), _p(w2)
    e0 = _ev() if profile is not None else None
    rc = _lib.lib().tgsr_word_attention_fwd(_p(h), hbs, wp, w2p, _p(m8), 1 if correct_mask else 0, B, idf,
                                            cdf, T, Q, _p(ws), _p(out), cbs, _p(attn), _stream())
    check(rc, "tgsr_word_attention_fwd")
    if profile is not None:
        nbytes = 4 * B * Q * (2 * idf + (T if need_attn else 0))
        profile.append(("word_attention_kernel", 4.0 * B * Q * idf * T, nbytes, e0, _ev()))
    return out, attn


# ----------------------------------------------------------------------------------------- text encoder
_LENS_CACHE = {}


def _lens_on_device(lens: tuple, dev) -> torch.Tensor:
    """int32 caption lengths on the device; cached so a steady-state step issues no blocking H2D copy."""
    key = (lens, str(dev))
    t = _LENS_CACHE.pop(key, None)
    if t is None:
        if len(_LENS_CACHE) >= 256:
            _LENS_CACHE.pop(next(iter(_LENS_CACHE)))         # least recently used (dicts keep insertion order; hits re-insert)
        t = torch.tensor(lens, dtype=torch.int32).to(dev)
    _LENS_CACHE[key] = t
    if t.is_cuda:
        # the caller reads it on the CURRENT stream, which need not be the one it was allocated on (stream lanes share the
        # cache): an evicted entry's memory must not be handed out again while such a read is pending
        t.record_stream(torch.cuda.current_stream(t.device))
    return t


def bilstm(captions: torch.Tensor, cap_lens, emb: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
           b_ih: torch.Tensor, b_hh: torch.Tensor):
    """captions int64 [B,W]; cap_lens list/tensor (host or device) ; emb [ntoken,ninput]; w_* stacked over the two
    directions [2,4H,*].  Returns (words_emb [B,2H,Tmax], sent_emb [B,2H])."""
    _need_hip(captions, emb, w_ih, w_hh, b_ih, b_hh)
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    B, width = captions.shape
    if len(lens) != B or min(lens) < 1 or max(lens) > width:
        raise TgsrError("bilstm: cap_lens %s invalid for captions %s" % (lens, tuple(captions.shape)))
    Tmax = max(lens)
    H = w_hh.shape[2]
    dev = emb.device
    captions = captions.to(torch.int64).contiguous()
    lens_d = _lens_on_device(tuple(lens), dev)
    gates = torch.empty(B * Tmax * 8 * H, dtype=torch.float32, device=dev)
    words = torch.empty(B, 2 * H, Tmax, dtype=torch.float32, device=dev)
    sent = torch.empty(B, 2 * H, dtype=torch.float32, device=dev)
    ts = [_f32(t.detach(), "lstm tensor").contiguous() for t in (emb, w_ih, w_hh, b_ih, b_hh)]
    rc = _lib.lib().tgsr_bilstm_fwd(_p(captions), width, _p(lens_d), B, Tmax, _p(ts[0]), emb.shape[0], emb.shape[1],
                                    _p(ts[1]), _p(ts[2]), _p(ts[3]), _p(ts[4]), H, _p(gates), _p(words), _p(sent),
                                    _stream())
    check(rc, "tgsr_bilstm_fwd")
    return words, sent


def bilstm_train_fwd(x: torch.Tensor, cap_lens, w_ih, w_hh, b_ih, b_hh):
    """Training forward on embedded inputs x [B,Tmax,ninput]: returns (words_emb, sent_emb, acts) where acts
    [B,Tmax,2,5,H] holds the gate activations / cell states tgsr_bilstm_bwd needs."""
    _need_hip(x, w_ih, w_hh, b_ih, b_hh)
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    B, Tmax, K = x.shape
    if len(lens) != B or min(lens) < 1 or max(lens) > Tmax:
        raise TgsrError("bilstm_train_fwd: cap_lens %s invalid for x %s" % (lens, tuple(x.shape)))
    H = w_hh.shape[2]
    dev = x.device
    ts = [_f32(t.detach(), "lstm tensor").contiguous() for t in (x, w_ih, w_hh, b_ih, b_hh)]
    gates = torch.empty(B * Tmax * 8 * H, dtype=torch.float32, device=dev)
    acts = torch.zeros(B, Tmax, 2, 5, H, dtype=torch.float32, device=dev)
    words = torch.empty(B, 2 * H, Tmax, dtype=torch.float32, device=dev)
    sent = torch.empty(B, 2 * H, dtype=torch.float32, device=dev)
    rc = _lib.lib().tgsr_bilstm_train_fwd(_p(ts[0]), _p(_lens_on_device(tuple(lens), dev)), B, Tmax, K, _p(ts[1]),
                                          _p(ts[2]), _p(ts[3]), _p(ts[4]), H, _p(gates), _p(acts), _p(words), _p(sent),
                                          _stream())
    check(rc, "tgsr_bilstm_train_fwd")
    return words, sent, acts


def bilstm_bwd(cap_lens, w_hh, acts, words, d_words, d_sent):
    """BPTT of both directions: returns (dgates [B,Tmax,2,4H], hprev [B,Tmax,2,H], dbias [2,4H])."""
    _need_hip(w_hh, acts, words, d_words, d_sent)
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    B, Tmax, _, _, H = acts.shape
    dev = acts.device
    dgates = torch.empty(B, Tmax, 2, 4 * H, dtype=torch.float32, device=dev)
    hprev = torch.empty(B, Tmax, 2, H, dtype=torch.float32, device=dev)
    dbias = torch.empty(2, 4 * H, dtype=torch.float32, device=dev)
    dw = _f32(d_words, "d_words").contiguous()
    ds = None if d_sent is None else _f32(d_sent, "d_sent").contiguous()
    rc = _lib.lib().tgsr_bilstm_bwd(_p(_lens_on_device(tuple(lens), dev)), B, Tmax, H,
                                    _p(_f32(w_hh.detach(), "w_hh").contiguous()), _p(acts), _p(words.contiguous()),
                                    _p(dw), _p(ds), _p(dgates), _p(hprev), _p(dbias), _stream())
    check(rc, "tgsr_bilstm_bwd")
    return dgates, hprev, dbias


def bigru_train_fwd(x: torch.Tensor, cap_lens, w_ih, w_hh, b_ih, b_hh):
    """Training forward of the bidirectional GRU on embedded inputs x [B,Tmax,ninput] (w_* stacked over the two directions:
    [2,3H,ninput], [2,3H,H], [2,3H]): returns (words_emb [B,2H,Tmax], sent_emb [B,2H], acts [B,Tmax,2,4,H])."""
    _need_hip(x, w_ih, w_hh, b_ih, b_hh)
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    B, Tmax, K = x.shape
    if len(lens) != B or min(lens) < 1 or max(lens) > Tmax:
        raise TgsrError("bigru_train_fwd: cap_lens %s invalid for x %s" % (lens, tuple(x.shape)))
    H = w_hh.shape[2]
    dev = x.device
    ts = [_f32(t.detach(), "gru tensor").contiguous() for t in (x, w_ih, w_hh, b_ih, b_hh)]
    b_rz = ts[4].clone()
    b_rz[:, 2 * H:] = 0
    b_hn = ts[4][:, 2 * H:].contiguous()
    gates = torch.empty(B * Tmax * 6 * H, dtype=torch.float32, device=dev)
    acts = torch.empty(B, Tmax, 2, 4, H, dtype=torch.float32, device=dev)
    words = torch.empty(B, 2 * H, Tmax, dtype=torch.float32, device=dev)
    sent = torch.empty(B, 2 * H, dtype=torch.float32, device=dev)
    rc = _lib.lib().tgsr_bigru_train_fwd(_p(ts[0]), _p(_lens_on_device(tuple(lens), dev)), B, Tmax, K, _p(ts[1]), _p(ts[2]),
                                         _p(ts[3]), _p(b_rz), _p(b_hn), H, _p(gates), _p(acts), _p(words), _p(sent), _stream())
    check(rc, "tgsr_bigru_train_fwd")
    return words, sent, acts


def bigru_bwd(cap_lens, w_hh, acts, words, d_words, d_sent):
    """BPTT of both directions: (dgx [B,Tmax,2,3H], dgh [B,Tmax,2,3H], hprev [B,Tmax,2,H], dbias [2,2,3H] = (d b_ih, d b_hh))."""
    _need_hip(w_hh, acts, words, d_words, d_sent)
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    B, Tmax, _, _, H = acts.shape
    dev = acts.device
    dgx = torch.empty(B, Tmax, 2, 3 * H, dtype=torch.float32, device=dev)
    dgh = torch.empty(B, Tmax, 2, 3 * H, dtype=torch.float32, device=dev)
    hprev = torch.empty(B, Tmax, 2, H, dtype=torch.float32, device=dev)
    dbias = torch.empty(2, 2, 3 * H, dtype=torch.float32, device=dev)
    dw = _f32(d_words, "d_words").contiguous()
    ds = None if d_sent is None else _f32(d_sent, "d_sent").contiguous()
    rc = _lib.lib().tgsr_bigru_bwd(_p(_lens_on_device(tuple(lens), dev)), B, Tmax, H, _p(_f32(w_hh.detach(), "w_hh").contiguous()),
                                   _p(acts), _p(words.contiguous()), _p(dw), _p(ds), _p(dgx), _p(dgh), _p(hprev), _p(dbias), _stream())
    check(rc, "tgsr_bigru_bwd")
    return dgx, dgh, hprev, dbias


def lstm_gate_table(emb, w_ih, b_ih, b_hh):
    """[ntoken, 2, 4H] gate pre-activations of every token (eval mode, frozen weights); see tgsr_lstm_gate_table."""
    _need_hip(emb, w_ih, b_ih, b_hh)
    ts = [_f32(t.detach(), "lstm tensor").contiguous() for t in (emb, w_ih, b_ih, b_hh)]
    H = w_ih.shape[1] // 4
    table = torch.empty(emb.shape[0], 2, 4 * H, dtype=torch.float32, device=emb.device)
    check(_lib.lib().tgsr_lstm_gate_table(_p(ts[0]), emb.shape[0], emb.shape[1], _p(ts[1]), _p(ts[2]), _p(ts[3]), H,
                                          _p(table), _stream()), "tgsr_lstm_gate_table")
    return table


def gru_gate_table(emb, w_ih, b_ih, b_hh):
    """[ntoken, 2, 3H] gate pre-activations of every token for the GRU encoder (tgsr_gru_gate_table): b_hh's r and z thirds
    fold into the table, its n third stays with the recurrence (returned as b_hn [2, H])."""
    _need_hip(emb, w_ih, b_ih, b_hh)
    ts = [_f32(t.detach(), "gru tensor").contiguous() for t in (emb, w_ih, b_ih, b_hh)]
    H = w_ih.shape[1] // 3
    b_rz = ts[3].clone()
    b_rz[:, 2 * H:] = 0
    b_hn = ts[3][:, 2 * H:].contiguous()
    table = torch.empty(emb.shape[0], 2, 3 * H, dtype=torch.float32, device=emb.device)
    check(_lib.lib().tgsr_gru_gate_table(_p(ts[0]), emb.shape[0], emb.shape[1], _p(ts[1]), _p(ts[2]), _p(b_rz), H, _p(table),
                                         _stream()), "tgsr_gru_gate_table")
    return table, b_hn


def bigru_table(captions, cap_lens, table, w_hh, b_hn):
    """The bidirectional GRU recurrence over a per-token gate table (one launch): (words_emb, sent_emb); cap_lens on the host
    (-> T_max columns) or as a device int32 tensor (-> full caption width, see bilstm_table)."""
    _need_hip(captions, table, w_hh, b_hn)
    B, width = captions.shape
    H, dev = w_hh.shape[2], table.device
    if torch.is_tensor(cap_lens) and cap_lens.is_cuda:
        if cap_lens.dtype != torch.int32 or cap_lens.numel() != B or not cap_lens.is_contiguous():
            raise TgsrError("bigru: device cap_lens must be a contiguous int32 [%d] tensor" % B)
        Tmax, lens_d = width, cap_lens
    else:
        lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
        if len(lens) != B or min(lens) < 1 or max(lens) > width:
            raise TgsrError("bigru: cap_lens %s invalid for captions %s" % (lens, tuple(captions.shape)))
        Tmax, lens_d = max(lens), _lens_on_device(tuple(lens), dev)
    captions = captions.to(torch.int64).contiguous()
    words = torch.empty(B, 2 * H, Tmax, dtype=torch.float32, device=dev)
    sent = torch.empty(B, 2 * H, dtype=torch.float32, device=dev)
    rc = _lib.lib().tgsr_bigru_table_fwd(_p(captions), width, _p(lens_d), B, Tmax, _p(table), table.shape[0],
                                         _p(_f32(w_hh.detach(), "w_hh").contiguous()), _p(_f32(b_hn, "b_hn").contiguous()), H,
                                         _p(words), _p(sent), _stream())
    check(rc, "tgsr_bigru_table_fwd")
    return words, sent


def bilstm_table(captions, cap_lens, table, w_hh):
    """The BiLSTM recurrence over a per-token gate table (one launch).  Returns (words_emb, sent_emb).

    cap_lens on the HOST (list / CPU tensor): words_emb is [B, 2H, max(cap_lens)] like the reference's
    pad_packed_sequence output (util.py:250-253).  cap_lens as a DEVICE int32 tensor [B]: the lengths are read by the
    kernel only - nothing of the launch (shapes, grid, arguments) depends on their values, so the step can be captured
    once and replayed on any batch; words_emb is then [B, 2H, captions.size(1)] with zeros behind each caption, and the
    caller crops to the batch's longest caption on its side (SRPipeline / GraphedStep do)."""
    _need_hip(captions, table, w_hh)
    B, width = captions.shape
    H, dev = w_hh.shape[2], table.device
    if torch.is_tensor(cap_lens) and cap_lens.is_cuda:
        if cap_lens.dtype != torch.int32 or cap_lens.numel() != B or not cap_lens.is_contiguous():
            raise TgsrError("bilstm: device cap_lens must be a contiguous int32 [%d] tensor, got %s %s"
                            % (B, cap_lens.dtype, tuple(cap_lens.shape)))
        _need_hip(cap_lens)
        Tmax, lens_d = width, cap_lens
    else:
        lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
        if len(lens) != B or min(lens) < 1 or max(lens) > width:
            raise TgsrError("bilstm: cap_lens %s invalid for captions %s" % (lens, tuple(captions.shape)))
        Tmax, lens_d = max(lens), _lens_on_device(tuple(lens), dev)
    captions = captions.to(torch.int64).contiguous()
    words = torch.empty(B, 2 * H, Tmax, dtype=torch.float32, device=dev)
    sent = torch.empty(B, 2 * H, dtype=torch.float32, device=dev)
    w = _f32(w_hh.detach(), "w_hh").contiguous()
    rc = _lib.lib().tgsr_bilstm_table_fwd(_p(captions), width, _p(lens_d), B, Tmax, _p(table),
                                          table.shape[0], _p(w), H, _p(words), _p(sent), _stream())
    check(rc, "tgsr_bilstm_table_fwd")
    return words, sent


# ----------------------------------------------------------------------------------------- DAMSM
def damsm_words_similarity(img_features: torch.Tensor, words_emb: torch.Tensor, cap_lens, gamma1: float,
                           gamma2: float, need_att: bool = True):
    """All (image j, caption i) word-level similarities in one launch: returns (sim [B,B] = log sum_w exp(gamma2 *
    cos), att_diag [B,Tw,ih,iw] or None).  img_features [B,ndf,ih,iw], words_emb [B,ndf,Tw]."""
    _need_hip(img_features, words_emb)
    B, ndf, ih, iw = img_features.shape
    Tw = words_emb.shape[2]
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    if len(lens) != B or min(lens) < 1 or max(lens) > Tw:
        raise TgsrError("damsm: cap_lens %s invalid for words %s" % (lens, tuple(words_emb.shape)))
    ctx = _f32(img_features, "img_features").contiguous()
    words = _f32(words_emb, "words_emb").contiguous()
    dev = ctx.device
    sim = torch.empty(B, B, dtype=torch.float32, device=dev)
    att = torch.empty(B, Tw, ih, iw, dtype=torch.float32, device=dev) if need_att else None
    rc = _lib.lib().tgsr_damsm_words_fwd(_p(words), _p(_lens_on_device(tuple(lens), dev)), _p(ctx), B, ndf, Tw,
                                         ih * iw, float(gamma1), float(gamma2), _p(sim), _p(att), _stream())
    check(rc, "tgsr_damsm_words_fwd")
    return sim, att


def damsm_words_bwd(img_features: torch.Tensor, words_emb: torch.Tensor, cap_lens, gamma1: float, gamma2: float,
                    grad_sim: torch.Tensor):
    """Backward of damsm_words_similarity: grad_sim [B,B] -> (grad_img_features [B,ndf,ih,iw], grad_words [B,ndf,Tw])."""
    _need_hip(img_features, words_emb, grad_sim)
    B, ndf, ih, iw = img_features.shape
    Tw, S = words_emb.shape[2], ih * iw
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    ctx = _f32(img_features.detach(), "img_features").contiguous()
    words = _f32(words_emb.detach(), "words_emb").contiguous()
    gs = _f32(grad_sim, "grad_sim").contiguous()
    dev = ctx.device
    L = _lib.lib()
    ws = torch.empty(L.tgsr_damsm_words_bwd_ws_elems(B, ndf, S), dtype=torch.float32, device=dev)
    gw32 = torch.empty(B, ndf, 32, dtype=torch.float32, device=dev)
    gctx = torch.empty(B, ndf, ih, iw, dtype=torch.float32, device=dev)
    rc = L.tgsr_damsm_words_bwd(_p(words), _p(_lens_on_device(tuple(lens), dev)), _p(ctx), _p(gs), B, ndf, Tw, S,
                                float(gamma1), float(gamma2), _p(ws), _p(gw32), _p(gctx), _stream())
    check(rc, "tgsr_damsm_words_bwd")
    return gctx, gw32[:, :, :Tw].contiguous()


def func_attention(query: torch.Tensor, context: torch.Tensor, gamma1: float):
    """GlobalAttention.func_attention: query [B,ndf,L], context [B,ndf,ih,iw] -> (weightedContext [B,ndf,L],
    attn [B,L,ih,iw])."""
    _need_hip(query, context)
    B, ndf, L = query.shape
    ih, iw = context.shape[2], context.shape[3]
    q = _f32(query, "query").contiguous()
    c = _f32(context, "context").contiguous()
    wc = torch.empty(B, ndf, L, dtype=torch.float32, device=q.device)
    attn = torch.empty(B, L, ih, iw, dtype=torch.float32, device=q.device)
    rc = _lib.lib().tgsr_func_attention_fwd(_p(q), _p(c), B, ndf, L, ih * iw, float(gamma1), _p(wc), _p(attn),
                                            _stream())
    check(rc, "tgsr_func_attention_fwd")
    return wc, attn


# ----------------------------------------------------------------------------------------- text-image retrieval
def check_candidates(cand: torch.Tensor, N: int, M: int) -> torch.Tensor:
    """The host check of a CPU candidate table: int [N, K] with entries in [-1, M) (-1 = an empty slot).  Returns it as a
    contiguous int32 tensor, still on the host."""
    if cand.is_cuda:
        raise TgsrError("check_candidates reads a host tensor (a device table is taken as it is)")
    if cand.dtype not in (torch.int32, torch.int64) or cand.dim() != 2 or cand.shape[0] != N or cand.shape[1] < 1:
        raise TgsrError("cand must be an int32 / int64 [N = %d, K >= 1] tensor, got %s %s" % (N, cand.dtype, tuple(cand.shape)))
    lo, hi = int(cand.min()), int(cand.max())
    if lo < -1 or hi >= M:
        raise TgsrError("cand entries must be in [-1, %d) (-1 = an empty slot), got [%d, %d]" % (M, lo, hi))
    return cand.to(torch.int32).contiguous()


def _candidates(cand, N: int, M: int, dev):
    """(device int32 table or None, K).  A host table is range-checked before the upload; a device table is taken as it is (the
    kernels treat an entry outside [0, M) as an empty slot)."""
    if cand is None:
        return None, M
    if not cand.is_cuda:
        return check_candidates(cand, N, M).to(dev), cand.shape[1]
    if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != N or cand.shape[1] < 1:
        raise TgsrError("a device cand must be an int32 [N = %d, K >= 1] tensor, got %s %s" % (N, cand.dtype, tuple(cand.shape)))
    return cand.contiguous(), cand.shape[1]


def damsm_gallery(img_features: torch.Tensor, words_emb: torch.Tensor, cap_lens, gamma1: float, gamma2: float,
                  cand: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Word-level similarities of N images against candidate captions out of a pool of M, one launch: sim [N, K] with
    sim[n][k] = log sum_w exp(gamma2 * cos) of image n and caption cand[n][k] (what damsm_words_similarity gives the pair).
    img_features [N,ndf,ih,iw], words_emb [M,ndf,Tw], cap_lens M ints, cand int [N,K] (host: checked to lie in [-1, M); device: taken
    as it is) or None = every caption (K = M).  An empty slot (-1) scores -inf.  Evaluation only: no backward."""
    _need_hip(img_features, words_emb, cand if cand is not None and cand.is_cuda else None)
    if img_features.dim() != 4 or words_emb.dim() != 3 or img_features.shape[1] != words_emb.shape[1]:
        raise TgsrError("damsm_gallery: img_features [N,ndf,ih,iw] and words_emb [M,ndf,Tw] expected, got %s and %s"
                        % (tuple(img_features.shape), tuple(words_emb.shape)))
    N, ndf, ih, iw = img_features.shape
    M, _, Tw = words_emb.shape
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    if len(lens) != M or min(lens) < 1 or max(lens) > Tw:
        raise TgsrError("damsm_gallery: cap_lens %s invalid for words %s" % (lens, tuple(words_emb.shape)))
    ctx = _f32(img_features.detach(), "img_features").contiguous()
    words = _f32(words_emb.detach(), "words_emb").contiguous()
    dev = ctx.device
    cand_d, K = _candidates(cand, N, M, dev)
    sim = torch.empty(N, K, dtype=torch.float32, device=dev)
    rc = _lib.lib().tgsr_damsm_gallery_fwd(_p(words), _p(_lens_on_device(tuple(lens), dev)), _p(ctx), _p(cand_d), N, M, K, ndf, Tw,
                                           ih * iw, float(gamma1), float(gamma2), _p(sim), _stream())
    check(rc, "tgsr_damsm_gallery_fwd")
    return sim


def sent_gallery(cnn_code: torch.Tensor, rnn_code: torch.Tensor, eps: float, gamma3: float,
                 cand: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sentence-level similarities: sim [N, K] = gamma3 * cos(cnn_code[n], rnn_code[cand[n][k]]) with the reference's clamp of the
    norm product at eps (losses.py:234-250).  cnn_code [N,ndf], rnn_code [M,ndf]; cand as in damsm_gallery."""
    _need_hip(cnn_code, rnn_code, cand if cand is not None and cand.is_cuda else None)
    if cnn_code.dim() != 2 or rnn_code.dim() != 2 or cnn_code.shape[1] != rnn_code.shape[1]:
        raise TgsrError("sent_gallery: cnn_code [N,ndf] and rnn_code [M,ndf] expected, got %s and %s"
                        % (tuple(cnn_code.shape), tuple(rnn_code.shape)))
    N, ndf = cnn_code.shape
    M = rnn_code.shape[0]
    x = _f32(cnn_code.detach(), "cnn_code").contiguous()
    y = _f32(rnn_code.detach(), "rnn_code").contiguous()
    cand_d, K = _candidates(cand, N, M, x.device)
    sim = torch.empty(N, K, dtype=torch.float32, device=x.device)
    rc = _lib.lib().tgsr_sent_gallery_fwd(_p(x), _p(y), _p(cand_d), N, M, K, ndf, float(eps), float(gamma3), _p(sim), _stream())
    check(rc, "tgsr_sent_gallery_fwd")
    return sim


def retrieval_ranks(sim: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """rank [N] int32: the position of column target[n] in a stable descending sort of row n of sim [N, K], by counting (no sort);
    -1 where target[n] is outside [0, K).  target: int32 [N] on the device."""
    _need_hip(sim, target)
    if sim.dim() != 2 or target.dim() != 1 or target.shape[0] != sim.shape[0] or target.dtype != torch.int32:
        raise TgsrError("retrieval_ranks: sim [N,K] float32 and target [N] int32 expected, got %s and %s %s"
                        % (tuple(sim.shape), target.dtype, tuple(target.shape)))
    s = _f32(sim, "sim").contiguous()
    N, K = s.shape
    rank = torch.empty(N, dtype=torch.int32, device=s.device)
    rc = _lib.lib().tgsr_retrieval_ranks(_p(s), _p(target.contiguous()), N, K, _p(rank), _stream())
    check(rc, "tgsr_retrieval_ranks")
    return rank


# ----------------------------------------------------------------------------------------- distribution distances
def _feature_rows(t: torch.Tensor, name: str):
    """(tensor, row stride in floats) of a float32 [n, D] feature matrix: a view with unit column stride is taken as it is (a
    column slice of a wider matrix), anything else is copied."""
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise TgsrError("%s must be a float32 [n >= 1, D >= 1] matrix, got %s" % (name, tuple(t.shape)))
    t = _f32(t.detach(), name)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def feat_moments_add(x: torch.Tensor, sum: torch.Tensor, outer: torch.Tensor) -> None:
    """sum[i] += sum_r x[r][i] and outer[i][j] += sum_r x[r][i] x[r][j] in fp64, one launch (tgsr_feat_moments_add).  x float32
    [n, D] (any row stride >= D), sum float64 [D], outer float64 [D, D], both dense and updated in place.  Of `outer` only the
    block-upper part (i // 64 <= j // 64) is read and written: featdist.FeatureMoments mirrors the upper triangle."""
    _need_hip(x, sum, outer)
    xs, ldx = _feature_rows(x, "x")
    n, D = xs.shape
    if (sum.dtype != torch.float64 or outer.dtype != torch.float64 or tuple(sum.shape) != (D,) or tuple(outer.shape) != (D, D)
            or not sum.is_contiguous() or not outer.is_contiguous()):
        raise TgsrError("feat_moments_add: sum float64 [%d] and outer float64 [%d, %d], dense, expected; got %s %s and %s %s"
                        % (D, D, D, sum.dtype, tuple(sum.shape), outer.dtype, tuple(outer.shape)))
    rc = _lib.lib().tgsr_feat_moments_add(_p(xs), n, D, ldx, _p(sum), _p(outer), _stream())
    check(rc, "tgsr_feat_moments_add")


def check_subset_table(table: torch.Tensor, n: int, name: str = "table") -> torch.Tensor:
    """The host check of a subset table: int [S >= 1, m >= 2] with entries in [0, n).  Returns it as a contiguous int32 host
    tensor or raises TgsrError.  Touches no device."""
    if table.is_cuda:
        raise TgsrError("check_subset_table reads a host tensor (a device table is taken as it is)")
    if table.dtype not in (torch.int32, torch.int64) or table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 2:
        raise TgsrError("%s must be an int32 / int64 [S >= 1, m >= 2] tensor, got %s %s" % (name, table.dtype, tuple(table.shape)))
    lo, hi = int(table.min()), int(table.max())
    if lo < 0 or hi >= n:
        raise TgsrError("%s entries must be in [0, %d), got [%d, %d]" % (name, n, lo, hi))
    return table.to(torch.int32).contiguous()


def _subset_table(table, n, name, dev):
    if not table.is_cuda:
        return check_subset_table(table, n, name).to(dev)
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 2:
        raise TgsrError("a device %s must be an int32 [S >= 1, m >= 2] tensor, got %s %s" % (name, table.dtype, tuple(table.shape)))
    return table.contiguous()


def poly_mmd_sums(x: torch.Tensor, y: torch.Tensor, ix: torch.Tensor, iy: torch.Tensor) -> torch.Tensor:
    """The three kernel sums of KID for S subsets of m rows (tgsr_poly_mmd_sums): out float64 [S, 3] = (sum_{i != j} k(x_i, x_j),
    sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)) over the rows ix[s] of x and iy[s] of y, k(a, b) = (<a, b> / D + 1)^3 in fp64.
    x float32 [nx, D], y float32 [ny, D]; ix, iy int [S, m] (host: checked to lie in [0, nx) / [0, ny), then uploaded; device: int32,
    taken as they are - the kernel scores an entry outside the set as a row of zeros)."""
    _need_hip(x, y, ix if ix.is_cuda else None, iy if iy.is_cuda else None)
    xs, ldx = _feature_rows(x, "x")
    ys, ldy = _feature_rows(y, "y")
    (nx, D), ny = xs.shape, ys.shape[0]
    if ys.shape[1] != D:
        raise TgsrError("poly_mmd_sums: x %s and y %s differ in their feature width" % (tuple(xs.shape), tuple(ys.shape)))
    tx, ty = _subset_table(ix, nx, "ix", xs.device), _subset_table(iy, ny, "iy", xs.device)
    if tuple(tx.shape) != tuple(ty.shape):
        raise TgsrError("poly_mmd_sums: ix %s and iy %s differ in shape" % (tuple(tx.shape), tuple(ty.shape)))
    S, m = tx.shape
    L = _lib.lib()
    ws = L.tgsr_poly_mmd_ws_elems(S, m)
    if ws < 1:
        raise TgsrError("poly_mmd_sums: %d subsets of %d rows refused" % (S, m))
    work = torch.empty(ws, dtype=torch.float64, device=xs.device)
    out = torch.empty(S, 3, dtype=torch.float64, device=xs.device)
    rc = L.tgsr_poly_mmd_sums(_p(xs), nx, ldx, _p(ys), ny, ldy, _p(tx), _p(ty), S, m, D, _p(work), _p(out), _stream())
    check(rc, "tgsr_poly_mmd_sums")
    return out


# ----------------------------------------------------------------------------------------- CNN_ENCODER heads
CONV1X1_GCONV = os.environ.get("TGSR_CONV1X1_GCONV", "1") != "0"


def conv1x1(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """1x1 convolution [B,Cin,H,W] -> [B,Cout,H,W] (emb_features, util.py:300,367) as an MFMA GEMM."""
    _need_hip(x, w, bias)
    x = _f32(x, "x").contiguous()
    B, Cin, H, W = x.shape
    w2 = _f32(w.detach(), "w").reshape(w.shape[0], -1).contiguous()
    if w2.shape[1] != Cin:
        raise TgsrError("conv1x1: weight %s vs input channels %d" % (tuple(w.shape), Cin))
    out = torch.empty(B, w2.shape[0], H, W, dtype=torch.float32, device=x.device)
    if bias is None and Cin % 16 == 0 and B * H * W >= 1024 and CONV1X1_GCONV:
        # the implicit-GEMM kernel of CNN_ENCODER's trunk (three-piece bf16 operands: tgsr_gconv) takes a 1x1 filter as it is - the
        # weight [Cout, Cin] IS its A operand: emb_features on the 17 x 17 x 768 region features, forward and (through the
        # transposed weight, custom_ops._conv1x1_backward) data gradient, 80 -> ~20 us each at batch 16
        need = gconv_ws_elems(B, w2.shape[0], H, W, Cin)
        ws = torch.empty(need, dtype=torch.float32, device=x.device) if need else None
        gconv(False, w2, x, 0, Cin, out, 0, 1, 1, 1, 0, 0, None, False, False, ws, None)
        return out
    b = None if bias is None else _f32(bias.detach(), "bias").contiguous()
    check(_lib.lib().tgsr_conv1x1_fwd(_p(x), B, Cin, H * W, _p(w2), _p(b), w2.shape[0], _p(out), _stream()),
          "tgsr_conv1x1_fwd")
    return out


def conv1x1_wgrad(dy: torch.Tensor, x: torch.Tensor) -> Optional[torch.Tensor]:
    """Weight gradient of a bias-free 1x1 convolution, dW[co][ci] = sum over (b, pixel) of dy[b][co][p] x[b][ci][p], on the implicit-GEMM
    kernel: with K = B H W as the "channels" and Cin as the "pixels" it IS a 1x1 convolution - A = dy as [Cout, K], the image x as
    [1, K, Cin, 1] - split over K into slabs summed in a fixed order (emb_features in DAMSM pre-training, pretrain_DAMSM.py:79-98: the
    plain GEMM kernel took ~1 ms for these 1.8 GFLOP, half of the step's kernel time).  None when the shape does not qualify
    (K % 16 != 0, few channels): the caller keeps its own form."""
    _need_hip(dy, x)
    B, Cout, H, W = dy.shape
    Cin, K = x.shape[1], B * H * W
    if not CONV1X1_GCONV or K % 16 != 0 or K < 1024 or Cin < 64 or tuple(x.shape) != (B, Cin, H, W):
        return None
    a = _f32(dy, "dy").permute(1, 0, 2, 3).reshape(Cout, K).contiguous()
    xt = _f32(x, "x").permute(0, 2, 3, 1).reshape(1, K, Cin, 1).contiguous()
    out = torch.empty(1, Cout, Cin, 1, dtype=torch.float32, device=dy.device)
    need = gconv_ws_elems(1, Cout, Cin, 1, K)
    ws = torch.empty(need, dtype=torch.float32, device=dy.device) if need else None
    gconv(False, a, xt, 0, K, out, 0, 1, 1, 1, 0, 0, None, False, False, ws, None)
    return out.reshape(Cout, Cin)


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B,K] @ w[Cout,K]^T + bias (emb_cnn_code, util.py:301,364) as an MFMA GEMM."""
    _need_hip(x, w, bias)
    x = _f32(x, "x").contiguous()
    w2 = _f32(w.detach(), "w").contiguous()
    B, K = x.shape
    if w2.shape[1] != K:
        raise TgsrError("linear: weight %s vs input %s" % (tuple(w.shape), tuple(x.shape)))
    b = None if bias is None else _f32(bias.detach(), "bias").contiguous()
    if CONV1X1_GCONV and K % 16 == 0 and K >= 256:
        # long reductions over few rows (emb_cnn_code: 16 x 2048 -> 256; the recurrent weights' gradients: K = B T): on the plain
        # GEMM kernel a handful of workgroups walk K alone (~100 us for a few MFLOP); the implicit-GEMM kernel splits K over the
        # chip - x^T as a [1, K, B, 1] image, the weight as its A operand, the bias in its epilogue
        xt = x.t().contiguous().view(1, K, B, 1)
        img = torch.empty(1, w2.shape[0], B, 1, dtype=torch.float32, device=x.device)
        need = gconv_ws_elems(1, w2.shape[0], B, 1, K)
        ws = torch.empty(need, dtype=torch.float32, device=x.device) if need else None
        gconv(False, w2, xt, 0, K, img, 0, 1, 1, 1, 0, 0, b, False, False, ws, None)
        return img.view(w2.shape[0], B).t().contiguous()
    out = torch.empty(B, w2.shape[0], dtype=torch.float32, device=x.device)
    check(_lib.lib().tgsr_linear_fwd(_p(x), B, K, _p(w2), _p(b), w2.shape[0], _p(out), _stream()), "tgsr_linear_fwd")
    return out


# ----------------------------------------------------------------------------------------- training path primitives
def conv_to3_set_pipe(on: bool) -> bool:
    """The image heads' streaming kernel with its copies two stages ahead (default) or the plain double buffer; returns the previous setting."""
    return bool(_lib.lib().tgsr_conv_to3_set_pipe(1 if on else 0))


def conv_to3_pipe() -> bool:
    """The current setting of conv_to3_set_pipe (the library has only the exchange: set it and put it back)."""
    L = _lib.lib()
    was = L.tgsr_conv_to3_set_pipe(1)
    L.tgsr_conv_to3_set_pipe(was)
    return bool(was)


def wino4w_set_persist(cap: int) -> int:
    """How many workgroups a register-fed F(4x4) launch starts for its plan's tiles: -1 what the device holds at once (default), 0 one
    per tile, n > 0 at most n.  Bit-identical outputs either way; returns the previous value."""
    return int(_lib.lib().tgsr_wino4w_set_persist(int(cap)))


def bn_set_fuse_small(on: bool) -> bool:
    """Small BatchNorm layers (one workgroup per channel) as one launch per direction (default) or two; returns the previous setting."""
    return bool(_lib.lib().tgsr_bn_set_fuse_small(1 if on else 0))


def bn_train_fwd(raw: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, momentum: float,
                 running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], act: int = 0,
                 residual: Optional[torch.Tensor] = None, nbt: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                 stat_partial: Optional[torch.Tensor] = None):
    """nn.BatchNorm2d(train) on the raw conv output [B,C,H,W] + act (0 none [+ residual], 1 GLU, 2 LeakyReLU(0.2)):
    batch statistics, running statistics / num_batches_tracked updated in place through their pointers.  Returns
    (out, stats [4, C] = mean, invstd, scale, shift).  `out` / `stats` may be given (slices of larger tensors).
    `stat_partial` [C, nslots, 2]: the (sum, sumsq) pairs conv3x3_wino_stats left - the pass over `raw` that would compute
    them is then skipped."""
    _need_hip(raw, gamma, beta, running_mean, running_var, residual, nbt, out, stats, stat_partial)
    L = _lib.lib()
    B, C, Ho, Wo = raw.shape
    HW, dev = Ho * Wo, raw.device
    raw = _f32(raw, "raw")
    if not raw.is_contiguous():
        raise TgsrError("bn_train_fwd: raw must be contiguous")
    co = C // 2 if act == 1 else C
    if out is None:
        out = torch.empty(B, co, Ho, Wo, dtype=torch.float32, device=dev)
    if stats is None:
        stats = torch.empty(4, C, dtype=torch.float32, device=dev)
    res = None if residual is None else residual.contiguous()
    if stat_partial is not None:
        if (stat_partial.dim() != 3 or stat_partial.shape[0] != C or stat_partial.shape[2] != 2 or
                stat_partial.dtype != torch.float32 or not stat_partial.is_contiguous()):
            raise TgsrError("bn_train_fwd: stat_partial %s for %d channels" % (tuple(stat_partial.shape), C))
        s0, s1, s2, s3 = _rows4(stats)
        rc = L.tgsr_bn_train_fwd_from_stats(_p(raw), B, C, HW, _p(gamma), _p(beta), float(eps),
                                            float(momentum), _p(running_mean), _p(running_var), int(act), _p(res),
                                            0 if res is None else co * HW, _p(stat_partial), stat_partial.shape[1],
                                            s0, s1, s2, s3, _p(out), co * HW, _p(nbt), _stream())
        check(rc, "tgsr_bn_train_fwd_from_stats")
        return out, stats
    ws = torch.empty(C * L.tgsr_bn_train_nsplit(B, C, HW) * 4, dtype=torch.float32, device=dev)
    s0, s1, s2, s3 = _rows4(stats)
    rc = L.tgsr_bn_train_fwd(_p(raw), B, C, HW, _p(gamma), _p(beta), float(eps), float(momentum),
                             _p(running_mean), _p(running_var), int(act), _p(res), 0 if res is None else co * HW, _p(ws),
                             s0, s1, s2, s3, _p(out), co * HW, _p(nbt), _stream())
    check(rc, "tgsr_bn_train_fwd")
    return out, stats


def bn_train_bwd(dout: torch.Tensor, raw: torch.Tensor, stats: torch.Tensor, act: int, dgamma: Optional[torch.Tensor] = None,
                 dbeta: Optional[torch.Tensor] = None, draw: Optional[torch.Tensor] = None):
    """Backward of bn_train_fwd: (draw like raw, dgamma [C], dbeta [C]); the three may be given (gradient slots of a flat
    bucket, slices of a batched tensor)."""
    _need_hip(dout, raw, stats, dgamma, dbeta, draw)
    L = _lib.lib()
    B, C, Ho, Wo = raw.shape
    HW, dev = Ho * Wo, raw.device
    dout = _f32(dout, "dout").contiguous()
    co = C // 2 if act == 1 else C
    if draw is None:
        draw = torch.empty_like(raw)
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    ws = torch.empty(co * L.tgsr_bn_train_nsplit(B, co, HW) * 4, dtype=torch.float32, device=dev)
    s0, s1, s2, s3 = _rows4(stats)
    rc = L.tgsr_bn_train_bwd(_p(dout), _p(raw), B, C, HW, s2, s3, s0, s1, int(act),
                             _p(ws), _p(ws), _p(draw), _p(dgamma), _p(dbeta), _stream())
    check(rc, "tgsr_bn_train_bwd")
    return draw, dgamma, dbeta


def sumpool2x2(x: torch.Tensor) -> torch.Tensor:
    """Backward of nn.Upsample(x2, nearest): [B,C,2H,2W] -> [B,C,H,W], each output the sum of its 2x2 block."""
    _need_hip(x)
    x = _f32(x, "x").contiguous()
    B, C, H2, W2 = x.shape
    out = torch.empty(B, C, H2 // 2, W2 // 2, dtype=torch.float32, device=x.device)
    check(_lib.lib().tgsr_sumpool2x2(_p(x), B * C, H2 // 2, W2 // 2, _p(out), _stream()), "tgsr_sumpool2x2")
    return out


def conv3x3_wgrad_kind(Cin: int, Cout: int, upsample: bool, winograd: bool = True) -> str:
    """Which weight-gradient kernel serves a conv3x3 layer: "wino" (16 positions per 2x2 output tile) where Cout % 32 == 0 and
    Cin % 32 == 0; for an upBlock "upwino" (9 Winograd positions on the low-resolution pixels) where Cout % 64 == 0 and
    Cin % 32 == 0 - that kernel has 64-row co-blocks only (tgsr_upwino_wgrad.hip), so upBlock(32, 16) / GF_DIM = 16 (Cout = 32)
    stay on the direct kernel; else "direct"."""
    if winograd and Cin % 32 == 0:
        if upsample:
            return "upwino" if Cout % 64 == 0 else "direct"
        if Cout % 32 == 0:
            return "wino"
    return "direct"


# conv3x3_wgrad_kind -> (the launcher - its planner is <launcher>_ws_elems, 0 for what the launcher refuses; the profile row's name)
_WGRAD = {"direct": ("tgsr_conv3x3_wgrad", "conv3x3_wgrad_kernel"), "wino": ("tgsr_wino_wgrad", "wino_wgrad_kernel"),
          "upwino": ("tgsr_upwino_wgrad", "upwino_wgrad_kernel")}


def conv3x3_wgrad(draw: torch.Tensor, x: torch.Tensor, upsample: bool = False, winograd: bool = True,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient [Cout,Cin,3,3] of conv3x3(upsample ? nearest_x2(x) : x): draw [B,Cout,Ho,Wo] (gradient at the raw
    conv output), x [B,Cin,H,W]; per-workgroup partial slabs summed in a fixed order (reproducible).  `out`: where to
    write it (a gradient slot).  A shape the kernel refuses (an empty batch) raises TgsrError."""
    _need_hip(draw, x, out)
    L = _lib.lib()
    draw = _f32(draw, "draw").contiguous()
    x = _f32(x, "x").contiguous()
    B, Cin, H, W = x.shape
    Cout, HW, dev = draw.shape[1], draw.shape[2] * draw.shape[3], x.device
    dw = out if out is not None else torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=dev)
    kind = conv3x3_wgrad_kind(Cin, Cout, upsample, winograd)
    entry, name = _WGRAD[kind]
    up = (1 if upsample else 0,) if kind == "direct" else ()         # the one argument only tgsr_conv3x3_wgrad takes
    e0 = _ev() if profile is not None else None
    ws = torch.empty(getattr(L, entry + "_ws_elems")(B, Cin, Cout, H, W, *up), dtype=torch.float32, device=dev)
    check(getattr(L, entry)(_p(draw), _p(x), Cin * H * W, B, Cin, H, W, Cout, *up, _p(ws), _p(dw), _stream()), entry)
    if profile is not None:      # direct-form FLOPs of the weight gradient: one MAC per (output pixel, tap, ci, co)
        profile.append((name, 2.0 * B * HW * Cout * Cin * 9, 4.0 * (B * Cin * H * W + B * Cout * HW + Cout * Cin * 9), e0, _ev()))
    return dw


def conv_to3_bwd(dy: torch.Tensor, out: Optional[torch.Tensor], addend: Optional[torch.Tensor], alpha: float, x: torch.Tensor,
                 w: torch.Tensor, tanh_axpy: bool, need_dx: bool = True, need_dw: bool = True):
    """(dx, dw) of conv_to3 (None for a gradient that is not needed); `out` = the forward output (tanh heads)."""
    _need_hip(dy, out, addend, x, w)
    L = _lib.lib()
    dy, x, w = _f32(dy, "dy").contiguous(), _f32(x, "x").contiguous(), _f32(w.detach(), "w").contiguous()
    addend = None if addend is None else addend.contiguous()     # the kernel reads it as dense NCHW
    B, Cin, H, W = x.shape
    K = w.shape[2]
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w) if need_dw else None
    ws = x.new_empty(L.tgsr_conv_to3_bwd_ws_elems(B, Cin, H, W, K)) if need_dw else None
    rc = L.tgsr_conv_to3_bwd(_p(dy), _p(out), _p(addend), float(alpha), _p(x), Cin * H * W, _p(w), B, Cin, H, W, K,
                             _lib.ACT_TANH_AXPY if tanh_axpy else _lib.ACT_NONE, _p(dx), _p(ws), _p(dw), _stream())
    check(rc, "tgsr_conv_to3_bwd")
    return dx, dw


def word_attention_bwd(h: torch.Tensor, src: torch.Tensor, mask: Optional[torch.Tensor], correct_mask: bool, T: int,
                       dc: torch.Tensor):
    """Backward of word_attention wrt h and the projected words: h [B,idf,ih,iw], src [B,idf,32] (zero padded past T),
    dc [B,idf,ih,iw] -> (dh like h, dsrc [B,idf,T]); P is recomputed, the per-chunk partial sums of d(src) are added in a
    fixed order."""
    _need_hip(h, src, mask, dc)
    L = _lib.lib()
    h, dc = _f32(h, "h").contiguous(), _f32(dc, "dc").contiguous()
    B, idf, ih, iw = h.shape
    Q = ih * iw
    part = torch.empty(B, L.tgsr_word_attention_bwd_chunks(Q), idf, 32, dtype=torch.float32, device=h.device)
    dh = torch.empty_like(h)
    m8 = None if mask is None else _mask_u8(mask)
    rc = L.tgsr_word_attention_bwd(_p(h), idf * Q, _p(src.contiguous()), _p(m8), 1 if correct_mask else 0, B, idf, T, Q,
                                   _p(dc), _p(dh), _p(part), _stream())
    check(rc, "tgsr_word_attention_bwd")
    return dh, part.sum(1)[:, :, :T].contiguous()


def rowdot(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """out[b] = <x[b, :], w> + bias (the discriminators' logit heads: a 4x4 / stride-4 conv of a 4x4 map to one channel)."""
    _need_hip(x, w, bias)
    x = _f32(x, "x").contiguous()
    w = _f32(w.detach(), "w").contiguous().view(-1)
    B, K = x.shape
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    check(_lib.lib().tgsr_rowdot_fwd(_p(x), _p(w), _p(None if bias is None else bias.detach()), _p(out), B, K, _stream()),
          "tgsr_rowdot_fwd")
    return out


def rowdot_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, need_dx: bool = True, need_dw: bool = True):
    """(dx [B,K], dw [K]) of rowdot (None where not needed)."""
    _need_hip(dy, x, w)
    dy, x = _f32(dy, "dy").contiguous(), _f32(x, "x").contiguous()
    w = _f32(w.detach(), "w").contiguous().view(-1)
    B, K = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty(K, dtype=torch.float32, device=x.device) if need_dw else None
    if need_dx or need_dw:
        check(_lib.lib().tgsr_rowdot_bwd(_p(dy), _p(x), _p(w), _p(dx), _p(dw), B, K, _stream()), "tgsr_rowdot_bwd")
    return dx, dw


def ca_net(sent_emb: torch.Tensor, w: torch.Tensor, b: torch.Tensor, ncf: int, eps: Optional[torch.Tensor]):
    """CA_NET.forward (util.py:372-400) in one launch: (c_code or None, mu, logvar); eps [B,ncf] = the standard normals of
    the re-parametrisation (None: c_code is not produced - the x8 / x16 generators discard it, model.py:51-52)."""
    _need_hip(sent_emb, w, b, eps)
    x = _f32(sent_emb, "sent_emb").contiguous()
    w, b = _f32(w.detach(), "w").contiguous(), _f32(b.detach(), "b").contiguous()
    B, tdim = x.shape
    mu = torch.empty(B, ncf, dtype=torch.float32, device=x.device)
    logvar = torch.empty_like(mu)
    c_code = torch.empty_like(mu) if eps is not None else None
    check(_lib.lib().tgsr_ca_net_fwd(_p(x), _p(w), _p(b), _p(eps), B, tdim, ncf, _p(c_code), _p(mu), _p(logvar), _stream()),
          "tgsr_ca_net_fwd")
    return c_code, mu, logvar


def text_tail(words: torch.Tensor, w_ctxs, sent_emb: torch.Tensor, ca_w: torch.Tensor, ca_b: torch.Tensor, ncf: int,
              captions: torch.Tensor, lp_dtype=None):
    """What an inference step needs between the text encoder and the generator, in one launch (tgsr_text_tail_fwd):
    word_project(words, w_ctxs), CA_NET's (mu, logvar) and mask = (captions[:, :T] == 0).
    Returns (src [nsets,B,idf,32], mu, logvar, mask uint8 [B,T] - `.view(torch.bool)` is the reference's mask).
    lp_dtype (torch.bfloat16 | torch.float16; idf == 32): a fifth value, the uint8 buffer `att_pack` of
    tgsr_text_tail_lp_fwd - the projections as MFMA A fragments of that type + the packed mask rows, which the
    reduced-precision kernels that attend in their epilogue read (lp.stem / lp.upconv_glu_head with att=...)."""
    import ctypes
    _need_hip(words, sent_emb, ca_w, ca_b, captions, *w_ctxs)
    words = _f32(words, "words").contiguous()
    B, cdf, T = words.shape
    n = len(w_ctxs)
    idf = w_ctxs[0].shape[0]
    ws = [_f32(w.detach(), "w_ctx").reshape(idf, cdf).contiguous() for w in w_ctxs]
    x = _f32(sent_emb, "sent_emb").contiguous()
    w, b = _f32(ca_w.detach(), "ca_w").contiguous(), _f32(ca_b.detach(), "ca_b").contiguous()
    if captions.dtype != torch.int64 or captions.dim() != 2 or captions.shape[0] != B or captions.shape[1] < T:
        raise TgsrError("text_tail: captions %s %s for words %s" % (tuple(captions.shape), captions.dtype, tuple(words.shape)))
    captions = captions.contiguous()
    if x.shape[0] != B or w.shape != (4 * ncf, x.shape[1]):
        raise TgsrError("text_tail: sent_emb %s / fc weight %s" % (tuple(x.shape), tuple(w.shape)))
    out = torch.empty(n, B, idf, 32, dtype=torch.float32, device=words.device)
    mu = torch.empty(B, ncf, dtype=torch.float32, device=words.device)
    logvar = torch.empty_like(mu)
    mask = torch.empty(B, T, dtype=torch.uint8, device=words.device)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ws])
    if lp_dtype is not None:
        L = _lib.lib()
        dt = {torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}[lp_dtype]
        pack = torch.empty(L.tgsr_lp_att_pack_bytes(n, B), dtype=torch.uint8, device=words.device)
        check(L.tgsr_text_tail_lp_fwd(_p(words), ptrs, n, B, idf, cdf, T, _p(out), _p(x), _p(w), _p(b), x.shape[1], ncf,
                                      _p(mu), _p(logvar), _p(captions), captions.shape[1], _p(mask), dt, _p(pack), _stream()),
              "tgsr_text_tail_lp_fwd")
        return out, mu, logvar, mask, pack
    check(_lib.lib().tgsr_text_tail_fwd(_p(words), ptrs, n, B, idf, cdf, T, _p(out), _p(x), _p(w), _p(b), x.shape[1], ncf,
                                        _p(mu), _p(logvar), _p(captions), captions.shape[1], _p(mask), _stream()),
          "tgsr_text_tail_fwd")
    return out, mu, logvar, mask


def multi_copy(dsts, srcs) -> None:
    """dst[i].copy_(src[i]) for up to 16 dense same-shape, same-dtype device tensors in one launch (tgsr_multi_copy)."""
    import ctypes
    n = len(dsts)
    if n == 0:
        return
    if n != len(srcs) or n > 16:
        raise TgsrError("multi_copy: %d destinations, %d sources" % (n, len(srcs)))
    _need_hip(*dsts, *srcs)
    for d, s_ in zip(dsts, srcs):
        if d.shape != s_.shape or d.dtype != s_.dtype or not d.is_contiguous() or not s_.is_contiguous():
            raise TgsrError("multi_copy: %s %s <- %s %s" % (tuple(d.shape), d.dtype, tuple(s_.shape), s_.dtype))
    dp = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts])
    sp = (ctypes.c_void_p * n)(*[s_.data_ptr() for s_ in srcs])
    nb = (ctypes.c_int64 * n)(*[d.numel() * d.element_size() for d in dsts])
    check(_lib.lib().tgsr_multi_copy(n, dp, sp, nb, _stream()), "tgsr_multi_copy")


# ----------------------------------------------------------------------------------------- RCCL behind the C ABI
def comm_available() -> bool:
    """librccl could be opened by the library (tgsr_comm_available)."""
    return bool(_lib.lib().tgsr_comm_available())


def comm_unique_id() -> bytes:
    """The 128-byte id rank 0 creates and every rank passes to comm_init (ncclGetUniqueId)."""
    import ctypes
    buf = ctypes.create_string_buffer(128)
    check(_lib.lib().tgsr_comm_unique_id(buf), "tgsr_comm_unique_id")
    return bytes(buf.raw)


def comm_init(unique_id: bytes, rank: int, world: int) -> int:
    """An RCCL communicator on the current device (ncclCommInitRank; collective over the ranks); returns an opaque handle."""
    import ctypes
    if len(unique_id) != 128:
        raise TgsrError("comm_init: the unique id has %d bytes, not 128" % len(unique_id))
    comm = ctypes.c_void_p()
    check(_lib.lib().tgsr_comm_init(ctypes.byref(comm), ctypes.create_string_buffer(unique_id, 128), int(rank), int(world)),
          "tgsr_comm_init")
    return comm.value


def allreduce_flat(comm: int, flat: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """flat <- scale * sum over ranks of flat, in place, on torch's current stream (tgsr_allreduce_flat: ncclAllReduce + one
    scaling launch): the gradient bucket's collective without torch.distributed in the way."""
    _need_hip(flat)
    if flat.dtype != torch.float32 or not flat.is_contiguous():
        raise TgsrError("allreduce_flat: a dense fp32 buffer, got %s %s" % (flat.dtype, tuple(flat.shape)))
    check(_lib.lib().tgsr_allreduce_flat(comm, _p(flat), flat.numel(), float(scale), _stream()), "tgsr_allreduce_flat")
    return flat


def comm_count(comm: int) -> tuple:
    """(world, rank) as RCCL reports them for a communicator (ncclCommCount, ncclCommUserRank)."""
    import ctypes
    w, r = ctypes.c_int(-1), ctypes.c_int(-1)
    check(_lib.lib().tgsr_comm_count(comm, ctypes.byref(w), ctypes.byref(r)), "tgsr_comm_count")
    return int(w.value), int(r.value)


def comm_destroy(comm: int) -> None:
    check(_lib.lib().tgsr_comm_destroy(comm), "tgsr_comm_destroy")


def axpy_images(ts, ss, alpha: float, outs=None):
    """[t + alpha * s for t, s in zip(ts, ss)] for up to 4 dense fp32 images in one launch (tgsr_axpy_images): the closing
    `+ a * SRb` of NetG_highweight's heads when tanh(conv5x5(.)) was computed ahead of the low-frequency images."""
    import ctypes
    n = len(ts)
    if n == 0:
        return []
    if n != len(ss) or n > 4:
        raise TgsrError("axpy_images: %d / %d images (at most 4)" % (n, len(ss)))
    _need_hip(*ts, *ss)
    ts = [_f32(t, "t").contiguous() for t in ts]
    ss = [_f32(s_, "s").contiguous() for s_ in ss]
    for t, s_ in zip(ts, ss):
        if t.shape != s_.shape:
            raise TgsrError("axpy_images: %s + alpha * %s" % (tuple(t.shape), tuple(s_.shape)))
    if outs is None:
        outs = [torch.empty_like(t) for t in ts]
    tp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    sp = (ctypes.c_void_p * n)(*[s_.data_ptr() for s_ in ss])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    ne = (ctypes.c_int64 * n)(*[t.numel() for t in ts])
    check(_lib.lib().tgsr_axpy_images(n, op, tp, sp, ne, float(alpha), _stream()), "tgsr_axpy_images")
    return outs



def adam_flat(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, state: torch.Tensor,
              lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, advance: bool) -> None:
    """One Adam update over flat buffers, in place (tgsr_adam_flat): `state` = 3 device floats [step, 1 - b1^t, sqrt(1 - b2^t)],
    advanced on the device first when `advance`."""
    _need_hip(param, grad, exp_avg, exp_avg_sq, state)
    n = param.numel()
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise TgsrError("adam_flat: dense fp32 buffers of one length expected")
    if state.dtype != torch.float32 or state.numel() != 3 or not state.is_contiguous():
        raise TgsrError("adam_flat: state = 3 fp32 values")
    check(_lib.lib().tgsr_adam_flat(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(state), n, float(lr), float(beta1),
                                    float(beta2), float(eps), float(weight_decay), 1 if advance else 0, _stream()), "tgsr_adam_flat")

def weighted_bce(a: torch.Tensor, b: Optional[torch.Tensor], target: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """sum_i weight[i] * BCEWithLogits([a; b][i], target[i]) as a 0-dim tensor (the adversarial terms of the GAN losses)."""
    _need_hip(a, b, target, weight)
    a = _f32(a, "a").contiguous().view(-1)
    b = None if b is None else _f32(b, "b").contiguous().view(-1)
    n = a.numel() + (0 if b is None else b.numel())
    if target.numel() != n or weight.numel() != n or target.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TgsrError("weighted_bce: %d logits, %d targets, %d weights" % (n, target.numel(), weight.numel()))
    out = torch.empty((), dtype=torch.float32, device=a.device)
    check(_lib.lib().tgsr_weighted_bce_fwd(_p(a), a.numel(), _p(b), 0 if b is None else b.numel(), _p(target.contiguous()),
                                           _p(weight.contiguous()), _p(out), _stream()), "tgsr_weighted_bce_fwd")
    return out


def weighted_bce_bwd(dy: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor], target: torch.Tensor, weight: torch.Tensor):
    """(da, db) of weighted_bce."""
    _need_hip(dy, a, b, target, weight)
    dy = _f32(dy, "dy").contiguous()
    af = a.contiguous().view(-1)
    bf = None if b is None else b.contiguous().view(-1)
    da = torch.empty_like(a, memory_format=torch.contiguous_format)
    db = None if b is None else torch.empty_like(b, memory_format=torch.contiguous_format)
    check(_lib.lib().tgsr_weighted_bce_bwd(_p(dy), _p(af), af.numel(), _p(bf), 0 if bf is None else bf.numel(),
                                           _p(target.contiguous()), _p(weight.contiguous()), _p(da), _p(db), _stream()),
          "tgsr_weighted_bce_bwd")
    return da, db


def axpy_map(t: torch.Tensor, s: torch.Tensor, amap: torch.Tensor) -> torch.Tensor:
    """t + amap * s with amap [H, W] broadcast over batch and channels (NetG_highweight(weightmap=True), model.py:276-297)."""
    _need_hip(t, s, amap)
    t, s, amap = _f32(t, "t").contiguous(), _f32(s, "s").contiguous(), _f32(amap.detach(), "amap").contiguous()
    if t.shape != s.shape or t.dim() != 4 or tuple(amap.shape) != tuple(t.shape[2:]):
        raise TgsrError("axpy_map: %s + %s * %s" % (tuple(t.shape), tuple(amap.shape), tuple(s.shape)))
    out = torch.empty_like(t)
    check(_lib.lib().tgsr_axpy_map_fwd(_p(t), _p(s), _p(amap), _p(out), t.shape[0] * t.shape[1], t.shape[2] * t.shape[3], _stream()),
          "tgsr_axpy_map_fwd")
    return out


def axpy_map_bwd(dy: torch.Tensor, s: torch.Tensor, amap: torch.Tensor, need_ds: bool = True, need_da: bool = True):
    """(ds, damap) of axpy_map: ds = amap * dy, damap = sum over batch and channels of dy * s."""
    _need_hip(dy, s, amap)
    dy, s, amap = _f32(dy, "dy").contiguous(), _f32(s, "s").contiguous(), _f32(amap.detach(), "amap").contiguous()
    ds = torch.empty_like(dy) if need_ds else None
    da = torch.empty_like(amap) if need_da else None
    if ds is None and da is None:
        return None, None
    check(_lib.lib().tgsr_axpy_map_bwd(_p(dy), _p(s), _p(amap), _p(ds), _p(da), dy.shape[0] * dy.shape[1], dy.shape[2] * dy.shape[3],
                                       _stream()), "tgsr_axpy_map_bwd")
    return ds, da


def affine_act(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, act: int) -> torch.Tensor:
    """act(raw * scale[c] + shift[c]) on a dense NCHW tensor (eval-mode BatchNorm + LeakyReLU(0.2) for act = 2)."""
    _need_hip(raw, scale, shift)
    raw = _f32(raw, "raw").contiguous()
    B, Cc, H, W = raw.shape
    out = torch.empty_like(raw)
    check(_lib.lib().tgsr_affine_act_fwd(_p(raw), _p(scale.contiguous()), _p(shift.contiguous()), _p(out), B, Cc, H * W, int(act),
                                         _stream()), "tgsr_affine_act_fwd")
    return out


def affine_act_bwd(dy: torch.Tensor, out: Optional[torch.Tensor], scale: torch.Tensor, act: int) -> torch.Tensor:
    _need_hip(dy, out, scale)
    dy = _f32(dy, "dy").contiguous()
    B, Cc, H, W = dy.shape
    draw = torch.empty_like(dy)
    check(_lib.lib().tgsr_affine_act_bwd(_p(dy), _p(None if out is None else out.contiguous()), _p(scale.contiguous()), _p(draw),
                                         B, Cc, H * W, int(act), _stream()), "tgsr_affine_act_bwd")
    return draw


# ----------------------------------------------------------------------------------------- CNN_ENCODER's frozen trunk (tgsr_igemm.hip)
def _slice_ptr(t: torch.Tensor, coff: int):
    """Pointer to channel `coff` of a dense NCHW tensor and its batch stride in elements."""
    if t.dim() != 4 or not t.is_contiguous() or t.dtype != torch.float32:
        raise TgsrError("dense fp32 NCHW tensor expected, got %s %s" % (t.dtype, tuple(t.shape)))
    return t.data_ptr() + 4 * coff * t.shape[2] * t.shape[3], t.shape[1] * t.shape[2] * t.shape[3]


def gconv_pack(w: torch.Tensor, scale: Optional[torch.Tensor], dgrad: bool) -> torch.Tensor:
    """The filter [Cout, Cin, KH, KW] times the folded BatchNorm scale, as the A operand of gconv: forward [Cout, Cin KH KW] or data
    gradient [Cin, Cout KH KW]."""
    _need_hip(w, scale)
    w = _f32(w.detach(), "w").contiguous()
    Cout, Cin, KH, KW = w.shape
    out = torch.empty((Cin, Cout * KH * KW) if dgrad else (Cout, Cin * KH * KW), dtype=torch.float32, device=w.device)
    check(_lib.lib().tgsr_gconv_pack(_p(w), _p(scale), _p(out), Cout, Cin, KH * KW, 1 if dgrad else 0, _stream()), "tgsr_gconv_pack")
    return out


def gconv_set_form(split: bool) -> bool:
    """The arithmetic form of gconv: True (default) = three-piece bf16 operands on the bf16 matrix pipe where the shape qualifies,
    False = fp32 MFMA everywhere.  Returns the previous setting."""
    return bool(_lib.lib().tgsr_gconv_set_form(1 if split else 0))


def gconv_ws_elems(B: int, M: int, PH: int, PW: int, K: int) -> int:
    return int(_lib.lib().tgsr_gconv_ws_elems(B, M, PH, PW, K))


def _gconv_check(name, dgrad, A, S, s_coff, s_ch, out, o_coff, kh, kw, stride, padh, padw, ws):
    """The shape and workspace checks gconv and gconv_stats share; returns (B, Hs, Ws, M, K, PH, PW)."""
    M, K = A.shape
    B, Hs, Ws = S.shape[0], S.shape[2], S.shape[3]
    PH, PW = out.shape[2], out.shape[3]
    if K != s_ch * kh * kw or s_coff + s_ch > S.shape[1] or o_coff + M > out.shape[1] or out.shape[0] != B:
        raise TgsrError("%s: A %s against %d channels of %s -> channels %d.. of %s" % (name, tuple(A.shape), s_ch, tuple(S.shape), o_coff,
                                                                                       tuple(out.shape)))
    (h_in, w_in), (h_out, w_out) = ((PH, PW), (Hs, Ws)) if dgrad else ((Hs, Ws), (PH, PW))
    if h_out != (h_in + 2 * padh - kh) // stride + 1 or w_out != (w_in + 2 * padw - kw) // stride + 1:
        raise TgsrError("%s: %dx%d / stride %d / pad (%d, %d) does not map %s to %s" % (name, kh, kw, stride, padh, padw, tuple(S.shape),
                                                                                       tuple(out.shape)))
    need = gconv_ws_elems(B, M, PH, PW, K)
    if need and (ws is None or ws.numel() < need):
        raise TgsrError("%s: %d floats of workspace needed" % (name, need))
    return B, Hs, Ws, M, K, PH, PW


def gconv(dgrad: bool, A: torch.Tensor, S: torch.Tensor, s_coff: int, s_ch: int, out: torch.Tensor, o_coff: int, kh: int, kw: int,
          stride: int, padh: int, padw: int, bias: Optional[torch.Tensor], relu: bool, accumulate: bool, ws: Optional[torch.Tensor],
          mask: Optional[torch.Tensor] = None):
    """Convolution (dgrad False) or its data gradient (True) as one implicit GEMM: reads channels [s_coff, s_coff + s_ch) of S,
    writes channels [o_coff, o_coff + A.shape[0]) of out (+= when accumulate).  mask (shaped like out): the contribution is kept
    where mask > 0 (the ReLU of the tensor whose gradient `out` is)."""
    _need_hip(A, S, out, bias, ws, mask)
    if mask is not None and (mask.shape != out.shape or not mask.is_contiguous() or mask.dtype != torch.float32):
        raise TgsrError("gconv: the mask must be a dense fp32 tensor shaped like the output")
    B, Hs, Ws, M, K, PH, PW = _gconv_check("gconv", dgrad, A, S, s_coff, s_ch, out, o_coff, kh, kw, stride, padh, padw, ws)
    sp, sbs = _slice_ptr(S, s_coff)
    op, obs = _slice_ptr(out, o_coff)
    mp = None if mask is None else _slice_ptr(mask, o_coff)[0]
    check(_lib.lib().tgsr_gconv(1 if dgrad else 0, _p(A.contiguous()), sp, sbs, B, Hs, Ws, M, K, PH, PW, kh, kw, stride, padh, padw,
                                _p(bias), 1 if relu else 0, 1 if accumulate else 0, mp, op, obs, _p(ws), _stream()), "tgsr_gconv")


def gconv_stats_nslots(B: int, M: int, PH: int, PW: int, K: int) -> int:
    """Statistics slots per channel gconv_stats writes for this forward shape (stat_partial is [M, nslots, 2])."""
    return int(_lib.lib().tgsr_gconv_stats_nslots(B, M, PH, PW, K))


def gconv_stats_slot_pixels(B: int, M: int, PH: int, PW: int, K: int) -> int:
    """Pixels per statistics slot of gconv_stats for this forward shape (the last slot holds the remainder)."""
    return int(_lib.lib().tgsr_gconv_stats_slot_pixels(B, M, PH, PW, K))


def gconv_stats(A: torch.Tensor, S: torch.Tensor, s_coff: int, s_ch: int, out: torch.Tensor, o_coff: int, kh: int, kw: int,
                stride: int, padh: int, padw: int, ws: Optional[torch.Tensor], stat_partial: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw forward convolution (gconv without bias / ReLU, the same bits) into channels [o_coff, o_coff + A.shape[0]) of out, and
    its BatchNorm batch statistics: per output channel and slot of gconv_stats_slot_pixels pixels the pair (sum, sum of squared
    deviations from the slot's mean), stat_partial [M, nslots, 2] (allocated when None).  Returns stat_partial."""
    _need_hip(A, S, out, ws, stat_partial)
    B, Hs, Ws, M, K, PH, PW = _gconv_check("gconv_stats", False, A, S, s_coff, s_ch, out, o_coff, kh, kw, stride, padh, padw, ws)
    ns = gconv_stats_nslots(B, M, PH, PW, K)
    if stat_partial is None:
        stat_partial = torch.empty(M, ns, 2, dtype=torch.float32, device=out.device)
    elif tuple(stat_partial.shape) != (M, ns, 2) or stat_partial.dtype != torch.float32 or not stat_partial.is_contiguous():
        raise TgsrError("gconv_stats: stat_partial %s, expected (%d, %d, 2) fp32" % (tuple(stat_partial.shape), M, ns))
    sp, sbs = _slice_ptr(S, s_coff)
    op, obs = _slice_ptr(out, o_coff)
    check(_lib.lib().tgsr_gconv_stats(_p(A.contiguous()), sp, sbs, B, Hs, Ws, M, K, PH, PW, kh, kw, stride, padh, padw, op, obs, _p(ws),
                                      _p(stat_partial), _stream()), "tgsr_gconv_stats")
    return stat_partial


def bn_train_relu_slice_from_stats(y: torch.Tensor, coff: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, momentum: float,
                                   running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor],
                                   nbt: Optional[torch.Tensor], stat_partial: torch.Tensor, slot_px: int,
                                   stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place over channels [coff, coff + C) of y (C = stat_partial.shape[0], the raw convolution gconv_stats wrote there, slots
    of slot_px pixels): y = relu(batch_norm(y, training=True)), the batch statistics combined from stat_partial; running_mean /
    running_var (momentum,
    unbiased variance) and nbt (num_batches_tracked, += 1) updated in place.  Returns stats [4, C] = mean, invstd, scale, shift."""
    _need_hip(y, gamma, beta, running_mean, running_var, nbt, stat_partial, stats)
    if stat_partial.dim() != 3 or stat_partial.shape[2] != 2 or stat_partial.dtype != torch.float32 or not stat_partial.is_contiguous():
        raise TgsrError("bn_train_relu_slice_from_stats: stat_partial %s" % (tuple(stat_partial.shape),))
    C = stat_partial.shape[0]
    if coff < 0 or coff + C > y.shape[1] or gamma.numel() != C or beta.numel() != C:
        raise TgsrError("bn_train_relu_slice_from_stats: %d channels at %d of %s" % (C, coff, tuple(y.shape)))
    for t in (running_mean, running_var):
        if t is not None and (t.numel() != C or t.dtype != torch.float32 or not t.is_contiguous()):
            raise TgsrError("bn_train_relu_slice_from_stats: running statistics of %d fp32 channels expected" % C)
    if nbt is not None and nbt.dtype != torch.int64:
        raise TgsrError("bn_train_relu_slice_from_stats: num_batches_tracked must be int64")
    if stats is None:
        stats = torch.empty(4, C, dtype=torch.float32, device=y.device)
    elif tuple(stats.shape) != (4, C) or not stats.is_contiguous() or stats.dtype != torch.float32:
        raise TgsrError("bn_train_relu_slice_from_stats: stats must be a dense fp32 [4, %d]" % C)
    yp, ybs = _slice_ptr(y, coff)
    check(_lib.lib().tgsr_bn_train_relu_slice_from_stats(yp, ybs, y.shape[0], C, y.shape[2] * y.shape[3], _p(_f32(gamma, "gamma").contiguous()),
                                                         _p(_f32(beta, "beta").contiguous()), float(eps), float(momentum),
                                                         _p(running_mean), _p(running_var), _p(stat_partial), stat_partial.shape[1],
                                                         int(slot_px), _p(stats), _p(nbt), _stream()),
          "tgsr_bn_train_relu_slice_from_stats")
    return stats


def sum_stack(stack: torch.Tensor, n: int, out: torch.Tensor):
    """out = ((stack[0] + stack[1]) + ...) + stack[n - 1]: the first n slices of a dense stack [N, ...] summed in order (tgsr_sum_stack)."""
    _need_hip(stack, out)
    if stack.dtype != torch.float32 or not stack.is_contiguous() or not out.is_contiguous() or out.dtype != torch.float32:
        raise TgsrError("sum_stack: dense fp32 tensors expected")
    if n < 1 or n > stack.shape[0] or tuple(stack.shape[1:]) != tuple(out.shape):
        raise TgsrError("sum_stack: %d slices of %s into %s" % (n, tuple(stack.shape), tuple(out.shape)))
    check(_lib.lib().tgsr_sum_stack(_p(stack), n, out.numel(), _p(out), _stream()), "tgsr_sum_stack")

def interleave2x2(parts, dx: torch.Tensor, accumulate: bool, mask: Optional[torch.Tensor] = None):
    """dx[:, :, py::2, px::2] (+)= parts[2 py + px] (dense [B, C, ceil((H - py) / 2), ceil((W - px) / 2)]), masked where mask <= 0:
    the four parity classes of a stride-2 convolution's data gradient woven into one tensor (tgsr_interleave2x2)."""
    _need_hip(dx, mask, *parts)
    B, Cc, H, W = dx.shape
    if not dx.is_contiguous() or dx.dtype != torch.float32 or len(parts) != 4:
        raise TgsrError("interleave2x2: a dense fp32 dx and four class tensors expected")
    for k, t in enumerate(parts):
        want = (B, Cc, (H - (k >> 1) + 1) // 2, (W - (k & 1) + 1) // 2)
        if tuple(t.shape) != want or not t.is_contiguous() or t.dtype != torch.float32:
            raise TgsrError("interleave2x2: class %d is %s, expected dense %s" % (k, tuple(t.shape), want))
    if mask is not None and (mask.shape != dx.shape or not mask.is_contiguous() or mask.dtype != torch.float32):
        raise TgsrError("interleave2x2: the mask must be a dense fp32 tensor shaped like dx")
    check(_lib.lib().tgsr_interleave2x2(_p(parts[0]), _p(parts[1]), _p(parts[2]), _p(parts[3]), _p(dx), B * Cc, H, W,
                                        1 if accumulate else 0, _p(mask), _stream()), "tgsr_interleave2x2")

def maxpool3s2(x: torch.Tensor, out: torch.Tensor, o_coff: int):
    _need_hip(x, out)
    B, Cc, H, W = x.shape
    xp, xbs = _slice_ptr(x, 0)
    op, obs = _slice_ptr(out, o_coff)
    if out.shape[2] != (H - 3) // 2 + 1 or out.shape[3] != (W - 3) // 2 + 1 or o_coff + Cc > out.shape[1]:
        raise TgsrError("maxpool3s2: %s -> %s" % (tuple(x.shape), tuple(out.shape)))
    check(_lib.lib().tgsr_maxpool3s2_fwd(xp, xbs, B, Cc, H, W, op, obs, _stream()), "tgsr_maxpool3s2_fwd")


def maxpool3s2_bwd(x: torch.Tensor, dy: torch.Tensor, dy_coff: int, dx: torch.Tensor, accumulate: bool, mask: Optional[torch.Tensor] = None):
    _need_hip(x, dy, dx, mask)
    if mask is not None and (mask.shape != dx.shape or not mask.is_contiguous()):
        raise TgsrError("maxpool3s2_bwd: the mask must be dense and shaped like dx")
    B, Cc, H, W = x.shape
    xp, xbs = _slice_ptr(x, 0)
    gp, gbs = _slice_ptr(dy, dy_coff)
    dp, dbs = _slice_ptr(dx, 0)
    if dx.shape != x.shape or dy_coff + Cc > dy.shape[1]:
        raise TgsrError("maxpool3s2_bwd: shapes")
    check(_lib.lib().tgsr_maxpool3s2_bwd(xp, xbs, gp, gbs, B, Cc, H, W, dp, dbs, 1 if accumulate else 0, _p(mask), _stream()),
          "tgsr_maxpool3s2_bwd")


def avgpool3(x: torch.Tensor, out: torch.Tensor, accumulate: bool, mask: Optional[torch.Tensor] = None):
    _need_hip(x, out, mask)
    if mask is not None and (mask.shape != out.shape or not mask.is_contiguous()):
        raise TgsrError("avgpool3: the mask must be dense and shaped like the output")
    if x.shape != out.shape:
        raise TgsrError("avgpool3: %s -> %s" % (tuple(x.shape), tuple(out.shape)))
    B, Cc, H, W = x.shape
    xp, xbs = _slice_ptr(x, 0)
    op, obs = _slice_ptr(out, 0)
    check(_lib.lib().tgsr_avgpool3(xp, xbs, B, Cc, H, W, op, obs, 1 if accumulate else 0, _p(mask), _stream()), "tgsr_avgpool3")


def plane_mean(x: torch.Tensor) -> torch.Tensor:
    _need_hip(x)
    x = _f32(x, "x").contiguous()
    B, Cc, H, W = x.shape
    out = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
    check(_lib.lib().tgsr_plane_mean(_p(x), _p(out), B * Cc, H * W, _stream()), "tgsr_plane_mean")
    return out


def plane_mean_bwd(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    _need_hip(dy)
    dy = _f32(dy, "dy").contiguous()
    B, Cc = dy.shape
    dx = torch.empty(B, Cc, H, W, dtype=torch.float32, device=dy.device)
    check(_lib.lib().tgsr_plane_mean_bwd(_p(dy), _p(dx), B * Cc, H * W, _stream()), "tgsr_plane_mean_bwd")
    return dx


def relu_mask_(dy: torch.Tensor, y: torch.Tensor, coff: int, ch: int):
    """dy[:, coff:coff+ch] *= (y[:, coff:coff+ch] > 0) in place (two equally shaped dense NCHW tensors)."""
    _need_hip(dy, y)
    if dy.shape != y.shape or coff + ch > dy.shape[1]:
        raise TgsrError("relu_mask: %s / %s" % (tuple(dy.shape), tuple(y.shape)))
    gp, gbs = _slice_ptr(dy, coff)
    yp, ybs = _slice_ptr(y, coff)
    check(_lib.lib().tgsr_relu_mask(gp, gbs, yp, ybs, gp, gbs, dy.shape[0], ch * dy.shape[2] * dy.shape[3], _stream()), "tgsr_relu_mask")


def bilinear(x: torch.Tensor, OH: int, OW: int) -> torch.Tensor:
    _need_hip(x)
    x = _f32(x, "x").contiguous()
    B, Cc, H, W = x.shape
    out = torch.empty(B, Cc, OH, OW, dtype=torch.float32, device=x.device)
    check(_lib.lib().tgsr_bilinear_fwd(_p(x), B * Cc, H, W, OH, OW, _p(out), _stream()), "tgsr_bilinear_fwd")
    return out


def bilinear_bwd(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    _need_hip(dy)
    dy = _f32(dy, "dy").contiguous()
    B, Cc, OH, OW = dy.shape
    dx = torch.empty(B, Cc, H, W, dtype=torch.float32, device=dy.device)
    check(_lib.lib().tgsr_bilinear_bwd(_p(dy), B * Cc, H, W, OH, OW, _p(dx), _stream()), "tgsr_bilinear_bwd")
    return dx


# ----------------------------------------------------------------------------------------- image pyramid (uint8)
def _u8_images(x: torch.Tensor, what: str, min_dim: int = 2) -> torch.Tensor:
    """The image operand of the pyramid wrappers: uint8 (any other type would be read as bytes), at least `min_dim` dimensions,
    not empty, on the HIP device; returned dense."""
    if x.dtype != torch.uint8:
        raise TgsrError("%s: uint8 images expected, got %s" % (what, x.dtype))
    if x.dim() < min_dim:
        raise TgsrError("%s: at least %d dimension%s expected, got shape %s" % (what, min_dim, "s" if min_dim > 1 else "", tuple(x.shape)))
    if x.numel() < 1:
        raise TgsrError("%s: an empty tensor, shape %s" % (what, tuple(x.shape)))
    _need_hip(x)
    return x.contiguous()


def resize_bilinear_u8(x: torch.Tensor, out_h: int, out_w: int, htab, vtab) -> torch.Tensor:
    """Pillow's `resize(BILINEAR)` of planar uint8 images [..., H, W]; htab / vtab = (bounds, coefficients, ksize) device
    tables of the horizontal / vertical pass, or None when that size does not change."""
    if out_h < 1 or out_w < 1:
        raise TgsrError("resize: the output size must be at least 1 x 1, got %d x %d" % (out_h, out_w))
    x = _u8_images(x, "resize")
    H, W = x.shape[-2], x.shape[-1]
    N = x.numel() // (H * W)
    out = torch.empty(x.shape[:-2] + (out_h, out_w), dtype=torch.uint8, device=x.device)
    hb, hk, hks = htab if htab is not None else (None, None, 0)
    vb, vk, vks = vtab if vtab is not None else (None, None, 0)
    tmp = torch.empty(N * H * out_w, dtype=torch.uint8, device=x.device) if (hb is not None and vb is not None) else None
    check(_lib.lib().tgsr_resize_bilinear_u8(_p(x), N, H, W, out_h, out_w, _p(hb), _p(hk), hks, _p(vb), _p(vk), vks, _p(tmp),
                                             _p(out), _stream()), "tgsr_resize_bilinear_u8")
    return out


def gaussian_blur_u8(x: torch.Tensor, r: int, ww: int, fw: int, passes: int = 3) -> torch.Tensor:
    """Pillow's GaussianBlur (extended box blur, `passes` per axis) of planar uint8 images [..., H, W]."""
    if passes < 1:
        raise TgsrError("gaussian_blur: passes must be at least 1, got %d" % passes)
    x = _u8_images(x, "gaussian_blur")
    H, W = x.shape[-2], x.shape[-1]
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    check(_lib.lib().tgsr_gaussian_blur_u8(_p(x), x.numel() // (H * W), H, W, r, ww, fw, passes, _p(tmp), _p(out), _stream()),
          "tgsr_gaussian_blur_u8")
    return out


def u8_normalize(x: torch.Tensor) -> torch.Tensor:
    """ToTensor + Normalize((0.5,)*3, (0.5,)*3) (datasets.py:286-288): uint8 -> float32 in [-1, 1]."""
    x = _u8_images(x, "u8_normalize", 1)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(_lib.lib().tgsr_u8_normalize(_p(x), _p(out), x.numel(), _stream()), "tgsr_u8_normalize")
    return out


# ----------------------------------------------------------------------------------------- crop / resize / window / flip
AUG_DESC = 12            # int32 per image: byte offset, H, W, x1, y1, x2, y2, oh, ow, top, left, flip
AUG_MAX_SIDE = 4096      # source H, W
AUG_MAX_OUT = 65536      # resized oh, ow
AUG_MAX_RATIO = 16       # reduction per axis (Pillow's tap count 33)


def resize_ksize(in_size: int, out_size: int) -> int:
    """Pillow's tap-table width for a bilinear resample of in_size -> out_size: 2 ceil(max(in / out, 1)) + 1."""
    support = max(in_size / out_size, 1.0)
    c = int(support)
    return 2 * (c + (c < support)) + 1


def check_augment_table(table, S: int, nbytes: int) -> torch.Tensor:
    """The descriptor checks of tgsr_augment_u8 (include/tgsr_hip.h), on the host and with a message: returns the table as a
    contiguous int32 [B, 12] host tensor or raises TgsrError.  Touches no device."""
    t = torch.as_tensor(table)
    if t.is_cuda or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != AUG_DESC or t.shape[0] < 1:
        raise TgsrError("augment: the descriptor table is a host int32 [B, %d] tensor, got %s %s on %s"
                        % (AUG_DESC, t.dtype, tuple(t.shape), t.device))
    if not 1 <= int(S) <= AUG_MAX_SIDE:
        raise TgsrError("augment: window size %r is outside [1, %d]" % (S, AUG_MAX_SIDE))
    if not 1 <= int(nbytes) < 2 ** 31:
        raise TgsrError("augment: a packed buffer of %d bytes (must be in [1, 2^31))" % nbytes)
    t = t.contiguous()
    off, H, W, x1, y1, x2, y2, oh, ow, top, left, flip = (c.to(torch.int64) for c in t.unbind(1))
    rules = (
        ("a source side outside [1, %d]" % AUG_MAX_SIDE, (H < 1) | (W < 1) | (H > AUG_MAX_SIDE) | (W > AUG_MAX_SIDE)),
        ("an image outside the packed buffer", (off < 0) | (off + 3 * H * W > nbytes)),
        ("an empty crop box or one outside its image", (x1 < 0) | (x2 <= x1) | (x2 > W) | (y1 < 0) | (y2 <= y1) | (y2 > H)),
        ("a resized image smaller than the window", (oh < S) | (ow < S)),
        ("a resized side above %d" % AUG_MAX_OUT, (oh > AUG_MAX_OUT) | (ow > AUG_MAX_OUT)),
        ("a window outside the resized image", (top < 0) | (top > oh - S) | (left < 0) | (left > ow - S)),
        ("a reduction above %dx" % AUG_MAX_RATIO, (x2 - x1 > AUG_MAX_RATIO * ow) | (y2 - y1 > AUG_MAX_RATIO * oh)),
        ("a flip flag that is not 0 or 1", (flip != 0) & (flip != 1)),
    )
    for what, bad in rules:
        if bool(bad.any()):
            b = int(bad.nonzero()[0])
            raise TgsrError("augment: image %d has %s (descriptor %s, S = %d)" % (b, what, t[b].tolist(), S))
    return t


def augment_u8(packed: torch.Tensor, table, S: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch of crop -> Pillow `resize(BILINEAR)` -> window -> mirror over a ragged batch: `packed` uint8, the decoded
    H x W x 3 images back to back on the device; `table` the host int32 [B, 12] descriptors (check_augment_table).  Returns
    planar uint8 [B, 3, S, S] (`out` if given: dense, on the same device), per image the bytes of
    `img.crop((x1, y1, x2, y2)).resize((ow, oh), BILINEAR).crop((left, top, left + S, top + S))`, mirrored where flip is set.
    The C entry takes `packed` and `out` at any byte and the int32 tables and workspace on 4 bytes; what the workspace holds before
    the call does not matter; `out` is written whole (the kernels would leave an image whose device descriptor fails the checks as
    it was - here both copies are the checked table); on a refusal nothing is launched or written."""
    if not torch.is_tensor(packed) or packed.dtype != torch.uint8 or packed.dim() != 1:
        raise TgsrError("augment: the packed buffer is a flat uint8 tensor")
    packed = packed.contiguous()
    t = check_augment_table(table, S, packed.numel())
    B = t.shape[0]
    if B > 65535:
        raise TgsrError("augment: at most 65535 images per launch, got %d" % B)
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (B, 3, S, S) or not out.is_contiguous()):
        raise TgsrError("augment: out must be a dense uint8 [%d, 3, %d, %d] tensor" % (B, S, S))
    _need_hip(packed, out)
    L = _lib.lib()
    tdev = t.to(packed.device, non_blocking=True)
    ws = torch.empty(L.tgsr_augment_ws_elems(B, S), dtype=torch.int32, device=packed.device)
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=torch.uint8, device=packed.device)
    check(L.tgsr_augment_u8(_p(packed), packed.numel(), _p(t), _p(tdev), B, S, _p(ws), _p(out), _stream()), "tgsr_augment_u8")
    return out


def resize_coeffs_device(in_size: int, out_size: int, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """Pillow's precompute_coeffs (bilinear) computed on the device in fp64, the step augment_u8 runs per image and axis:
    (bounds int32 [out_size, 2] = (first input index, tap count), taps int32 [out_size, ksize] in 22-bit fixed point)."""
    in_size, out_size = int(in_size), int(out_size)
    if not (1 <= in_size <= AUG_MAX_OUT and 1 <= out_size <= AUG_MAX_OUT):
        raise TgsrError("resize_coeffs: sizes must lie in [1, %d], got %d -> %d" % (AUG_MAX_OUT, in_size, out_size))
    if in_size > AUG_MAX_RATIO * out_size:
        raise TgsrError("resize_coeffs: %d -> %d is a reduction above %dx" % (in_size, out_size, AUG_MAX_RATIO))
    dev = torch.device(device)
    if dev.type != "cuda":
        raise TgsrError("resize_coeffs_device computes on a HIP device, got %s" % dev)
    ks = resize_ksize(in_size, out_size)
    with torch.cuda.device(dev):
        bounds = torch.empty(out_size, 2, dtype=torch.int32, device=dev)
        taps = torch.empty(out_size, ks, dtype=torch.int32, device=dev)
        check(_lib.lib().tgsr_resize_coeffs(in_size, out_size, ks, _p(bounds), _p(taps), _stream()), "tgsr_resize_coeffs")
    return bounds, taps


# ----------------------------------------------------------------------------------------- stand-alone GLU
def glu(x: torch.Tensor) -> torch.Tensor:
    """GLU.forward (util.py:45-53): x[:, :C/2] * sigmoid(x[:, C/2:]) for x [B, C, ...] with C even."""
    _need_hip(x)
    x = _f32(x, "x").contiguous()
    if x.dim() < 2 or x.shape[1] % 2 != 0:
        raise TgsrError("glu: channels dont divide 2! (shape %s)" % (tuple(x.shape),))
    B, nc = x.shape[0], x.shape[1] // 2
    out = torch.empty((B, nc) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    if out.numel():
        check(_lib.lib().tgsr_glu(_p(x), None, _p(out), B, out.numel() // B, _stream()), "tgsr_glu")
    return out


def glu_bwd(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Backward of glu: dy [B, C/2, ...], x [B, C, ...] -> dx like x."""
    _need_hip(dy, x)
    x = _f32(x, "x").contiguous()
    dy = _f32(dy, "dy").contiguous()
    dx = torch.empty_like(x)
    if dx.numel():
        check(_lib.lib().tgsr_glu(_p(x), _p(dy), _p(dx), x.shape[0], dy.numel() // x.shape[0], _stream()), "tgsr_glu")
    return dx


# ----------------------------------------------------------------------------------------- image epilogue
def to_uint8(img: torch.Tensor) -> torch.Tensor:
    """trainer_objective.py:153-155 on the device: round(clip((x + 1) * 127.5, 0, 255)) -> uint8, same shape.
    Byte-identical to the reference's numpy expression (float32 add, multiply, round-half-even)."""
    _need_hip(img)
    x = _f32(img.detach(), "img").contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(_lib.lib().tgsr_to_uint8(_p(x), _p(out), x.numel(), _stream()), "tgsr_to_uint8")
    return out


# ----------------------------------------------------------------------------------------- whole images by tiles
TILE_DESC = 6            # int32 per window: y0, x0, oy0, oy1, ox0, ox1 (LR pixels; tgsr_amd.tiles.plan_tiles)
TILE_MAX_SIDE = 1 << 20  # LR H, W
TILE_MAX_TILE = 4096     # th, tw
STITCH_MAX = 12          # outputs per tile_stitch launch (TGSR_STITCH_MAX)


def _tile_table_host(table, H: int, W: int, th: int, tw: int) -> torch.Tensor:
    """The checks that cost no tensor operation: the table is readable host memory of the stated shape, the sides are in range."""
    t = torch.as_tensor(table)
    if t.is_cuda or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != TILE_DESC or not 1 <= t.shape[0] <= 65535:
        raise TgsrError("tiles: the window table is a host int32 [Tb, %d] tensor with 1 <= Tb <= 65535, got %s %s on %s"
                        % (TILE_DESC, t.dtype, tuple(t.shape), t.device))
    H, W, th, tw = int(H), int(W), int(th), int(tw)
    if not (1 <= H <= TILE_MAX_SIDE and 1 <= W <= TILE_MAX_SIDE):
        raise TgsrError("tiles: an image of %d x %d (sides must lie in [1, %d])" % (H, W, TILE_MAX_SIDE))
    if not (1 <= th <= min(H, TILE_MAX_TILE) and 1 <= tw <= min(W, TILE_MAX_TILE)):
        raise TgsrError("tiles: a %d x %d window for a %d x %d image (1 <= window <= min(side, %d))" % (th, tw, H, W, TILE_MAX_TILE))
    return t.contiguous()


def check_tile_table(table, H: int, W: int, th: int, tw: int) -> torch.Tensor:
    """The window checks of tgsr_tile_gather / tgsr_tile_stitch (include/tgsr_hip.h), on the host and with a message: returns
    the table as a contiguous int32 [Tb, 6] host tensor or raises TgsrError.  Touches no device.  tile_gather / tile_stitch leave
    the windows to the C entry's own pass over the host table and come here only for the message when it refuses."""
    t = _tile_table_host(table, H, W, th, tw)
    H, W, th, tw = int(H), int(W), int(th), int(tw)
    y0, x0, oy0, oy1, ox0, ox1 = (c.to(torch.int64) for c in t.unbind(1))
    rules = (
        ("a window outside the image", (y0 < 0) | (x0 < 0) | (y0 > H - th) | (x0 > W - tw)),
        ("owned rows that are empty or outside the window", (oy0 < y0) | (oy1 <= oy0) | (oy1 > y0 + th)),
        ("owned columns that are empty or outside the window", (ox0 < x0) | (ox1 <= ox0) | (ox1 > x0 + tw)),
    )
    for what, bad in rules:
        if bool(bad.any()):
            b = int(bad.nonzero()[0])
            raise TgsrError("tiles: window %d has %s (row %s, image %d x %d, window %d x %d)" % (b, what, t[b].tolist(), H, W, th, tw))
    return t


def _tile_table_dev(table_dev, t, device):
    if table_dev is None:
        return t.to(device)
    if (not table_dev.is_cuda or table_dev.dtype != torch.int32 or tuple(table_dev.shape) != tuple(t.shape)
            or not table_dev.is_contiguous()):
        raise TgsrError("tiles: table_dev must be the dense int32 %s device copy of the table" % (tuple(t.shape),))
    return table_dev


def tile_gather(img: torch.Tensor, table, th: int, tw: int, img2: Optional[torch.Tensor] = None,
                table_dev: Optional[torch.Tensor] = None):
    """Windows of one planar image [3, H, W] (and of a second one of the same shape and dtype - the blurred LR - in the same
    launch) as float32 [Tb, 3, th, tw] (tgsr_tile_gather): uint8 is normalised exactly like `u8_normalize`, float32 is a bit
    copy.  table: host int32 [Tb, 6] (check_tile_table); table_dev: its device copy where the caller keeps one.  Returns
    (LR, LRb) - LRb None without img2."""
    for name, x in (("img", img), ("img2", img2)):
        if x is None:
            continue
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[0] != 3 or x.dtype not in (torch.uint8, torch.float32):
            raise TgsrError("tile_gather: %s must be a planar uint8 or float32 [3, H, W] image, got %s" % (
                name, "%s %s" % (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__))
    if img2 is not None and (img2.shape != img.shape or img2.dtype != img.dtype):
        raise TgsrError("tile_gather: img2 is %s %s, img %s %s" % (img2.dtype, tuple(img2.shape), img.dtype, tuple(img.shape)))
    H, W = int(img.shape[1]), int(img.shape[2])
    t = _tile_table_host(table, H, W, th, tw)
    _need_hip(img, img2, table_dev)
    tdev = _tile_table_dev(table_dev, t, img.device)
    img = img.contiguous()
    img2 = None if img2 is None else img2.contiguous()
    Tb = t.shape[0]
    out = torch.empty(Tb, 3, th, tw, dtype=torch.float32, device=img.device)
    out2 = torch.empty_like(out) if img2 is not None else None
    rc = _lib.lib().tgsr_tile_gather(_p(img), _p(img2), int(img.dtype == torch.uint8), H, W, _p(t), _p(tdev), Tb, int(th), int(tw),
                                     _p(out), _p(out2), _stream())
    if rc:
        check_tile_table(t, H, W, th, tw)                  # the window at fault, by name
    check(rc, "tgsr_tile_gather")
    return out, out2


def tile_stitch(tiles, outs, table, H: int, W: int, th: int, tw: int, table_dev: Optional[torch.Tensor] = None) -> None:
    """The owned rectangle of every tile of every tile output, into the whole-image outputs, in one launch (tgsr_tile_stitch).
    tiles[e]: float32 [Tb, C, s th, s tw] with a dense (C, s th, s tw) block and any tile stride; outs[e]: dense [C, s H, s W],
    float32 (a bit copy) or uint8 (`to_uint8`'s bytes); the scale s is read off the shapes.  Pixels no tile owns keep what `outs`
    held, and so does the rectangle of a row of `table_dev` that fails the window checks (the kernel skips it).  No alignment is
    needed beyond the element's: a uint8 output may start at any byte."""
    tiles, outs = list(tiles), list(outs)
    n = len(tiles)
    if n < 1 or n != len(outs) or n > STITCH_MAX:
        raise TgsrError("tile_stitch: %d tile outputs for %d images (1 to %d per launch)" % (n, len(outs), STITCH_MAX))
    t = _tile_table_host(table, H, W, th, tw)
    Tb = t.shape[0]
    _need_hip(*tiles, *outs, table_dev)
    tdev = _tile_table_dev(table_dev, t, tiles[0].device)
    Cs, ss, u8s, strides = [], [], [], []
    for e, (x, o) in enumerate(zip(tiles, outs)):
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[0] != Tb:
            raise TgsrError("tile_stitch: tiles[%d] must be float32 [%d, C, s*%d, s*%d], got %s %s" % (e, Tb, th, tw, x.dtype, tuple(x.shape)))
        C, s = int(x.shape[1]), int(x.shape[2]) // int(th)
        if s < 1 or s > 64 or tuple(x.shape[2:]) != (s * th, s * tw) or C < 1 or C > 65535:
            raise TgsrError("tile_stitch: tiles[%d] %s is no [%d, C, s*%d, s*%d] for an integer scale 1 <= s <= 64"
                            % (e, tuple(x.shape), Tb, th, tw))
        if (x.stride(3) != 1 or x.stride(2) != s * tw or (C > 1 and x.stride(1) != s * th * s * tw)
                or (Tb > 1 and x.stride(0) < C * s * th * s * tw)):
            raise TgsrError("tile_stitch: tiles[%d] needs a dense (C, H, W) block per tile (strides %s)" % (e, tuple(x.stride())))
        if o.dtype not in (torch.float32, torch.uint8) or tuple(o.shape) != (C, s * H, s * W) or not o.is_contiguous():
            raise TgsrError("tile_stitch: outs[%d] must be a dense float32 or uint8 [%d, %d, %d], got %s %s"
                            % (e, C, s * H, s * W, o.dtype, tuple(o.shape)))
        Cs.append(C)
        ss.append(s)
        u8s.append(int(o.dtype == torch.uint8))
        strides.append(x.stride(0) if Tb > 1 else C * s * th * s * tw)
    src = (ctypes.c_void_p * n)(*[x.data_ptr() for x in tiles])
    dst = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    rc = _lib.lib().tgsr_tile_stitch(n, src, (ctypes.c_int64 * n)(*strides), dst, (ctypes.c_int * n)(*Cs), (ctypes.c_int * n)(*ss),
                                     (ctypes.c_int * n)(*u8s), int(H), int(W), _p(t), _p(tdev), Tb, int(th), int(tw), _stream())
    if rc:
        check_tile_table(t, H, W, th, tw)                  # the window at fault, by name
    check(rc, "tgsr_tile_stitch")


# ----------------------------------------------------------------------------------------- geometric self-ensemble (x8)
D8_MAX_N = 4096          # images per d8_gather / d8_merge launch
_D8_GROUPS = ((0, 8), (0, 4), (4, 4))


def d8_gather(img: torch.Tensor, table, th: int, tw: int, k0: int = 0, nk: int = 8, img2: Optional[torch.Tensor] = None,
              table_dev: Optional[torch.Tensor] = None):
    """The variants k0 .. k0 + nk - 1 (tgsr_amd.tiles: the transform) of every window of N planar images [N, 3, H, W] (and of a
    second batch of the same shape and dtype - the blurred LR - in the same launch) as float32 [N, Tb, nk, 3, th', tw']
    (tgsr_d8_gather): uint8 is normalised exactly like `u8_normalize`, float32 is a bit copy.  (k0, nk): (0, 8) - square windows
    only -, (0, 4) or (4, 4), the transposed group [N, Tb, 4, 3, tw, th].  table: host int32 [Tb, 6] (check_tile_table), applied to
    every image; table_dev: its device copy where the caller keeps one.  Returns (LR, LRb) - LRb None without img2."""
    for name, x in (("img", img), ("img2", img2)):
        if x is None:
            continue
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.dtype not in (torch.uint8, torch.float32):
            raise TgsrError("d8_gather: %s must be a batch of planar uint8 or float32 [N, 3, H, W] images, got %s" % (
                name, "%s %s" % (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__))
    if img2 is not None and (img2.shape != img.shape or img2.dtype != img.dtype):
        raise TgsrError("d8_gather: img2 is %s %s, img %s %s" % (img2.dtype, tuple(img2.shape), img.dtype, tuple(img.shape)))
    N, H, W = int(img.shape[0]), int(img.shape[2]), int(img.shape[3])
    k0, nk, th, tw = int(k0), int(nk), int(th), int(tw)
    if not 1 <= N <= D8_MAX_N:
        raise TgsrError("d8_gather: %d images (1 to %d per launch)" % (N, D8_MAX_N))
    if (k0, nk) not in _D8_GROUPS:
        raise TgsrError("d8_gather: variants k0 = %d, nk = %d - the groups are (0, 8), (0, 4) and (4, 4)" % (k0, nk))
    if nk == 8 and th != tw:
        raise TgsrError("d8_gather: all eight variants in one batch need a square window, got %d x %d - gather (0, 4) and (4, 4)"
                        % (th, tw))
    t = _tile_table_host(table, H, W, th, tw)
    _need_hip(img, img2, table_dev)
    tdev = _tile_table_dev(table_dev, t, img.device)
    img = img.contiguous()
    img2 = None if img2 is None else img2.contiguous()
    Tb = t.shape[0]
    hh, ww = (tw, th) if k0 == 4 else (th, tw)
    out = torch.empty(N, Tb, nk, 3, hh, ww, dtype=torch.float32, device=img.device)
    out2 = torch.empty_like(out) if img2 is not None else None
    rc = _lib.lib().tgsr_d8_gather(_p(img), _p(img2), int(img.dtype == torch.uint8), N, H, W, _p(t), _p(tdev), Tb, th, tw, k0, nk,
                                   _p(out), _p(out2), _stream())
    if rc:
        check_tile_table(t, H, W, th, tw)                  # the window at fault, by name
    check(rc, "tgsr_d8_gather")
    return out, out2


def d8_merge(srcs, outs, table, H: int, W: int, th: int, tw: int, srcs_t=None, table_dev: Optional[torch.Tensor] = None) -> None:
    """The owned rectangle of every window of the MEAN of the eight variant outputs, each mapped back (tgsr_amd.tiles: the
    transform and the fixed float32 summation order), into the whole-image outputs, in one launch (tgsr_d8_merge).
    srcs[e]: float32 [N * Tb * nk, C, s th, s tw], the outputs of the variant batch `d8_gather` made - a dense (C, s th, s tw) block
    per batch row, any row stride.  Without srcs_t nk = 8 (square windows); with it nk = 4 and srcs_t[e] is the transposed group
    [N * Tb * 4, C, s tw, s th] with the same row stride.  outs[e]: dense [N, C, s H, s W], float32 (the mean) or uint8 (`to_uint8`
    of the mean); N and the scale s are read off the shapes.  Pixels no window owns keep what `outs` held, and so does the
    rectangle of a row of `table_dev` that fails the window checks."""
    srcs, outs = list(srcs), list(outs)
    n = len(srcs)
    if n < 1 or n != len(outs) or n > STITCH_MAX:
        raise TgsrError("d8_merge: %d variant outputs for %d images (1 to %d per launch)" % (n, len(outs), STITCH_MAX))
    nk = 8 if srcs_t is None else 4
    srcs_t = [None] * n if srcs_t is None else list(srcs_t)
    if len(srcs_t) != n or any(x is None for x in srcs_t) != (nk == 8):
        raise TgsrError("d8_merge: srcs_t holds the transposed group of EVERY output (%d entries), or is None when srcs hold all "
                        "eight variants" % n)
    th, tw, H, W = int(th), int(tw), int(H), int(W)
    if nk == 8 and th != tw:
        raise TgsrError("d8_merge: eight variants in one batch need a square window, got %d x %d - pass the transposed group as "
                        "srcs_t" % (th, tw))
    t = _tile_table_host(table, H, W, th, tw)
    Tb = t.shape[0]
    _need_hip(*srcs, *[x for x in srcs_t if x is not None], *outs, table_dev)
    tdev = _tile_table_dev(table_dev, t, srcs[0].device)
    N = int(outs[0].shape[0]) if torch.is_tensor(outs[0]) and outs[0].dim() == 4 else 0
    if not 1 <= N <= D8_MAX_N or n * N > 65535:
        raise TgsrError("d8_merge: outs[0] must be [N, C, s*%d, s*%d] with 1 <= N <= %d and %d N <= 65535, got %s"
                        % (H, W, D8_MAX_N, n, tuple(outs[0].shape)))
    rows = N * Tb * nk
    Cs, ss, u8s, strides = [], [], [], []
    for e, (x, xt, o) in enumerate(zip(srcs, srcs_t, outs)):
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[0] != rows:
            raise TgsrError("d8_merge: srcs[%d] must be float32 [%d, C, s*%d, s*%d] (N = %d images x %d windows x %d variants), got "
                            "%s %s" % (e, rows, th, tw, N, Tb, nk, x.dtype, tuple(x.shape)))
        C, s = int(x.shape[1]), int(x.shape[2]) // th
        if s < 1 or s > 64 or tuple(x.shape[2:]) != (s * th, s * tw) or C < 1 or C > 65535:
            raise TgsrError("d8_merge: srcs[%d] %s is no [%d, C, s*%d, s*%d] for an integer scale 1 <= s <= 64"
                            % (e, tuple(x.shape), rows, th, tw))
        block = C * s * th * s * tw
        for name, y, hw in (("srcs", x, (s * th, s * tw)), ("srcs_t", xt, (s * tw, s * th))):
            if y is None:
                continue
            if y.dtype != torch.float32 or tuple(y.shape) != (rows, C) + hw:
                raise TgsrError("d8_merge: %s[%d] must be float32 %s, got %s %s" % (name, e, (rows, C) + hw, y.dtype, tuple(y.shape)))
            if (y.stride(3) != 1 or y.stride(2) != hw[1] or (C > 1 and y.stride(1) != hw[0] * hw[1]) or y.stride(0) < block
                    or y.stride(0) != x.stride(0)):
                raise TgsrError("d8_merge: %s[%d] needs a dense (C, H, W) block per batch row and one row stride for both groups "
                                "(strides %s)" % (name, e, tuple(y.stride())))
        if o.dtype not in (torch.float32, torch.uint8) or tuple(o.shape) != (N, C, s * H, s * W) or not o.is_contiguous():
            raise TgsrError("d8_merge: outs[%d] must be a dense float32 or uint8 [%d, %d, %d, %d], got %s %s"
                            % (e, N, C, s * H, s * W, o.dtype, tuple(o.shape)))
        Cs.append(C)
        ss.append(s)
        u8s.append(int(o.dtype == torch.uint8))
        strides.append(x.stride(0))
    srcA = (ctypes.c_void_p * n)(*[x.data_ptr() for x in srcs])
    srcB = (ctypes.c_void_p * n)(*[None if x is None else x.data_ptr() for x in srcs_t])
    dst = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    rc = _lib.lib().tgsr_d8_merge(n, srcA, srcB, (ctypes.c_int64 * n)(*strides), dst, (ctypes.c_int * n)(*Cs), (ctypes.c_int * n)(*ss),
                                  (ctypes.c_int * n)(*u8s), nk, N, H, W, _p(t), _p(tdev), Tb, th, tw, _stream())
    if rc:
        check_tile_table(t, H, W, th, tw)                  # the window at fault, by name
    check(rc, "tgsr_d8_merge")


# ----------------------------------------------------------------------------------------- image quality
METRICS_WINDOW = 11      # the SSIM window; a shaved crop may not be smaller


def _metrics_image(t: torch.Tensor, name: str, dtypes) -> torch.Tensor:
    if t.dtype not in dtypes:
        raise TgsrError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    if t.dim() != 4 or t.shape[1] != 3:
        raise TgsrError("%s must be [B, 3, H, W], got %s" % (name, tuple(t.shape)))
    if t.shape[0] < 1:
        raise TgsrError("%s: empty batch" % name)
    if not t.is_contiguous():
        raise TgsrError("%s must be contiguous NCHW (strides %s)" % (name, tuple(t.stride())))
    return t.detach()


def sr_metrics(sr: torch.Tensor, hr: torch.Tensor, shave: int = 0) -> torch.Tensor:
    """float64 [B, 3] = (SSE over RGB, SSE over Y, sum of the SSIM-on-Y window values) of `sr` against `hr` (tgsr_sr_metrics), on
    uint8 images: each input is uint8 NCHW or float32 NCHW (quantised in the kernel like `to_uint8`); `shave` pixels leave every
    border first.  The SSEs are exact integers; the crop has (H - 2 shave - 10)(W - 2 shave - 10) windows.  The workspace is
    exactly tgsr_sr_metrics_ws_elems doubles, uninitialised: the kernels write every element before they read it."""
    _need_hip(sr, hr)
    sr = _metrics_image(sr, "sr", (torch.float32, torch.uint8))
    hr = _metrics_image(hr, "hr", (torch.float32, torch.uint8))
    if sr.shape != hr.shape:
        raise TgsrError("sr_metrics: sr %s and hr %s differ in shape" % (tuple(sr.shape), tuple(hr.shape)))
    shave = int(shave)
    B, _, H, W = sr.shape
    if shave < 0 or H - 2 * shave < METRICS_WINDOW or W - 2 * shave < METRICS_WINDOW:
        raise ValueError("sr_metrics: %d x %d images shaved by %d leave a crop under %d x %d"
                         % (H, W, shave, METRICS_WINDOW, METRICS_WINDOW))
    L = _lib.lib()
    ws = torch.empty(L.tgsr_sr_metrics_ws_elems(B, H, W, shave), dtype=torch.float64, device=sr.device)
    out = torch.empty(B, 3, dtype=torch.float64, device=sr.device)
    check(L.tgsr_sr_metrics(_p(sr), int(sr.dtype == torch.float32), _p(hr), int(hr.dtype == torch.float32), B, H, W, shave,
                            _p(ws), _p(out), _stream()), "tgsr_sr_metrics")
    return out


def rgb_to_y(rgb: torch.Tensor) -> torch.Tensor:
    """The reference's rgb2y (trainer_objective.py:168-174) on uint8 [B, 3, H, W] -> uint8 [B, H, W], byte for byte."""
    _need_hip(rgb)
    rgb = _metrics_image(rgb, "rgb", (torch.uint8,))
    B, _, H, W = rgb.shape
    out = torch.empty(B, H, W, dtype=torch.uint8, device=rgb.device)
    check(_lib.lib().tgsr_rgb_to_y_u8(_p(rgb), B, H, W, _p(out), _stream()), "tgsr_rgb_to_y_u8")
    return out


NIQE_BLOCK = 96
_NIQE_TABLE = {}          # device -> (gam, r_gam) float64 tensors there


def niqe_gamma_table():
    """(gam, r_gam) as float64 numpy arrays: gam = np.arange(0.2, 10.001, 0.001) (9801 entries, numpy's own values) and
    r_gam = G(2 / gam)^2 / (G(1 / gam) G(3 / gam)), through lgamma in fp64 - strictly increasing, smallest step 1.7e-6."""
    import math
    import numpy as np
    gam = np.arange(0.2, 10.001, 0.001)
    r_gam = np.array([math.exp(2.0 * math.lgamma(2.0 / g) - math.lgamma(1.0 / g) - math.lgamma(3.0 / g)) for g in gam.tolist()])
    return gam, r_gam


def niqe_table_on(device):
    """The table on `device` (a tensor's own), built on the host and uploaded once per device (before any capture: the first call
    is eager)."""
    if device not in _NIQE_TABLE:
        _NIQE_TABLE[device] = tuple(torch.from_numpy(a).to(device) for a in niqe_gamma_table())
    return _NIQE_TABLE[device]


def niqe_features(img: torch.Tensor, shave: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(feats float64 [B, nblk, 36], sharp float64 [B, nblk]) of `img`, uint8 NCHW or float32 NCHW in [-1, 1] (quantised in the kernel
    like `to_uint8`): the NIQE features and the sharpness of every 96 x 96 block of the Y plane (tgsr_niqe_features; tgsr_amd.niqe
    states the definition).  `shave` pixels leave every border first; fewer than 96 on a side afterwards is a ValueError."""
    _need_hip(img)
    img = _metrics_image(img, "img", (torch.float32, torch.uint8))
    shave = int(shave)
    B, _, H, W = img.shape
    if shave < 0 or H - 2 * shave < NIQE_BLOCK or W - 2 * shave < NIQE_BLOCK:
        raise ValueError("niqe_features: %d x %d images shaved by %d leave a crop under %d x %d" % (H, W, shave, NIQE_BLOCK, NIQE_BLOCK))
    nblk = ((H - 2 * shave) // NIQE_BLOCK) * ((W - 2 * shave) // NIQE_BLOCK)
    L = _lib.lib()
    n_ws = L.tgsr_niqe_ws_elems(B, H, W, shave)
    if n_ws < 1:
        raise TgsrError("niqe_features: %d images of %d x %d shaved by %d refused" % (B, H, W, shave))
    gam, r_gam = niqe_table_on(img.device)
    ws = torch.empty(n_ws, dtype=torch.float64, device=img.device)
    feats = torch.empty(B, nblk, 36, dtype=torch.float64, device=img.device)
    sharp = torch.empty(B, nblk, dtype=torch.float64, device=img.device)
    check(L.tgsr_niqe_features(_p(img), int(img.dtype == torch.float32), B, H, W, shave, _p(gam), _p(r_gam), gam.numel(), _p(ws),
                               _p(feats), _p(sharp), _stream()), "tgsr_niqe_features")
    return feats, sharp


# ----------------------------------------------------------------------------------------- LPIPS (tgsr_lpips.hip)
LPIPS_MAX_TAPS = 8       # taps of one tgsr_lpips_finish launch


def maxpool2s2(x: torch.Tensor, out: torch.Tensor, o_coff: int):
    """F.max_pool2d(x, 2) of a dense fp32 NCHW x (H, W >= 2, floor) into channels [o_coff, o_coff + C) of out (tgsr_maxpool2s2_fwd)."""
    _need_hip(x, out)
    xp, xbs = _slice_ptr(x, 0)
    B, Cc, H, W = x.shape
    op, obs = _slice_ptr(out, o_coff)
    if H < 2 or W < 2 or out.shape[0] != B or out.shape[2] != H // 2 or out.shape[3] != W // 2 or o_coff < 0 or o_coff + Cc > out.shape[1]:
        raise TgsrError("maxpool2s2: %s -> channels %d.. of %s" % (tuple(x.shape), o_coff, tuple(out.shape)))
    check(_lib.lib().tgsr_maxpool2s2_fwd(xp, xbs, B, Cc, H, W, op, obs, _stream()), "tgsr_maxpool2s2_fwd")


def maxpool2s2_bwd(x: torch.Tensor, dy: torch.Tensor, dy_coff: int, dx: torch.Tensor, accumulate: bool, mask: Optional[torch.Tensor] = None):
    """dx (+)= the gradient of maxpool2s2 at x for dy = channels [dy_coff, dy_coff + C) of `dy`: to the first maximum of every window,
    kept where mask > 0 (mask dense, shaped like dx).  accumulate False writes dx whole (tgsr_maxpool2s2_bwd)."""
    _need_hip(x, dy, dx, mask)
    if mask is not None and (mask.shape != dx.shape or not mask.is_contiguous() or mask.dtype != torch.float32):
        raise TgsrError("maxpool2s2_bwd: the mask must be a dense fp32 tensor shaped like dx")
    xp, xbs = _slice_ptr(x, 0)
    B, Cc, H, W = x.shape
    gp, gbs = _slice_ptr(dy, dy_coff)
    dp, dbs = _slice_ptr(dx, 0)
    if (H < 2 or W < 2 or dx.shape != x.shape or dy.shape[0] != B or dy.shape[2] != H // 2 or dy.shape[3] != W // 2 or dy_coff < 0
            or dy_coff + Cc > dy.shape[1]):
        raise TgsrError("maxpool2s2_bwd: x %s, dy %s from channel %d, dx %s" % (tuple(x.shape), tuple(dy.shape), dy_coff, tuple(dx.shape)))
    check(_lib.lib().tgsr_maxpool2s2_bwd(xp, xbs, gp, gbs, B, Cc, H, W, dp, dbs, 1 if accumulate else 0, _p(mask), _stream()),
          "tgsr_maxpool2s2_bwd")


def lpips_nslots(C: int, HW: int) -> int:
    """Slots per image of lpips_layer's partial sums (tgsr_lpips_nslots): ceil(tiles / t) <= 512 for tiles of 16 (HW <= 1024) or 64
    pixels and t = ceil(tiles / 512) tiles per slot, at least 4 where HW >= 32768.  0 for a shape the kernels refuse."""
    return int(_lib.lib().tgsr_lpips_nslots(int(C), int(HW)))


def _lpips_feature(t, name, what):
    """(pointer, batch stride, B, C, HW) of a float32 [B, C, H, W] whose samples are dense (any batch stride, any 4-byte base)."""
    _dense_f32(t, name, what, "[B, C, H, W]")
    B, C, H, W = t.shape
    if t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W or (B > 1 and t.stride(0) < C * H * W):
        raise TgsrError("%s: %s %s with strides %s: dense samples expected (any batch stride)" % (what, name, tuple(t.shape), t.stride()))
    return _p(t), (t.stride(0) if B > 1 else C * H * W), B, C, H * W


def lpips_layer(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """One LPIPS tap (tgsr_lpips_layer_fwd): f0, f1 float32 [B, C, H, W] (dense samples, any batch stride), w float32 [C].  Returns
    partial float64 [B, lpips_nslots(C, H W)]: per slot sum_p sum_c w[c] (n(f0) - n(f1))^2, n(f) = f / (sqrt(sum_c f^2) + 1e-10) -
    `lpips_finish` sums the slots and divides by H W.  One launch, every feature read once."""
    p0, bs0, B, C, HW = _lpips_feature(f0, "f0", "lpips_layer")
    p1, bs1 = _lpips_feature(f1, "f1", "lpips_layer")[:2]
    if f1.shape != f0.shape or not torch.is_tensor(w) or w.dtype != torch.float32 or w.numel() != C or not w.is_contiguous():
        raise TgsrError("lpips_layer: f0 %s, f1 %s and a dense float32 w of %d weights expected" % (tuple(f0.shape), tuple(f1.shape), C))
    _need_hip(f0, f1, w)
    ns = lpips_nslots(C, HW)
    if ns < 1 or B > 65535:
        raise TgsrError("lpips_layer: %s refused" % (tuple(f0.shape),))
    partial = torch.empty(B, ns, dtype=torch.float64, device=f0.device)
    check(_lib.lib().tgsr_lpips_layer_fwd(p0, bs0, p1, bs1, _p(w), B, C, HW, _p(partial), _stream()), "tgsr_lpips_layer_fwd")
    return partial


def lpips_finish(partials, hws) -> Tuple[torch.Tensor, torch.Tensor]:
    """(per_layer float32 [L, B], total float32 [B]) of 1 to 8 taps' partial sums (lpips_layer) and their pixel counts H W: every tap's
    slots summed in index order and divided by H W, the taps summed in order (tgsr_lpips_finish, one launch)."""
    partials, hws = list(partials), [int(v) for v in hws]
    L = len(partials)
    if L < 1 or L > LPIPS_MAX_TAPS or len(hws) != L or min(hws) < 1:
        raise TgsrError("lpips_finish: %d taps with %d pixel counts, 1 to %d of each expected" % (L, len(hws), LPIPS_MAX_TAPS))
    B = partials[0].shape[0] if partials[0].dim() == 2 else 0
    for t in partials:
        if t.dim() != 2 or t.dtype != torch.float64 or not t.is_contiguous() or t.shape[0] != B or t.numel() == 0:
            raise TgsrError("lpips_finish: dense float64 [B, nslots] partial sums of one batch size expected")
    _need_hip(*partials)
    per_layer = torch.empty(L, B, dtype=torch.float32, device=partials[0].device)
    total = torch.empty(B, dtype=torch.float32, device=partials[0].device)
    check(_lib.lib().tgsr_lpips_finish(_ptr_array(partials), _int_array([t.shape[1] for t in partials]), _int_array(hws), L, B,
                                       _p(per_layer), _p(total), _stream()), "tgsr_lpips_finish")
    return per_layer, total


def lpips_layer_bwd(g: torch.Tensor, f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor, df0: torch.Tensor, accumulate: bool,
                    mask: Optional[torch.Tensor] = None):
    """df0 (+)= g[b] d(d_l[b]) / d(f0) of one LPIPS tap (tgsr_lpips_layer_bwd): g float32 [B] on the device, df0 shaped like f0 (dense
    samples, any batch stride), mask (nullable, df0's shape and strides) keeps the value where mask > 0.  accumulate False writes
    every element; a pixel whose f0 column is all zero gets 0."""
    p0, bs0, B, C, HW = _lpips_feature(f0, "f0", "lpips_layer_bwd")
    p1, bs1 = _lpips_feature(f1, "f1", "lpips_layer_bwd")[:2]
    dp, dbs = _lpips_feature(df0, "df0", "lpips_layer_bwd")[:2]
    if f1.shape != f0.shape or df0.shape != f0.shape or not torch.is_tensor(w) or w.dtype != torch.float32 or w.numel() != C or \
            not w.is_contiguous():
        raise TgsrError("lpips_layer_bwd: f0 %s, f1 %s, df0 %s and a dense float32 w of %d weights expected"
                        % (tuple(f0.shape), tuple(f1.shape), tuple(df0.shape), C))
    if not torch.is_tensor(g) or g.dtype != torch.float32 or g.numel() != B or not g.is_contiguous():
        raise TgsrError("lpips_layer_bwd: g must be a dense float32 [%d]" % B)
    if mask is not None and (_lpips_feature(mask, "mask", "lpips_layer_bwd")[1] != dbs or mask.shape != df0.shape):
        raise TgsrError("lpips_layer_bwd: the mask must have df0's shape and batch stride")
    _need_hip(g, f0, f1, w, df0, mask)
    if lpips_nslots(C, HW) < 1 or B > 65535:
        raise TgsrError("lpips_layer_bwd: %s refused" % (tuple(f0.shape),))
    check(_lib.lib().tgsr_lpips_layer_bwd(_p(g), p0, bs0, p1, bs1, _p(w), B, C, HW, dp, dbs, 1 if accumulate else 0, _p(mask), _stream()),
          "tgsr_lpips_layer_bwd")


# ----------------------------------------------------------------------------------------- attention panels
ATTN_MAX_SIDE, ATTN_MAX_TILE, ATTN_MAX_WORDS = 128, 512, 64


def check_cap_lens(cap_lens, B: int, T: int) -> list:
    """The host check of the caption lengths of an attention panel: B ints in [1, T].  Returns them as a list."""
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    if len(lens) != B or min(lens) < 1 or max(lens) > T:
        raise TgsrError("attn_panels: cap_lens %s must be %d lengths in [1, %d]" % (lens, B, T))
    return lens


def attn_panels(images: torch.Tensor, att: torch.Tensor, cap_lens, Mh: torch.Tensor, Mw: torch.Tensor, u: int, alpha: int, K: int,
                by_conf: bool, with_maps: bool):
    """tgsr_attn_panels: (panel uint8 [B, Vh, K (Vw + 2), 3], conf float64 [B, T], order int32 [B, T], maps uint8 [B, T, Vh, Vw] or
    [0]) from att [B, T, h, w] float32, cap_lens (B host ints in [1, T]), images [B, 3, u h, u w] float32 or uint8 and the fp64
    operators Mh [u h, h], Mw [u w, w] (attnviz.expand_operator).  The arithmetic: tgsr_amd/attnviz.py.
    The C entry takes panel, maps and a uint8 image at any byte, att, cap_lens, order and a float32 image on 4 bytes, Mh, Mw, the
    workspace and conf on 8 bytes (TGSR_EUNSUPPORTED otherwise); the workspace tiles of words behind a caption are neither written nor
    read; conf and order are written whole; on a refusal nothing is launched or written."""
    if att.dim() != 4:
        raise TgsrError("attn_panels: att [B, T, h, w] expected, got %s" % (tuple(att.shape),))
    B, T, h, w = att.shape
    lens = check_cap_lens(cap_lens, B, T)
    _need_hip(images, att, Mh, Mw)
    u, alpha, K = int(u), int(alpha), int(K)
    Vh, Vw = u * h, u * w
    if images.dtype not in (torch.float32, torch.uint8) or tuple(images.shape) != (B, 3, Vh, Vw):
        raise TgsrError("attn_panels: images must be float32 or uint8 [%d, 3, %d, %d], got %s %s"
                        % (B, Vh, Vw, images.dtype, tuple(images.shape)))
    for name, m, shape in (("Mh", Mh, (Vh, h)), ("Mw", Mw, (Vw, w))):
        if m.dtype != torch.float64 or tuple(m.shape) != shape:
            raise TgsrError("attn_panels: %s must be float64 %s, got %s %s" % (name, shape, m.dtype, tuple(m.shape)))
    if not (1 <= K <= T) or not (0 <= alpha <= 255) or u < 1:
        raise TgsrError("attn_panels: K %d (1..%d), alpha %d (0..255), u %d (>= 1)" % (K, T, alpha, u))
    L = _lib.lib()
    n_ws = L.tgsr_attn_panels_ws_elems(B, T, h, w, u)
    if n_ws <= 0:
        raise TgsrError("attn_panels: maps of %d x %d (sides 2..%d), tiles of %d x %d (<= %d) and %d words (<= %d) are what the "
                        "kernels take" % (h, w, ATTN_MAX_SIDE, Vh, Vw, ATTN_MAX_TILE, T, ATTN_MAX_WORDS))
    dev = att.device
    att = _f32(att.detach(), "att").contiguous()
    images = images.detach().contiguous()
    ws = torch.empty(n_ws, dtype=torch.float64, device=dev)
    panel = torch.empty(B, Vh, K * (Vw + 2), 3, dtype=torch.uint8, device=dev)
    maps = torch.empty((B, T, Vh, Vw) if with_maps else (0,), dtype=torch.uint8, device=dev)
    conf = torch.empty(B, T, dtype=torch.float64, device=dev)
    order = torch.empty(B, T, dtype=torch.int32, device=dev)
    rc = L.tgsr_attn_panels(_p(att), _p(_lens_on_device(tuple(lens), dev)), _p(images), int(images.dtype == torch.float32),
                            _p(Mh.contiguous()), _p(Mw.contiguous()), B, T, h, w, u, alpha, K, int(bool(by_conf)), _p(ws), _p(panel),
                            _p(maps) if with_maps else None, _p(conf), _p(order), _stream())
    check(rc, "tgsr_attn_panels")
    return panel, conf, order, maps


# ----------------------------------------------------------------------------------------- attention-guided losses
WMSE_MAX_WORDS = 255     # the saved argmax word of a map pixel is one byte


def _dense_f32(t, name: str, what: str, form: str) -> torch.Tensor:
    """A non-empty float32 tensor of as many dimensions as `form` ("[B, C, H, W]") names, or TgsrError."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != form.count(",") + 1:
        raise TgsrError("%s: %s must be a float32 %s tensor, got %s"
                        % (what, name, form, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    if t.numel() == 0:
        raise TgsrError("%s: %s %s is empty" % (what, name, tuple(t.shape)))
    return t


def check_weight_mse(fake_shape, label_shape, att_shape) -> Tuple[int, ...]:
    """The shape checks of tgsr_weight_mse_fwd / _bwd (include/tgsr_hip.h) on the host and with a message: fake, label [B, C, H, W]
    against att [B, T, h, w] with H = r h, W = r w for one integer r >= 1 and T <= 255.  Returns (B, C, T, H, W, h, w, r) or raises
    TgsrError.  Touches no device."""
    fs, ls, ms = (tuple(int(v) for v in s) for s in (fake_shape, label_shape, att_shape))
    if len(fs) != 4 or len(ms) != 4 or min(fs) < 1 or min(ms) < 1:
        raise TgsrError("weight_mse: fake [B, C, H, W] and att [B, T, h, w] expected, got %s and %s" % (fs, ms))
    if ls != fs:
        raise TgsrError("weight_mse: fake %s and label %s differ in shape" % (fs, ls))
    (B, C, H, W), (Bm, T, h, w) = fs, ms
    if Bm != B:
        raise TgsrError("weight_mse: %d images against the maps of %d" % (B, Bm))
    if T > WMSE_MAX_WORDS:
        raise TgsrError("weight_mse: %d words per map, the kernels take at most %d (the saved argmax is one byte)" % (T, WMSE_MAX_WORDS))
    if H % h or W % w or H // h != W // w:
        raise TgsrError("weight_mse: %d x %d images over %d x %d maps is no integer ratio (the kernels take H = r h, W = r w; "
                        "miscc.losses.weight_MSE(fused=False) interpolates any size)" % (H, W, h, w))
    return B, C, T, H, W, h, w, H // h


def attn_confidence(att: torch.Tensor, cap_lens: torch.Tensor) -> torch.Tensor:
    """conf float32 [B, T] of words_reweight_loss (tgsr_attn_confidence): for t < cap_lens[b] the fp32 sum of the values of
    att[b, t] strictly above float32(2 * (2 / cap_lens[b])), 0 behind the caption's length; a length outside [1, T] gives a zero
    row.  att: float32 [B, T, ...] (the trailing dimensions are one map); cap_lens: int32 [B] ON THE DEVICE - nothing here reads it
    on the host."""
    if not torch.is_tensor(att) or att.dtype != torch.float32 or att.dim() < 3 or att.numel() == 0:
        raise TgsrError("attn_confidence: att must be a non-empty float32 [B, T, ...] tensor, got %s"
                        % ("%s %s" % (att.dtype, tuple(att.shape)) if torch.is_tensor(att) else type(att).__name__))
    B, T = int(att.shape[0]), int(att.shape[1])
    if T > WMSE_MAX_WORDS or B > 65535:
        raise TgsrError("attn_confidence: %d captions of %d words; the kernel takes at most 65535 of %d" % (B, T, WMSE_MAX_WORDS))
    if not torch.is_tensor(cap_lens) or cap_lens.dtype != torch.int32 or tuple(cap_lens.shape) != (B,):
        raise TgsrError("attn_confidence: cap_lens must be an int32 [%d] tensor, got %s"
                        % (B, "%s %s" % (cap_lens.dtype, tuple(cap_lens.shape)) if torch.is_tensor(cap_lens) else type(cap_lens).__name__))
    _need_hip(att, cap_lens)
    att = att.detach().contiguous()
    conf = torch.empty(B, T, dtype=torch.float32, device=att.device)
    check(_lib.lib().tgsr_attn_confidence(_p(att), _p(cap_lens.contiguous()), B, T, att.numel() // (B * T), _p(conf), _stream()),
          "tgsr_attn_confidence")
    return conf


def weight_mse(fake: torch.Tensor, label: torch.Tensor, att: torch.Tensor, want_wlast: bool = False):
    """One scale of weight_MSE (tgsr_weight_mse_fwd): (loss [], wmax float32 [B, h, w], widx uint8 [B, h, w], wlast float32
    [B, 1, H, W] or [0]) - the term sum(T wups (fake - label)^2) / (H W B C), the per-pixel maximum over the words and its word (the
    lowest on a tie) for `weight_mse_bwd`, and on request the up-sampled maximum."""
    for name, t in (("fake", fake), ("label", label), ("att", att)):
        _dense_f32(t, name, "weight_mse", "[B, T, h, w]" if name == "att" else "[B, C, H, W]")
    B, C, T, H, W, h, w, _r = check_weight_mse(fake.shape, label.shape, att.shape)
    _need_hip(fake, label, att)
    fake, label, att = fake.detach().contiguous(), label.detach().contiguous(), att.detach().contiguous()
    dev = fake.device
    L = _lib.lib()
    ws = torch.empty(L.tgsr_weight_mse_ws_elems(B, C, T, H, W, h, w), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    wmax = torch.empty(B, h, w, dtype=torch.float32, device=dev)
    widx = torch.empty(B, h, w, dtype=torch.uint8, device=dev)
    wlast = torch.empty((B, 1, H, W) if want_wlast else (0,), dtype=torch.float32, device=dev)
    check(L.tgsr_weight_mse_fwd(_p(fake), _p(label), _p(att), B, C, T, H, W, h, w, _p(ws), _p(loss), _p(wmax), _p(widx),
                                _p(wlast) if want_wlast else None, _stream()), "tgsr_weight_mse_fwd")
    return loss, wmax, widx, wlast


def weight_mse_bwd(grad: torch.Tensor, fake: torch.Tensor, label: torch.Tensor, wmax: torch.Tensor, widx: torch.Tensor, T: int,
                   need_fake: bool = True, need_label: bool = False, need_att: bool = False):
    """(d_fake, d_label, d_att) of weight_mse (tgsr_weight_mse_bwd), None where not asked for: grad the [] gradient of the term,
    wmax / widx what the forward saved, T the number of words.  d_att [B, T, h, w] is written completely (zeros off the argmax)."""
    for name, t in (("fake", fake), ("label", label)):
        _dense_f32(t, name, "weight_mse_bwd", "[B, C, H, W]")
    _dense_f32(wmax, "wmax", "weight_mse_bwd", "[B, h, w]")
    if not torch.is_tensor(widx) or widx.dtype != torch.uint8 or widx.shape != wmax.shape:
        raise TgsrError("weight_mse_bwd: widx must be uint8 %s like wmax, got %s"
                        % (tuple(wmax.shape), "%s %s" % (widx.dtype, tuple(widx.shape)) if torch.is_tensor(widx) else type(widx).__name__))
    if not torch.is_tensor(grad) or grad.dtype != torch.float32 or grad.numel() != 1:
        raise TgsrError("weight_mse_bwd: grad must be one float32 value, got %s"
                        % ("%s %s" % (grad.dtype, tuple(grad.shape)) if torch.is_tensor(grad) else type(grad).__name__))
    T = int(T)
    if T < 1:
        raise TgsrError("weight_mse_bwd: T = %d words" % T)
    B, C, T, H, W, h, w, _r = check_weight_mse(fake.shape, label.shape, (wmax.shape[0], T, wmax.shape[1], wmax.shape[2]))
    if not (need_fake or need_label or need_att):
        raise TgsrError("weight_mse_bwd: no gradient asked for")
    _need_hip(grad, fake, label, wmax, widx)
    fake, label = fake.detach().contiguous(), label.detach().contiguous()
    dev = fake.device
    d_fake = torch.empty(B, C, H, W, dtype=torch.float32, device=dev) if need_fake else None
    d_label = torch.empty(B, C, H, W, dtype=torch.float32, device=dev) if need_label else None
    d_att = torch.empty(B, T, h, w, dtype=torch.float32, device=dev) if need_att else None
    check(_lib.lib().tgsr_weight_mse_bwd(_p(grad.contiguous()), _p(fake), _p(label), _p(wmax.contiguous()), _p(widx.contiguous()),
                                         B, C, T, H, W, h, w, _p(d_fake), _p(d_label), _p(d_att), _stream()), "tgsr_weight_mse_bwd")
    return d_fake, d_label, d_att


# ----------------------------------------------------------------------------------------- cycle-consistency loss
CYCLE_MAX_SCALES = 8     # scale descriptors of one launch (tgsr_cycle_mse.hip)
CYCLE_MAX_SIDE = 65536   # every image side: the backward's candidate ranges are float32 arithmetic


def check_cycle_mse(sr_shapes, lr_shape) -> Tuple[int, ...]:
    """The shape checks of tgsr_cycle_mse_fwd / _bwd (include/tgsr_hip.h) on the host and with a message: 1 to 8 SR images
    [B, C, H_i, W_i] against one LR image [B, C, h, w], every size in [1, 65536], H_i / h and W_i / w arbitrary.  Returns
    (n, B, C, h, w, (H_0, W_0, H_1, W_1, ...)) or raises TgsrError.  Touches no device."""
    shapes = [tuple(int(v) for v in s) for s in sr_shapes]
    ls = tuple(int(v) for v in lr_shape)
    if not 1 <= len(shapes) <= CYCLE_MAX_SCALES:
        raise TgsrError("cycle_mse: %d scales, the kernels take 1 to %d in one call" % (len(shapes), CYCLE_MAX_SCALES))
    if len(ls) != 4 or min(ls) < 1:
        raise TgsrError("cycle_mse: lr [B, C, h, w] expected (no empty dimension), got %s" % (ls,))
    B, C, h, w = ls
    sizes = []
    for i, s in enumerate(shapes):
        if len(s) != 4 or min(s) < 1:
            raise TgsrError("cycle_mse: sr[%d] [B, C, H, W] expected (no empty dimension), got %s" % (i, s))
        if s[:2] != (B, C):
            raise TgsrError("cycle_mse: sr[%d] %s and lr %s differ in batch or channels" % (i, s, ls))
        sizes += [s[2], s[3]]
    if max(sizes + [h, w]) > CYCLE_MAX_SIDE:
        raise TgsrError("cycle_mse: an image side of %d pixels, the kernels take at most %d" % (max(sizes + [h, w]), CYCLE_MAX_SIDE))
    return len(shapes), B, C, h, w, tuple(sizes)


def _int_array(values):
    return (ctypes.c_int * len(values))(*values)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def cycle_mse(sr, lr: torch.Tensor):
    """CycleMSE (tgsr_cycle_mse_fwd): `sr` a list of 1 to 8 float32 images [B, C, H_i, W_i], `lr` float32 [B, C, h, w].  Returns
    (loss [], terms [n], diff [n, B, C, h, w]): sum_i mean((bicubic(sr_i -> h x w) - lr)^2), its per-scale terms, and the
    differences `cycle_mse_bwd` reads.  One forward launch for all scales and one finish launch; dense tensors at any 4-byte
    aligned base."""
    sr = list(sr)
    for i, t in enumerate(sr):
        _dense_f32(t, "sr[%d]" % i, "cycle_mse", "[B, C, H, W]")
    _dense_f32(lr, "lr", "cycle_mse", "[B, C, h, w]")
    n, B, C, h, w, sizes = check_cycle_mse([t.shape for t in sr], lr.shape)
    _need_hip(lr, *sr)
    sr, lr = [t.detach().contiguous() for t in sr], lr.detach().contiguous()
    dev = lr.device
    L = _lib.lib()
    Hs, Ws = _int_array(sizes[0::2]), _int_array(sizes[1::2])
    ws = torch.empty(L.tgsr_cycle_mse_ws_elems(Hs, Ws, n, B, C, h, w), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    terms = torch.empty(n, dtype=torch.float32, device=dev)
    diff = torch.empty(n, B, C, h, w, dtype=torch.float32, device=dev)
    check(L.tgsr_cycle_mse_fwd(_ptr_array(sr), Hs, Ws, n, _p(lr), B, C, h, w, _p(ws), _p(diff), _p(loss), _p(terms), _stream()),
          "tgsr_cycle_mse_fwd")
    return loss, terms, diff


def cycle_mse_bwd(grad: torch.Tensor, diff: torch.Tensor, sizes, need_sr=None, need_lr: bool = False):
    """(d_sr list, d_lr) of cycle_mse (tgsr_cycle_mse_bwd), None where not asked for: grad the [] gradient of the loss ON THE DEVICE,
    diff [n, B, C, h, w] what the forward saved, sizes = (H_0, W_0, H_1, W_1, ...) of the SR images, need_sr one flag per scale
    (default: all).  Every d_sr[i] [B, C, H_i, W_i] is written completely (zeros where no tap lands), in one launch for all scales."""
    _dense_f32(diff, "diff", "cycle_mse_bwd", "[n, B, C, h, w]")
    if not torch.is_tensor(grad) or grad.dtype != torch.float32 or grad.numel() != 1:
        raise TgsrError("cycle_mse_bwd: grad must be one float32 value, got %s"
                        % ("%s %s" % (grad.dtype, tuple(grad.shape)) if torch.is_tensor(grad) else type(grad).__name__))
    sizes = [int(v) for v in sizes]
    n, B, C, h, w = (int(v) for v in diff.shape)
    if len(sizes) != 2 * n:
        raise TgsrError("cycle_mse_bwd: %d sizes for the %d scales of diff %s (H and W of each expected)" % (len(sizes), n, tuple(diff.shape)))
    check_cycle_mse([(B, C, sizes[2 * i], sizes[2 * i + 1]) for i in range(n)], (B, C, h, w))
    need_sr = [True] * n if need_sr is None else [bool(v) for v in need_sr]
    if len(need_sr) != n:
        raise TgsrError("cycle_mse_bwd: %d need_sr flags for %d scales" % (len(need_sr), n))
    if not (any(need_sr) or need_lr):
        raise TgsrError("cycle_mse_bwd: no gradient asked for")
    _need_hip(grad, diff)
    diff = diff.detach().contiguous()
    dev = diff.device
    d_sr = [torch.empty(B, C, sizes[2 * i], sizes[2 * i + 1], dtype=torch.float32, device=dev) if need_sr[i] else None for i in range(n)]
    d_lr = torch.empty(B, C, h, w, dtype=torch.float32, device=dev) if need_lr else None
    check(_lib.lib().tgsr_cycle_mse_bwd(_p(grad.detach().contiguous()), _p(diff), _int_array(sizes[0::2]), _int_array(sizes[1::2]), n, B, C,
                                        h, w, _ptr_array(d_sr), _p(d_lr), _stream()), "tgsr_cycle_mse_bwd")
    return d_sr, d_lr


# ----------------------------------------------------------------------------------------- discriminator convolutions
def _dconv(kind: int):
    L = _lib.lib()
    if kind == 4:
        return L.tgsr_conv4x4s2_ws_elems, L.tgsr_conv4x4s2_fwd, L.tgsr_conv4x4s2_dgrad, L.tgsr_conv4x4s2_wgrad, "tgsr_conv4x4s2"
    return (L.tgsr_conv3x3_gemm_ws_elems, L.tgsr_conv3x3_gemm_fwd, L.tgsr_conv3x3_gemm_dgrad, L.tgsr_conv3x3_gemm_wgrad,
            "tgsr_conv3x3_gemm")


def _dconv_fwd(kind, x, w, leaky):
    _need_hip(x, w)
    x = _f32(x, "x").contiguous()
    w = _f32(w.detach(), "w").contiguous()
    B, Cin, H, W = x.shape
    if tuple(w.shape[1:]) != (Cin, kind, kind):
        raise TgsrError("conv%dx%d: weight %s vs input %s" % (kind, kind, tuple(w.shape), tuple(x.shape)))
    ws_elems, fwd, _, _, name = _dconv(kind)
    Cout = w.shape[0]
    Ho, Wo = (H // 2, W // 2) if kind == 4 else (H, W)
    out = torch.empty(B, Cout, Ho, Wo, dtype=torch.float32, device=x.device)
    ws = torch.empty(ws_elems(0, B, Cin, H, W, Cout), dtype=torch.float32, device=x.device)
    e0 = _ev() if profile is not None else None
    if kind == 4:
        check(fwd(_p(x), B, Cin, H, W, _p(w), Cout, 1 if leaky else 0, _p(ws), _p(out), _stream()), name + "_fwd")
    else:
        assert not leaky
        check(fwd(_p(x), B, Cin, H, W, _p(w), Cout, _p(ws), _p(out), _stream()), name + "_fwd")
    _dconv_profile(e0, kind, B, Cin, H, W, Cout, Ho, Wo)
    return out


def _dconv_profile(e0, kind, B, Cin, H, W, Cout, Ho, Wo, op=0):
    """bench.py's per-launch hook for the discriminators' implicit-GEMM kernels (forward / data / weight gradient alike:
    2 B Ho Wo Cout Cin K^2 FLOPs, every one of them issued - no Winograd saving here; `dconv_igemm6_kernel` when the library
    takes the three-piece bf16 form for this shape: six bf16 MFMAs per fp32 MAC)."""
    if profile is not None:
        L = _lib.lib()
        split = (L.tgsr_conv4x4s2_split_form if kind == 4 else L.tgsr_conv3x3_gemm_split_form)(op, B, Cin, H, W, Cout)
        profile.append(("dconv_igemm6_kernel" if split else "dconv_igemm_kernel", 2.0 * B * Ho * Wo * Cout * Cin * kind * kind,
                        4.0 * (B * Cin * H * W + B * Cout * Ho * Wo + Cout * Cin * kind * kind), e0, _ev()))


def _dconv_dgrad(kind, dy, w, H, W):
    _need_hip(dy, w)
    dy = _f32(dy, "dy").contiguous()
    w = _f32(w.detach(), "w").contiguous()
    B, Cout, Cin = dy.shape[0], w.shape[0], w.shape[1]
    ws_elems, _, dgrad, _, name = _dconv(kind)
    dx = torch.empty(B, Cin, H, W, dtype=torch.float32, device=dy.device)
    ws = torch.empty(ws_elems(1, B, Cin, H, W, Cout), dtype=torch.float32, device=dy.device)
    e0 = _ev() if profile is not None else None
    check(dgrad(_p(dy), B, Cin, H, W, _p(w), Cout, _p(ws), _p(dx), _stream()), name + "_dgrad")
    _dconv_profile(e0, kind, B, Cin, H, W, Cout, dy.shape[2], dy.shape[3], 1)
    return dx


def _dconv_wgrad(kind, dy, x, out=None):
    _need_hip(dy, x)
    dy = _f32(dy, "dy").contiguous()
    x = _f32(x, "x").contiguous()
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    ws_elems, _, _, wgrad, name = _dconv(kind)
    ws = torch.empty(ws_elems(2, B, Cin, H, W, Cout), dtype=torch.float32, device=x.device)
    dw = out if out is not None else torch.empty(Cout, Cin, kind, kind, dtype=torch.float32, device=x.device)
    e0 = _ev() if profile is not None else None
    check(wgrad(_p(dy), _p(x), B, Cin, H, W, Cout, _p(ws), _p(dw), _stream()), name + "_wgrad")
    _dconv_profile(e0, kind, B, Cin, H, W, Cout, dy.shape[2], dy.shape[3], 2)
    return dw


def dconv_set_split(on: int) -> int:
    """The discriminators' 4x4 convolutions on the bf16 matrix pipe with three-piece fp32 operands (default on; profiles/HISTORY.md 3.18) or
    on the fp32 MFMA.  Returns the previous setting (tgsr_dconv_set_split)."""
    return _lib.lib().tgsr_dconv_set_split(int(on))


def conv4x4s2(x: torch.Tensor, w: torch.Tensor, leaky: bool = False) -> torch.Tensor:
    """nn.Conv2d(Cin, Cout, 4, 2, 1, bias=False) (downBlock, util.py:92-98) [+ LeakyReLU(0.2)]: x [B,Cin,H,W] ->
    [B,Cout,H/2,W/2]."""
    return _dconv_fwd(4, x, w, leaky)


def conv4x4s2_dgrad(dy: torch.Tensor, w: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Data gradient of conv4x4s2: dy [B,Cout,H/2,W/2] -> dx [B,Cin,H,W]."""
    return _dconv_dgrad(4, dy, w, H, W)


def conv4x4s2_wgrad(dy: torch.Tensor, x: torch.Tensor, out=None) -> torch.Tensor:
    """Weight gradient of conv4x4s2: dy [B,Cout,H/2,W/2], x [B,Cin,H,W] -> dw [Cout,Cin,4,4]."""
    return _dconv_wgrad(4, dy, x, out)


def conv3x3_gemm(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """conv3x3 stride 1 pad 1 without bias as an implicit GEMM: the discriminators' many-channel, few-pixel layers
    (Block3x3_leakRelu at 4x4 pixels, 512 ... 2048 channels)."""
    return _dconv_fwd(3, x, w, False)


def conv3x3_gemm_dgrad(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return _dconv_dgrad(3, dy, w, dy.shape[2], dy.shape[3])


def conv3x3_gemm_wgrad(dy: torch.Tensor, x: torch.Tensor, out=None) -> torch.Tensor:
    return _dconv_wgrad(3, dy, x, out)


def conv3x3_gemm_pays(Cin: int, Cout: int, H: int, W: int) -> bool:
    """Many channels on few pixels: the GEMM form; the generator's shapes stay on the tiled conv kernels."""
    return Cin >= 256 and Cout >= 256 and H * W <= 64 * 64


def leaky_relu_bwd(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dy * (y > 0 ? 1 : 0.2) from the forward OUTPUT y of a LeakyReLU(0.2)."""
    _need_hip(dy, y)
    dy = _f32(dy, "dy").contiguous()
    y = _f32(y, "y").contiguous()
    out = torch.empty_like(dy)
    check(_lib.lib().tgsr_leaky_relu(_p(dy), _p(y), _p(out), dy.numel(), _stream()), "tgsr_leaky_relu")
    return out
