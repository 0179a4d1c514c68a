"""Learned perceptual distance on the device: LPIPS v0.1 with the VGG16 trunk (Zhang, Isola, Efros, Shechtman and Wang, "The
unreasonable effectiveness of deep features as a perceptual metric", 2018) - the full-reference score of a GAN-SR table that does not
punish texture, and the same quantity as a training term (SRTrainer(perceptual=)).  Lower is better.

The definition (`net='vgg'`, `spatial=False`); x, y [B, 3, H, W] in [-1, 1]:
  scaling   s(x) = (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
  trunk     torchvision's vgg16().features[0:30]: thirteen 3 x 3 / stride 1 / pad 1 convolutions with bias + ReLU, four 2 x 2 max pools
  taps      the outputs of ReLU 1_2, 2_2, 3_3, 4_3, 5_3 (indices 3, 8, 15, 22, 29): 64, 128, 256, 512, 512 channels at H, H/2, H/4, H/8, H/16
  per tap   n(f) = f / (sqrt(sum_c f^2) + 1e-10),  d_l[b] = mean_p sum_c w_l[c] (n(f0) - n(f1))^2,  d[b] = sum_l d_l[b]
  gradient  only d(d)/d(x): the trunk is frozen and y is the target.  Where a pixel's whole channel column of f0 is zero torch's autograd
            returns NaN (sqrt'(0)); this build writes 0 there (the ReLU mask drops that contribution anyway).

The trained weights (torchvision's VGG16 and the lpips package's linear layers) are third-party and NOT shipped: a figure comparable
with PUBLISHED LPIPS numbers needs them (`load_state_dict` / `load`); `LPIPS.random(seed)` serves tests and benchmarks.  AlexNet is
out: its first layer is 11 x 11 / stride 4, 121 taps and a stride tgsr_gconv does not take.

Device tensors: the scaling in torch (three channels), then one stream of tgsr::gconv (filters packed once per weight version, bias +
ReLU in the epilogue, the exact three-piece bf16 form where Cin 9 % 16 == 0), tgsr::maxpool2s2, and per tap tgsr::lpips_layer (one pass
over the pair of features) with one tgsr::lpips_finish - a missing library is an error, never a fall-back.  x and y are walked as ONE
batch of 2 B.  With x.requires_grad the walk keeps its tape and runs it in reverse on the same kernels (tgsr::lpips_layer_bwd into the
tap's gradient, the data gradients with the consumer-side ReLU masks, tgsr::maxpool2s2_bwd); nothing in either direction synchronises
or reads device data on the host, so both are capturable.  CPU tensors run the same definition in torch float32 (host tests).
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import custom_ops as C
from . import ops
from .parallel import gather_rows

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
VGG16 = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
TAPS = (3, 8, 15, 22, 29)
WIDTHS = (64, 128, 256, 512, 512)
MIN_SIDE = 16
EPS = 1e-10


def _features():
    layers, cin = [], 3
    for v in VGG16:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=False)]
            cin = v
    return nn.Sequential(*layers)


def _translate(sd):
    """A state dict in one of the three layouts -> this module's keys.  The two foreign layouts are written down from memory of the
    lpips package and NOT verified against its files here."""
    out = {}
    for k, v in sd.items():
        p = k.split(".")
        if p[0] == "net" and len(p) == 4 and p[1].startswith("slice"):              # net.slice{k}.{i}.weight
            out["features.%s.%s" % (p[2], p[3])] = v
        elif p[0] == "lins" and len(p) == 5 and p[2:] == ["model", "1", "weight"]:   # lins.{k}.model.1.weight
            out["lin%s" % p[1]] = v
        elif p[0].startswith("lin") and p[1:] == ["model", "1", "weight"]:           # lin{k}.model.1.weight
            out[p[0]] = v
        elif p[0] == "scaling_layer":                                                # the constants above
            continue
        else:
            out[k] = v
    return out


class LPIPS(nn.Module):
    """LPIPS v0.1 / VGG16.  Parameters under torchvision's names (`features.{0,2,5,...,28}.weight / .bias`) plus `lin{0..4}`
    [1, C, 1, 1], all frozen.  `forward(x, y)` -> d [B] (float32)."""

    def __init__(self):
        super().__init__()
        self.features = _features()
        for k, c in enumerate(WIDTHS):
            setattr(self, "lin%d" % k, nn.Parameter(torch.zeros(1, c, 1, 1)))
        self.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1), persistent=False)
        for p in self.parameters():
            p.requires_grad_(False)
        self._packs = {}                          # conv index -> (key, forward pack, data-gradient pack)

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict=True, **kw):
        """Besides this module's own keys: the lpips package's linear-layer file (`lin{k}.model.1.weight` alone: the trunk keeps its
        weights) and its full-module layout (`net.slice{k}.{i}.*`, `lins.*` / `lin{k}.model.1.weight`, `scaling_layer.*`) - both
        layouts unverified: written from memory of that package, which was not at hand."""
        sd = _translate(state_dict)
        if strict and sd and not any(k.startswith("features.") for k in sd):
            missing = [k for k in ("lin%d" % i for i in range(len(WIDTHS))) if k not in sd]
            if missing:
                raise RuntimeError("LPIPS.load_state_dict: a linear-layer file without %s" % ", ".join(missing))
            res = super().load_state_dict(sd, strict=False, **kw)
            if res.unexpected_keys:
                raise RuntimeError("LPIPS.load_state_dict: unexpected keys %s" % ", ".join(res.unexpected_keys))
            return res
        return super().load_state_dict(sd, strict=strict, **kw)

    def save(self, path):
        """The state dict (this module's keys) at exactly `path`."""
        with open(path, "wb") as f:
            torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, f)
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        """A module saved by `save`, or a state dict in one of the layouts `load_state_dict` takes, on `device`."""
        m = cls()
        m.load_state_dict(torch.load(os.fspath(path), map_location="cpu", weights_only=True))
        return m.to(device)

    @classmethod
    def random(cls, seed=0, device="cpu"):
        """Seeded weights for tests and benchmarks: He-normal filters (activations keep their size through thirteen layers), small
        normal biases, lin weights uniform in [0, 0.1].  NOT a perceptual metric."""
        g = torch.Generator().manual_seed(int(seed))
        m = cls()
        with torch.no_grad():
            for mod in m.features:
                if isinstance(mod, nn.Conv2d):
                    mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / (mod.in_channels * 9)) ** 0.5)
                    mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
            for k in range(len(WIDTHS)):
                getattr(m, "lin%d" % k).copy_(torch.rand(1, WIDTHS[k], 1, 1, generator=g) * 0.1)
        return m.to(device)

    def lins(self):
        return [getattr(self, "lin%d" % k) for k in range(len(WIDTHS))]

    def refresh(self):
        """Packs every filter for tgsr::gconv (forward and data gradient), once per weight version.  `forward` calls it; call it
        yourself before capturing a forward into a graph (SRTrainer does), so that the packs are not part of the capture."""
        for i, mod in enumerate(self.features):
            if isinstance(mod, nn.Conv2d):
                w = mod.weight
                key = (w.data_ptr(), w._version, w.device)
                if self._packs.get(i, (None,))[0] != key:
                    self._packs[i] = (key, C.gconv_pack(w.detach(), None, False), C.gconv_pack(w.detach(), None, True))
        return self

    def _apply(self, fn, *a, **kw):
        self._packs = {}
        return super()._apply(fn, *a, **kw)

    # ------------------------------------------------------------------ forward
    def _check(self, x, y):
        for name, t in (("x", x), ("y", y)):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3 or t.dtype != torch.float32:
                raise ValueError("LPIPS: %s must be float32 [B, 3, H, W] in [-1, 1], got %s"
                                 % (name, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
        if x.shape != y.shape or x.device != y.device:
            raise ValueError("LPIPS: x %s on %s against y %s on %s" % (tuple(x.shape), x.device, tuple(y.shape), y.device))
        if x.shape[0] < 1 or x.shape[2] < MIN_SIDE or x.shape[3] < MIN_SIDE:
            raise ValueError("LPIPS: %d images of %d x %d: at least one image and %d pixels on a side (four poolings) expected"
                             % (x.shape[0], x.shape[2], x.shape[3], MIN_SIDE))

    def forward(self, x, y, per_layer=False):
        """d [B] float32 on the inputs' device; per_layer=True: (d, [5, B]).  The gradient reaches x only."""
        self._check(x, y)
        zx, zy = (x - self.shift) / self.scale, (y.detach() - self.shift) / self.scale
        if x.is_cuda:
            self.refresh()
            total, layers = _TailFn.apply(zx, zy, self)
        else:
            total, layers = self._forward_torch(zx, zy)
        return (total, layers) if per_layer else total

    @torch.no_grad()
    def taps(self, x, y):
        """The five tapped features of the pair, each [2 B, C, H, W] with x's samples first (diagnostics and tests)."""
        self._check(x, y)
        zx, zy = (x - self.shift) / self.scale, (y - self.shift) / self.scale
        if x.is_cuda:
            self.refresh()
            tensors, tape = self._walk(zx, zy, True)[2]
            return [tensors[src] for kind, _i, src, _dst in tape if kind == "tap"]
        z, feats = torch.cat([zx, zy]), []
        for i, mod in enumerate(self.features):
            z = mod(z)
            if i in TAPS:
                feats.append(z)
        return feats

    def _forward_torch(self, zx, zy):
        B = zx.shape[0]
        z, rows = torch.cat([zx, zy.detach()]), []
        lins = self.lins()
        for i, mod in enumerate(self.features):
            z = mod(z)
            if i in TAPS:
                f0, f1 = z[:B], z[B:].detach()
                n = []
                for f in (f0, f1):
                    s = (f * f).sum(1, keepdim=True)
                    pos = s > 0
                    n.append(torch.where(pos, f / (torch.sqrt(torch.where(pos, s, torch.ones_like(s))) + EPS), torch.zeros_like(f)))
                rows.append((lins[len(rows)] * (n[0] - n[1]) ** 2).sum(1).mean((1, 2)))
        layers = torch.stack(rows)
        return layers.sum(0), layers

    # ------------------------------------------------------------------ the walk on the device
    @torch.no_grad()
    def _walk(self, zx, zy, keep):
        """(total [B], per_layer [5, B], tape | None).  Tensors [2 B, C, H, W]: samples [0, B) of x, [B, 2 B) of y."""
        B = zx.shape[0]
        t = torch.cat([zx, zy]).contiguous()
        tensors, tape, partials, hws = [t], [], [], []
        lins = self.lins()
        ws = None
        for i, mod in enumerate(self.features):
            N, Cin, H, W = t.shape
            if isinstance(mod, nn.Conv2d):
                out = torch.empty(N, mod.out_channels, H, W, dtype=torch.float32, device=t.device)
                need = ops.gconv_ws_elems(N, mod.out_channels, H, W, Cin * 9)
                if need and (ws is None or ws.numel() < need):
                    ws = torch.empty(need, dtype=torch.float32, device=t.device)
                C.gconv(False, self._packs[i][1], t, 0, Cin, out, 0, 3, 3, 1, 1, 1, mod.bias.detach(), True, False, ws if need else None, None)
                tape.append(("conv", i, len(tensors) - 1, len(tensors)))
            elif isinstance(mod, nn.MaxPool2d):
                out = torch.empty(N, Cin, H // 2, W // 2, dtype=torch.float32, device=t.device)
                C.maxpool2s2(t, out, 0)
                tape.append(("pool", i, len(tensors) - 1, len(tensors)))
            else:                                   # the ReLU ran in the convolution's epilogue
                out = None
            if out is not None:
                t = out
                tensors.append(t if keep else None)   # without a tape a feature goes back to the allocator once its consumers are queued
            if i in TAPS:
                k = len(partials)
                partials.append(C.lpips_layer(t[:B], t[B:], lins[k].detach().reshape(-1).contiguous()))
                hws.append(t.shape[2] * t.shape[3])
                tape.append(("tap", k, len(tensors) - 1, None))
        layers, total = C.lpips_finish(partials, hws)
        return total, layers, ((tensors, tape) if keep else None)

    @torch.no_grad()
    def _walk_back(self, state, g_total, g_layers):
        """The tape in reverse over x's half of every tensor: d(sum_b g[b] d[b]) / d(zx)."""
        tensors, tape = state
        B = tensors[0].shape[0] // 2
        grads = [None] * len(tensors)
        lins = self.lins()
        ws = None

        def target(i):
            """(gradient buffer of x's half of tensor i, whether it holds a contribution, its ReLU mask)"""
            m = tensors[i][:B] if i != 0 else None
            if grads[i] is None:
                grads[i] = torch.empty_like(tensors[i][:B])
                return grads[i], False, m
            return grads[i], True, m

        for kind, i, src, dst in reversed(tape):
            if kind == "tap":
                g = g_total if g_layers is None else (g_layers[i] if g_total is None else g_total + g_layers[i])
                if g is None:
                    continue
                d, acc, m = target(src)
                f = tensors[src]
                C.lpips_layer_bwd(g.to(torch.float32).contiguous(), f[:B], f[B:], lins[i].detach().reshape(-1).contiguous(), d, acc, m)
                continue
            g = grads[dst]
            if g is None:
                continue
            d, acc, m = target(src)
            if kind == "pool":
                C.maxpool2s2_bwd(tensors[src][:B], g, 0, d, acc, m)
            else:
                mod = self.features[i]
                _, Cin, H, W = d.shape
                need = ops.gconv_ws_elems(B, Cin, H, W, mod.out_channels * 9)
                if need and (ws is None or ws.numel() < need):
                    ws = torch.empty(need, dtype=torch.float32, device=d.device)
                C.gconv(True, self._packs[i][2], g, 0, mod.out_channels, d, 0, 3, 3, 1, 1, 1, None, False, acc, ws if need else None, m)
            grads[dst] = None
        return grads[0]


class _TailFn(torch.autograd.Function):
    """(zx, zy) -> (d [B], per-layer [5, B]) through LPIPS._walk with its tape-driven backward: the gradient to zx only (the trunk is
    frozen, zy is the target)."""

    @staticmethod
    def forward(ctx, zx, zy, model):
        keep = ctx.needs_input_grad[0]
        ctx.set_materialize_grads(False)
        total, layers, state = model._walk(zx, zy, keep)
        ctx.model, ctx.state = model, state
        return total, layers

    @staticmethod
    def backward(ctx, g_total, g_layers):
        if ctx.state is None:
            return None, None, None
        state, ctx.state = ctx.state, None
        return ctx.model._walk_back(state, g_total, g_layers), None, None


def quantised(img):
    """The image a reader of the saved PNG holds, in [-1, 1]: float32 through `to_uint8`'s rule and back by u / 127.5 - 1 (uint8: the
    second half alone)."""
    if img.dtype != torch.uint8:
        img = C.to_uint8(img.detach().contiguous()) if img.is_cuda else \
            torch.clamp((img.detach() + 1.0) * 127.5, 0, 255).round().to(torch.uint8)
    return img.to(torch.float32) / 127.5 - 1.0


def as_model(lpips, device, what="evaluate: lpips"):
    """An LPIPS or the path of a saved one -> the module on `device`; anything else is a ValueError."""
    if isinstance(lpips, LPIPS):
        have, want = next(lpips.parameters()).device, torch.device(device)
        return lpips if have.type == want.type and want.index in (None, have.index) else lpips.to(want)
    if isinstance(lpips, (str, os.PathLike)):
        return LPIPS.load(lpips, device)
    raise ValueError("%s is an LPIPS module or the path of a saved one, got %r" % (what, lpips))


class PerceptualScores:
    """SRTrainer.evaluate's `lpips`: `add` per batch (one trunk walk over the pair, the rows stay on the device, no synchronisation),
    `result` once at the end.  Both images are scored as the saved PNGs would be (`quantised`); no border is shaved."""

    def __init__(self, model, device="cuda"):
        self.device = torch.device(device)
        self.model = as_model(model, self.device)
        self.total, self.layers = [], []

    @torch.no_grad()
    def add(self, sr, hr):
        """A batch of outputs and its ground truth, [B, 3, H, W] each (float32 in [-1, 1] or uint8), 16 pixels on a side at least."""
        total, layers = self.model(quantised(sr), quantised(hr), per_layer=True)
        self.total.append(total)
        self.layers.append(layers)

    def result(self):
        """{"fine": [N], "mean": their mean, "n": N, "per_layer": [5][N]}, float64 on the host.  Data parallel (call it once, on every
        rank): the rows are gathered in rank order."""
        if not self.total:
            raise ValueError("PerceptualScores.result: no batch was added")
        both = torch.cat([torch.cat(self.total)[:, None], torch.cat(self.layers, 1).t()], 1).to(torch.float64).cpu().numpy()   # [N, 1 + 5]
        rows, _ = gather_rows({"fine": both[:, 0], "per_layer": both[:, 1:]})
        fine = rows["fine"]
        return {"fine": fine, "mean": float(np.mean(fine)), "n": int(fine.shape[0]), "per_layer": np.ascontiguousarray(rows["per_layer"].T)}
