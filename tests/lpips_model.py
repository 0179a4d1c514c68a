"""A model of LPIPS v0.1 (net='vgg', spatial=False) for the tests, written from the definition and independently of tgsr_amd/lpips.py:
torch operators in the dtype asked for (float64 = the reference; float32 = the yardstick of what a plain evaluation loses).

  s(x) = (x - shift) / scale;  features[0:30] of VGG16 (tests/vgg16_arch.py);  taps after ReLU 1_2, 2_2, 3_3, 4_3, 5_3
  n(f) = f / (sqrt(sum_c f^2) + 1e-10);  d_l[b] = mean_p sum_c w_l[c] (n(f0) - n(f1))^2;  d[b] = sum_l d_l[b]
  gradient w.r.t. f0 (and so x): 0 from a pixel whose f0 column is all zero (autograd's sqrt'(0) would give NaN): the declared rule.
"""
import torch
import torch.nn.functional as F

import vgg16_arch as A

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10


def unit(f, rule=True):
    """f [B, C, ...] -> n(f) over dim 1; with `rule` no gradient flows from a zero column."""
    s = (f * f).sum(1, keepdim=True)
    if not rule:
        return f / (torch.sqrt(s) + EPS)
    pos = s > 0
    r = torch.sqrt(torch.where(pos, s, torch.ones_like(s)))
    return torch.where(pos, f / (r + EPS), torch.zeros_like(f))


def tail(f0, f1, w):
    """d_l [B] of one tap: f0, f1 [B, C, H, W], w [C] (any dtype; computed in it)."""
    d = (w.view(1, -1, 1, 1) * (unit(f0) - unit(f1)) ** 2).sum(1)
    return d.mean((1, 2))


def tail64(f0, f1, w, g=None):
    """(d_l float64 [B], d(sum_b g[b] d_l[b]) / d(f0) float64) of float inputs widened to float64."""
    f0 = f0.detach().cpu().to(torch.float64).requires_grad_(True)
    f1, w = f1.detach().cpu().to(torch.float64), w.detach().cpu().to(torch.float64)
    d = tail(f0, f1, w)
    g = torch.ones_like(d) if g is None else g.detach().cpu().to(torch.float64)
    (grad,) = torch.autograd.grad((d * g).sum(), f0)
    return d.detach(), grad


def trunk(sd, z, dtype):
    """The five tapped features of the scaled images z under the state dict `sd` (torchvision's names)."""
    feats = []
    for i, kind, _cin, _cout in A.layers():
        if kind == "conv":
            z = F.conv2d(z, sd["features.%d.weight" % i].to(dtype), sd["features.%d.bias" % i].to(dtype), padding=1)
        elif kind == "relu":
            z = F.relu(z)
        else:
            z = F.max_pool2d(z, 2)
        if i in A.LPIPS_TAPS:
            feats.append(z)
    return feats


def distance(sd, x, y, dtype=torch.float64, grad=False):
    """{"d": [B], "per_layer": [5, B], "feats": five [2 B, C, H, W] (x's rows first), "grad": d(sum_b d[b]) / d(x) | None} in `dtype`
    on the CPU."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    x = x.detach().cpu().to(dtype).requires_grad_(grad)
    y = y.detach().cpu().to(dtype)
    shift, scale = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (SHIFT, SCALE))
    B = x.shape[0]
    with torch.enable_grad() if grad else torch.no_grad():
        feats = trunk(sd, torch.cat([(x - shift) / scale, (y - shift) / scale]), dtype)
        rows = [tail(f[:B], f[B:].detach(), sd["lin%d" % k].to(dtype).reshape(-1)) for k, f in enumerate(feats)]
        per_layer = torch.stack(rows)
        d = per_layer.sum(0)
        gx = torch.autograd.grad(d.sum(), x)[0] if grad else None
    return {"d": d.detach(), "per_layer": per_layer.detach(), "feats": [f.detach() for f in feats], "grad": gx}
