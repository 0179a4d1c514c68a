"""Shared by tests/test_attn_losses_host.py and tests/test_hip_attn_losses.py: the inputs of tests/golden/attn_losses.npz as tensors
and the fp64 models the kernels of tgsr_attn_losses.hip are held to.  No test here; nothing reads the reference."""
import numpy as np
import torch
import torch.nn.functional as F


def u8_image(g, key, device="cpu"):
    """The fixture's uint8 codes k as the image x = k / 127.5 - 1 (exact in float32)."""
    return torch.from_numpy(np.asarray(g[key])).to(device).float() / 127.5 - 1.0


def wmse_inputs(g, name, device="cpu"):
    """(fake, label, att) lists of case `name` ("wmse": three scales at r = 2; "wmse1": one at r = 1)."""
    n = sum(1 for k in g if k.startswith(name + ".att"))
    return ([u8_image(g, "%s.fake%d.u8" % (name, i), device) for i in range(n)],
            [u8_image(g, "%s.label%d.u8" % (name, i), device) for i in range(n)],
            [torch.from_numpy(np.asarray(g["%s.att%d" % (name, i)])).to(device) for i in range(n)])


def weight_mse_fp64(fake, label, att):
    """One scale of weight_MSE in float64 on the float32 inputs: (term, d_fake, d_att, argmax [B, h, w], wups float32)."""
    f, l, a = (t.detach().double().cpu().requires_grad_(True) for t in (fake, label, att))
    w, idx = a.max(dim=1, keepdim=True)
    wups = F.interpolate(w, size=f.shape[2:])
    term = ((a.shape[1] * wups) * (f - l).pow(2)).sum() / f.numel()
    gf, ga = torch.autograd.grad(term, [f, a])
    return term.detach(), gf, ga, idx[:, 0], wups.detach().float()


def confidence_fp64(att, lens):
    """conf [B, T] in numpy: the comparison in float32 against float32(2 * (2 / n)), the sum in float64; zero rows for a length
    outside [1, T]."""
    a = np.asarray(att, dtype=np.float32).reshape(att.shape[0], att.shape[1], -1)
    out = np.zeros(a.shape[:2], dtype=np.float64)
    for b, n in enumerate(lens):
        if not 1 <= n <= a.shape[1]:
            continue
        thr = np.float32(2. * (2. / float(n)))
        for t in range(n):
            m = a[b, t]
            out[b, t] = m[m > thr].astype(np.float64).sum()
    return out


def confidence_maps(B, T, Q, lens, seed):
    """Softmaxed maps [B, T, Q] with, in every counted row, one value EQUAL to float32(4 / n) (must not count) and one at the next
    float32 above it (must count)."""
    g = torch.Generator().manual_seed(seed)
    att = torch.softmax(6.0 * torch.randn(B, T, Q, generator=g), dim=1).numpy().copy()
    for b, n in enumerate(lens):
        if not 1 <= n <= T:
            continue
        thr = np.float32(2. * (2. / float(n)))
        for t in range(n):
            att[b, t, (7 * t + 3) % Q] = thr
            att[b, t, (11 * t + 5 + Q // 2) % Q] = np.nextafter(thr, np.float32(np.inf))
    return att
