"""Shared by tests/test_cycle_mse_host.py and tests/test_hip_cycle_mse.py: the inputs of tests/golden/cycle_mse.npz as tensors, seeded
cases, and the fp64 model the kernels of tgsr_cycle_mse.hip are held to - F.interpolate(mode="bicubic") on doubles.  No test here;
nothing reads the reference."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

FIXTURE_CASES = ("down", "mixed", "up")


def u8_image(g, key, device="cpu"):
    """The fixture's uint8 codes k as the image x = k / 127.5 - 1 (exact in float32)."""
    return torch.from_numpy(np.asarray(g[key])).to(device).float() / 127.5 - 1.0


def fixture_inputs(g, name, device="cpu"):
    """(sr list, lr) of fixture case `name`."""
    n = sum(1 for k in g if k.startswith(name + ".sr"))
    return [u8_image(g, "%s.sr%d.u8" % (name, i), device) for i in range(n)], u8_image(g, name + ".lr.u8", device)


def cycle_mse_fp64(srs, lr):
    """CycleMSE in float64 on the float32 inputs: (loss, terms [n], [d_sr_i], d_lr) for a unit gradient, on the host."""
    s64 = [t.detach().double().cpu().requires_grad_(True) for t in srs]
    l64 = lr.detach().double().cpu().requires_grad_(True)
    terms = [((F.interpolate(s, size=[l64.shape[2], l64.shape[3]], mode="bicubic") - l64) ** 2).mean() for s in s64]
    loss = sum(terms)
    grads = torch.autograd.grad(loss, s64 + [l64])
    return loss.detach(), torch.stack(terms).detach(), list(grads[:-1]), grads[-1]


@functools.lru_cache(maxsize=None)
def seeded_case(sizes, lr_size, B=2, C=3):
    """Images of byte codes (x = k / 127.5 - 1) for SR sizes `sizes` = ((H, W), ...) and LR size `lr_size`, with their fp64 model:
    (srs, lr, (loss, terms, d_srs, d_lr)).  Computed once per shape and shared: treat as read-only."""
    g = torch.Generator().manual_seed(1000 * len(sizes) + 100 * sizes[0][0] + 10 * sizes[0][1] + lr_size[0] + B + C)
    img = lambda *s: torch.randint(0, 256, s, generator=g).float() / 127.5 - 1.0              # noqa: E731
    srs = [img(B, C, H, W) for H, W in sizes]
    lr = img(B, C, *lr_size)
    return srs, lr, cycle_mse_fp64(srs, lr)
