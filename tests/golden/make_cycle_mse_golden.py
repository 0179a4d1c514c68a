#!/usr/bin/env python3
"""Generate tests/golden/cycle_mse.npz: the reference's CycleMSE (miscc/losses.py:785-790) on seeded inputs (CPU, build container
only).

TEST INFRASTRUCTURE like make_golden.py, whose stubs (`_load_ref`) it uses: the reference is imported and its `CycleMSE` is
called; nothing of the reference is copied.  Stored per case: the SR images and the LR image as the uint8 codes k of
x = k / 127.5 - 1 (exact in float32), the loss, the per-scale terms (the function called on one scale at a time) and the
gradients with respect to every SR image and the LR image.  B = 2, C = 3; sizes are SR -> LR:

  down.*   12x16, 24x32, 48x64 -> 6x8: ratios 2 / 4 / 8, a training pyramid in small (clamped borders on every side);
  mixed.*  10x14, 23x17, 8x20, 4x5, 12x15 -> 4x5: non-integer ratios, 2 down and 4 across, the identity, ratio 3 (a single tap);
  up.*     3x4, 1x1, 2x2 -> 7x9: up-scaling, where several or all four taps of an axis collapse onto one pixel.

    python tests/golden/make_cycle_mse_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402

CASES = {
    "down": ([(12, 16), (24, 32), (48, 64)], (6, 8)),
    "mixed": ([(10, 14), (23, 17), (8, 20), (4, 5), (12, 15)], (4, 5)),
    "up": ([(3, 4), (1, 1), (2, 2)], (7, 9)),
}


def _img(gen, *shape):
    k = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    return k, k.float() / 127.5 - 1.0


def _case(losses, out, name, gen, sizes, lr_size, B=2, C=3):
    srs = []
    for i, (H, W) in enumerate(sizes):
        k, x = _img(gen, B, C, H, W)
        out["%s.sr%d.u8" % (name, i)] = G._np(k)
        srs.append(x.requires_grad_(True))
    k, lr = _img(gen, B, C, *lr_size)
    out[name + ".lr.u8"] = G._np(k)
    lr.requires_grad_(True)
    loss = losses.CycleMSE(srs, lr)
    grads = torch.autograd.grad(loss, srs + [lr])
    out[name + ".loss"] = G._np(loss)
    out[name + ".terms"] = np.array([float(losses.CycleMSE([s.detach()], lr.detach())) for s in srs], np.float32)
    for i, g in enumerate(grads[:-1]):
        out["%s.g_sr%d" % (name, i)] = G._np(g)
    out[name + ".g_lr"] = G._np(grads[-1])
    print("%s: loss %.7g, terms %s" % (name, float(loss.detach()), out[name + ".terms"].tolist()))


def main():
    _cfg, _GA, _util, _model, losses = G._load_ref(ngf=32, nef=32)
    out = {}
    gen = torch.Generator().manual_seed(2026)
    torch.manual_seed(2026)
    for name, (sizes, lr_size) in CASES.items():
        _case(losses, out, name, gen, sizes, lr_size)
    path = os.path.join(G.OUT, "cycle_mse.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d KB)" % (path, len(out), os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
