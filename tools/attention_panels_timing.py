#!/usr/bin/env python3
"""Time of the attention panels at the shipped shape (B = 16 images, T = 18 words, 32 x 32 maps -> 256 x 256 tiles): the new
operator (tgsr::attn_panels: two launches, the expand + blur as two fp64 MFMA products per map) against the same arithmetic from
torch device operators - threshold, F.interpolate, two fp64 blurs of 161 taps, min / max stretch, the integer blend, the panel
assembled by slices: what a user of the library could write before the operator existed - and against the scipy model on the CPU
(zoom + gaussian_filter per word, one channel, the 16 images one after the other).  The torch form is timed twice: with the blur
as F.conv1d, the obvious spelling, for which torch has no fast fp64 path on the device (seconds per call), and with the same taps
as one banded matrix product per axis, what a user who noticed would write.

    python tools/attention_panels_timing.py [--out profiles/attention_panels_timing.json] [--rounds 7] [--calls 5]

Each device figure is the median over `rounds` fenced regions (device events around `calls` back-to-back calls, a synchronise
behind them) of the time per call; the device forms alternate round by round, so that whatever else the machine does falls on
all of them (the conv1d form: three regions of one call).  The torch form is a stand-in for the cost, not for the bytes: F.interpolate clamps at the border where the definition
mirrors, F.pad's 'reflect' does not repeat the edge sample - how far its map bytes are from the operator's is recorded, not asserted.
No threshold is fixed in advance.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgsr_amd import attnviz  # noqa: E402

B, T, A, U, ALPHA, SIGMA, RADIUS = 16, 18, 32, 8, 180, 20.0, 80
V = A * U


def fenced(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def blur_rows(y, taps):
    """The 161-tap blur along the last axis of y [N, 1, V] fp64: conv1d where `taps` is the [1, 1, 161] filter, the same taps as
    one matrix product where it is the banded [V + 160, V] matrix (torch's fp64 conv1d has no fast path on the device: both are
    timed, the product is the form a user who noticed would write)."""
    y = F.pad(y, (RADIUS, RADIUS), mode="reflect")
    if taps.dim() == 3:
        return F.conv1d(y, taps)
    return y.reshape(-1, V + 2 * RADIUS) @ taps


def band_of(taps):
    band = torch.zeros(V + 2 * RADIUS, V, dtype=torch.float64, device=taps.device)
    for c in range(V):
        band[c:c + 2 * RADIUS + 1, c] = taps.reshape(-1)
    return band


def torch_form(img, att, taps):
    """(panel, map bytes) from torch device operators; every caption has T words here."""
    x = att.double()
    thresh = 2.0 / T
    x = x * (x > thresh)
    y = F.interpolate(x, scale_factor=U, mode="bilinear", align_corners=False)                 # [B, T, V, V] fp64
    y = blur_rows(y.reshape(B * T * V, 1, V), taps).reshape(B, T, V, V)
    y = blur_rows(y.transpose(2, 3).reshape(B * T * V, 1, V), taps).reshape(B, T, V, V).transpose(2, 3)
    mn, mx = y.amin(dim=(2, 3), keepdim=True), y.amax(dim=(2, 3), keepdim=True)
    m = ((y - mn) / (mx - mn) * 255.0).to(torch.uint8)
    i = img.add(1).div(2).mul(255).round().clamp(0, 255).to(torch.int32)                       # [B, 3, V, V]
    t = m.to(torch.int32)[:, :, None] * ALPHA + i[:, None] * (255 - ALPHA) + 128               # [B, T, 3, V, V]
    t = (((t >> 8) + t) >> 8).to(torch.uint8)
    panel = torch.zeros(B, V, T, V + 2, 3, dtype=torch.uint8, device=img.device)
    panel[:, :, :, :V] = t.permute(0, 3, 1, 4, 2)
    return panel.reshape(B, V, T * (V + 2), 3), m


def scipy_model(att):
    import scipy.ndimage as ndi
    out = np.empty((att.shape[0], T, V, V), dtype=np.uint8)
    thresh = 2.0 / T
    for b in range(att.shape[0]):
        for j in range(T):
            x = att[b, j].astype(np.float64)
            y = ndi.gaussian_filter(ndi.zoom(x * (x > thresh), U, order=1, mode='mirror', grid_mode=True), SIGMA, mode='reflect',
                                    truncate=4.0)
            out[b, j] = ((y - y.min()) / (y.max() - y.min()) * 255.0).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "attention_panels_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_panels_timing needs the GPU")
    g = torch.Generator().manual_seed(0)
    att = torch.softmax(3.0 * torch.randn(B, T, A, A, generator=g), dim=1)
    img = torch.tanh(torch.randn(B, 3, V, V, generator=g))
    att_d, img_d = att.cuda(), img.cuda()
    lens = [T] * B
    k = torch.arange(-RADIUS, RADIUS + 1, dtype=torch.float64)
    taps = torch.exp(-0.5 / (SIGMA * SIGMA) * k * k)
    taps = (taps / taps.sum()).reshape(1, 1, -1).cuda()
    band = band_of(taps)
    runs = {
        "attn_panels_op": lambda: attnviz.attention_panels(img_d, att_d, lens, with_maps=True),
        "torch_device_ops_matmul": lambda: torch_form(img_d, att_d, band),
        "torch_device_ops_conv1d": lambda: torch_form(img_d, att_d, taps),
    }
    slow = "torch_device_ops_conv1d"                                   # seconds per call: one call per region, three regions
    new = runs["attn_panels_op"]()
    old_panel, old_maps = runs["torch_device_ops_matmul"]()
    same_torch = bool(torch.equal(old_panel, runs[slow]()[0]))
    t0 = time.perf_counter()
    model = scipy_model(att.numpy())
    cpu_s = time.perf_counter() - t0
    d_model = (new["maps"].cpu().numpy().astype(np.int32) - model.astype(np.int32))
    d_torch = (new["maps"].to(torch.int32) - old_maps.to(torch.int32)).abs()
    for name, fn in runs.items():
        if name != slow:
            fenced(fn, 2)
    times = {name: [] for name in runs}
    for r in range(args.rounds):
        for name, fn in runs.items():
            if name != slow:
                times[name].append(fenced(fn, args.calls))
            elif r < 3:
                times[name].append(fenced(fn, 1))
    res = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"B": B, "T": T, "map": [A, A], "u": U, "tile": [V, V], "panel": list(new["panel"].shape), "alpha": ALPHA},
        "method": "median of %d fenced regions of %d calls each, the device forms alternating (the conv1d form: 3 regions of one "
                  "call); us per call of the whole batch; the CPU figure is one run of the scipy model over the %d images, one "
                  "channel, wall clock" % (args.rounds, args.calls, B),
        "times": {name: stats(v) for name, v in times.items()},
        "torch_forms_give_the_same_panel": same_torch,
        "scipy_cpu_model_us": round(cpu_s * 1e6, 1),
        "map_bytes_op_vs_scipy_model": {"bytes": int(d_model.size), "differing": int((d_model != 0).sum()),
                                        "largest_difference": int(np.abs(d_model).max())},
        "map_bytes_op_vs_torch_form": {"differing": int((d_torch != 0).sum()), "largest_difference": int(d_torch.max()),
                                       "note": "the torch form clamps / reflects differently at the borders: a stand-in for the cost"},
    }
    op = res["times"]["attn_panels_op"]["median_us"]
    res["speedup_vs_torch_device_ops_matmul"] = round(res["times"]["torch_device_ops_matmul"]["median_us"] / op, 2)
    res["speedup_vs_torch_device_ops_conv1d"] = round(res["times"][slow]["median_us"] / op, 1)
    res["speedup_vs_scipy_cpu_model"] = round(res["scipy_cpu_model_us"] / op, 1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
