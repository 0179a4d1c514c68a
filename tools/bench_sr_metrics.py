#!/usr/bin/env python3
"""The image-quality kernels (tgsr::sr_metrics: PSNR / RMSE on RGB and Y + SSIM on Y, two launches) against the same scores
composed from torch operators on the device - quantise, Y as a matrix product, conv2d with the 11 x 11 window over the five
maps, all in fp64 where the kernels are - at B = 16 on 64^2 / 128^2 / 256^2 float images.  HIP events around regions of
`--calls` calls, the two forms alternated, median of `--regions` regions; the two forms' results are compared first (the SSEs
must be equal, the SSIM sums within 1e-9 per window).  Launch counts: the kernels' by construction, torch's from its profiler.
One JSON line, also written to profiles/sr_metrics_bench.json.
    python tools/bench_sr_metrics.py [--batch 16] [--calls 50] [--regions 9] [--out profiles/sr_metrics_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgsr_amd import custom_ops  # noqa: E402,F401

Y_COEF = [65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0]


def torch_rows(sr, hr, window):
    """[B, 3] float64 = (SSE RGB, SSE Y, SSIM sum) from torch operators (no shave)."""
    def u8(x):
        return torch.round(torch.clamp((x + 1.0) * 127.5, 0.0, 255.0))

    def y_of(u):                                       # [B, 3, H, W] byte values in fp32 -> Y byte values in fp64
        f = (u / 255.0).to(torch.float64)
        y = torch.einsum("bchw,c->bhw", f, torch.tensor(Y_COEF, dtype=torch.float64, device=u.device)) + 16 / 255.0
        return torch.floor(y * 255.0 + 0.5)
    a, b = u8(sr), u8(hr)
    ya, yb = y_of(a), y_of(b)
    sse = ((a - b).to(torch.float64) ** 2).sum((1, 2, 3))
    sse_y = ((ya - yb) ** 2).sum((1, 2))
    maps = torch.stack([ya, yb, ya * ya, yb * yb, ya * yb], 1)                      # [B, 5, H, W]
    B, _, H, W = maps.shape
    m = F.conv2d(maps.reshape(B * 5, 1, H, W), window).reshape(B, 5, H - 10, W - 10)
    mu_a, mu_b = m[:, 0], m[:, 1]
    va, vb, cab = m[:, 2] - mu_a * mu_a, m[:, 3] - mu_b * mu_b, m[:, 4] - mu_a * mu_b
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    ssim = ((2 * mu_a * mu_b + c1) * (2 * cab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (va + vb + c2))
    return torch.stack([sse, sse_y, ssim.sum((1, 2))], 1)


def gaussian_window(device):
    g = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) ** 2) / (2 * 1.5 ** 2))
    w = torch.outer(g, g)
    return (w / w.sum()).reshape(1, 1, 11, 11).to(device)


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:                                  # noqa: BLE001 - a count that could not be taken is reported as such
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sr_metrics: no GPU")
    dev = "cuda"
    window = gaussian_window(dev)
    res = {"bench": "sr_metrics", "batch": a.batch, "calls_per_region": a.calls, "regions": a.regions,
           "timing": "HIP events around regions of back-to-back calls, forms alternated, median region", "sizes": {}}
    for size in (64, 128, 256):
        g = torch.Generator().manual_seed(size)
        hr = (torch.rand(a.batch, 3, size, size, generator=g) * 2 - 1).to(dev)
        sr = (hr + 0.1 * torch.randn(a.batch, 3, size, size, generator=g).to(dev)).contiguous()
        forms = {"hip": lambda: torch.ops.tgsr.sr_metrics(sr, hr, 0), "torch": lambda: torch_rows(sr, hr, window)}
        got, want = forms["hip"](), forms["torch"]()
        torch.cuda.synchronize()
        windows = (size - 10) ** 2
        # the torch form is a baseline, not the pinned definition: its Y is a GEMM (another summation order, fused multiply-adds),
        # so a Y byte may differ on a rare triple - the RGB sums must be equal, the Y-based figures close
        assert torch.equal(got[:, 0], want[:, 0]), "the two forms disagree on the RGB sums of squared differences"
        sse_y_dev = float(((got[:, 1] - want[:, 1]).abs() / want[:, 1].clamp_min(1)).max())
        ssim_dev = float(((got[:, 2] - want[:, 2]).abs() / windows).max())
        assert sse_y_dev <= 1e-4 and ssim_dev <= 1e-6, (sse_y_dev, ssim_dev)
        for f in forms.values():                        # warm both
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(a.regions):
            for k, f in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    f()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.calls)
        entry = {"ssim_max_dev_per_window": ssim_dev, "sse_y_max_rel_dev": sse_y_dev}
        for k in forms:
            entry[k] = {"ms_per_call_median": round(statistics.median(ms[k]), 4), "ms_per_call_min": round(min(ms[k]), 4),
                        "ms_per_call_max": round(max(ms[k]), 4),
                        "launches": 2 if k == "hip" else count_launches(forms[k])}
        entry["torch_over_hip"] = round(entry["torch"]["ms_per_call_median"] / entry["hip"]["ms_per_call_median"], 2)
        res["sizes"][str(size)] = entry
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
