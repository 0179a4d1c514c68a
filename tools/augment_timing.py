#!/usr/bin/env python3
"""Times one DeviceAugment call (tgsr_augment_u8: one coefficient launch + one image launch over the windows) against the
same bytes composed from the operations that existed before it: per image a crop to planar, ops.resize_bilinear_u8 over
the whole resized image (two launches), a slice and a flip.

    python tools/augment_timing.py [--batch 16] [--imsize 256] [--out profiles/augment_timing.json]

Sixteen 375 x 500 sources with CUB-like bounding boxes, Resize(304) + RandomCrop(256) + flip.  Warm, fenced: every region is
`--calls` calls between two device events behind a synchronise; the figure is the median over `--regions` regions, the two
forms alternating region by region in one process.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgsr_amd import _lib, ops  # noqa: E402
from tgsr_amd.datasets import DeviceAugment, GpuImagePyramid, RaggedImages  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--imsize", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "augment_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_timing.py measures on a GPU; none found")
    B, S, H, W = a.batch, a.imsize, 375, 500
    g = np.random.default_rng(0)
    srcs = [g.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    bboxes = [(int(g.integers(40, 160)), int(g.integers(20, 90)), int(g.integers(180, 330)), int(g.integers(150, 260))) for _ in range(B)]
    aug = DeviceAugment(S, device="cuda")
    batch = RaggedImages.pack(srcs)
    plan = aug.plan(batch, bboxes, generator=torch.Generator().manual_seed(1))
    pyr = GpuImagePyramid((S,), device="cuda")
    out_u = torch.empty(B, 3, S, S, dtype=torch.uint8, device="cuda")
    launches = {"fused": 2, "unfused": 0}

    def fused():
        return aug(batch, plan)

    def unfused(count=False):
        n = 0
        for b, (off, h, w, x1, y1, x2, y2, oh, ow, top, left, flip) in enumerate(plan.tolist()):
            x = batch.data[off:off + 3 * h * w].view(h, w, 3)[y1:y2, x1:x2].permute(2, 0, 1).contiguous()
            r = pyr.resize(x, oh, ow)
            win = r[:, top:top + S, left:left + S]
            out_u[b].copy_(win.flip(-1) if flip else win)
            n += 1 + (ow != x2 - x1) + (oh != y2 - y1) + (2 if flip else 1)
        if count:
            launches["unfused"] = n
        return out_u

    # the two launches alone: table already on the device, workspace and output allocated once, no host-side checks
    L = _lib.lib()
    tdev = plan.to("cuda")
    ws = torch.empty(L.tgsr_augment_ws_elems(B, S), dtype=torch.int32, device="cuda")
    out_k = torch.empty(B, 3, S, S, dtype=torch.uint8, device="cuda")

    def kernels():
        _lib.check(L.tgsr_augment_u8(ops._p(batch.data), batch.nbytes, ops._p(plan), ops._p(tdev), B, S, ops._p(ws), ops._p(out_k),
                                     ops._stream()), "tgsr_augment_u8")
        return out_k

    ref = unfused(count=True).clone()
    same = torch.equal(fused(), ref) and torch.equal(kernels(), ref)
    forms = {"fused": fused, "unfused": unfused, "kernels": kernels}
    for f in forms.values():                                   # warm: code objects, allocator, the pyramid's tap tables
        for _ in range(5):
            f()
    times = {k: [] for k in forms}
    for _ in range(a.regions):
        for k, f in forms.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    res = {"what": "one DeviceAugment call vs the same bytes from per-image resize_bilinear_u8 + slice + flip",
           "device": torch.cuda.get_device_name(0), "batch": B, "imsize": S, "source": [H, W], "resize_to": aug.size,
           "calls_per_region": a.calls, "regions": a.regions, "outputs_equal": bool(same),
           "fused_us_median": float(np.median(times["fused"])), "fused_us_min": float(np.min(times["fused"])),
           "unfused_us_median": float(np.median(times["unfused"])), "unfused_us_min": float(np.min(times["unfused"])),
           "fused_two_launches_alone_us_median": float(np.median(times["kernels"])),
           "fused_two_launches_alone_us_min": float(np.min(times["kernels"])),
           "fused_launches": launches["fused"], "fused_copies": 1, "unfused_launches": launches["unfused"],
           "note": "fused / unfused are whole calls as a loader makes them (descriptor checks, table upload, allocations, launches): "
                   "host-inclusive where the host cost exceeds the device work; the two launches alone are the C entry on a table "
                   "that is already on the device"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if not same:
        sys.exit("the two forms differ")


if __name__ == "__main__":
    main()
