#!/usr/bin/env python3
"""Times `SRPipeline.upscale` (whole images by overlapping tiles: tile_gather -> the pipeline's own __call__ per tile batch ->
tile_stitch) on the shipped face weights, fp32, for LR images of 256 x 256 and 192 x 328:

    python tools/upscale_timing.py [--out profiles/upscale_timing.json]

per image and form - tile 64 and tile 128 (both keep every layer on whole Winograd workgroup tiles), eager and with the tile-batch
step captured (graph=True), and the whole image in ONE __call__ where that runs - ms per image, peak allocated memory, the share of
the gather and stitch launches (timed alone over the image's batches, on resident tile outputs), and whether every form's images
are within the project's one fp32 tolerance (atol = rtol = 2e-4, tests/conftest.py) of the CPU fp32 oracle's run over the WHOLE
image - the reference that tolerance is stated against; the largest distance between two forms is recorded beside it (two correct
fp32 evaluations on different kernel forms may each use most of the tolerance in opposite directions at a few ill-conditioned
pixels of NetG_highweight's 128^2 section).  Tiles recompute (tile / (tile - 32))^2 of the
work at halo 16.  Warm, fenced: a region is `--calls` images between two device events behind a synchronise; the figure is the
median over `--regions` regions, the forms alternating region by region in one process.  Inputs are uniform noise (a smooth input
makes the shipped NetG_highweight ill-conditioned: two correct fp32 evaluations then differ by more than the tolerance).
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import tgsr_oracle as O  # noqa: E402
from tgsr_amd import custom_ops as C  # noqa: E402
from tgsr_amd import tiles as T  # noqa: E402
from tgsr_amd._lib import TgsrError  # noqa: E402
from tgsr_amd.miscc.config import cfg, cfg_reset  # noqa: E402
from tgsr_amd.trainer import SRPipeline  # noqa: E402

TOL = 2e-4


def load_pipeline():
    z = np.load(os.path.join(ROOT, "tests", "golden", "face_S8_weights.npz"))

    def sd(prefix):
        return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix) and z[k].dtype.kind in "fiub"}
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM, cfg.TREE.BRANCH_NUM = 32, 256, 4
    sds = (sd("E."), sd("GL."), sd("GH."))
    return SRPipeline(41, device="cuda", low="lr").load_state_dicts(*sds), sds


def tol_used(a, b):
    """(largest |a - b| / (atol + rtol |b|) over the values: <= 1 is within the tolerance; how many values are above it)."""
    r = (a - b).abs() / (TOL + TOL * b.abs())
    return float(r.max()), int((r > 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "upscale_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("upscale_timing.py measures on a GPU; none found")
    pipe, sds = load_pipeline()
    halo = T.receptive_halo(pipe.netGL, pipe.netGH)
    g = torch.Generator().manual_seed(100)
    cap = torch.zeros(18, dtype=torch.int64)
    cap[:9] = torch.randint(1, 41, (9,), generator=g)
    cap = cap.cuda()
    images, all_equal = [], True
    for H, W in ((256, 256), (192, 328)):
        lr = (torch.rand(3, H, W, generator=g) * 2 - 1).cuda()
        forms = {}
        for tile, tb in ((64, 4), (128, 4)):
            for graph in (False, True):
                forms["tile%d_batch%d%s" % (tile, tb, "_graph" if graph else "")] = (
                    lambda tile=tile, tb=tb, graph=graph: pipe.upscale(lr, cap, 9, tile=tile, tile_batch=tb, graph=graph))

        def whole():
            o = pipe(cap[None], [9], lr[None], lr[None])
            return {"fine": [t[0] for t in o["fine"]], "fake": [t[0] for t in o["fake"]]}
        forms["whole_image_one_call"] = whole

        def ends(tile, tb):          # the gather and stitch launches of one image alone, on resident tile outputs
            th, tw = min(tile, H), min(tile, W)
            table = T.plan_tiles(H, W, (th, tw), halo)
            table = torch.cat([table, table[-1:].expand((-len(table)) % tb, -1)]).contiguous()
            tdev = table.cuda()
            tiles = [torch.zeros(tb, 3, s * th, s * tw, device="cuda") for s in (2, 4, 8)] * 2
            outs = [torch.empty(3, s * H, s * W, device="cuda") for s in (2, 4, 8)] * 2

            def run():
                for b in range(0, len(table), tb):
                    C.tile_gather(lr, None, table[b:b + tb], tdev[b:b + tb], th, tw)
                    C.tile_stitch(tiles, outs, table[b:b + tb], tdev[b:b + tb], H, W, th, tw)
            return run, len(table) // tb
        with torch.no_grad():                                      # the CPU fp32 oracle over the whole image, once
            o = O.sr_forward(*sds, cap[None].cpu(), [9], lr[None].cpu(), lr[None].cpu())
        ref = {k: [t[0].cuda() for t in o[k]] for k in ("fine", "fake")}
        del o
        res, first, skipped, between = {}, None, {}, 0.0
        for name, f in list(forms.items()):
            try:                                                   # warm: code objects, weight packs, allocator, the capture
                for _ in range(2):
                    out = f()
                torch.cuda.synchronize()
            except (ValueError, TgsrError) as e:                   # a shape refusal: that form is reported, not timed
                skipped[name] = "%s: %s" % (type(e).__name__, str(e)[:200])
                del forms[name]
                continue
            used = [tol_used(out[k][i], ref[k][i]) for k in ("fine", "fake") for i in range(3)]
            res[name] = {"outputs_equal_within_tol": max(u for u, _ in used) <= 1.0,
                         "tolerance_used_vs_oracle": max(u for u, _ in used), "values_over_tolerance": sum(n for _, n in used)}
            all_equal = all_equal and res[name]["outputs_equal_within_tol"]
            if first is None:
                first = {k: [t.clone() for t in out[k]] for k in ("fine", "fake")}
            res[name]["tolerance_used_vs_first_form"] = max(tol_used(out[k][i], first[k][i])[0] for k in ("fine", "fake") for i in range(3))
            between = max(between, res[name]["tolerance_used_vs_first_form"])
            del out
        del ref, first
        end_forms = {}
        for tile, tb in ((64, 4), (128, 4)):
            run, nb = ends(tile, tb)
            for _ in range(2):
                run()
            end_forms["tile%d_batch%d" % (tile, tb)] = (run, nb)
        times = {k: [] for k in list(forms) + ["ends_" + k for k in end_forms]}
        peak = {}
        timed = dict(forms)
        timed.update({"ends_" + k: v[0] for k, v in end_forms.items()})
        for _ in range(a.regions):
            for k, f in timed.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.calls)
                peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated() - base)
        for k in forms:
            res[k].update({"ms_per_image_median": float(np.median(times[k])), "ms_per_image_min": float(np.min(times[k])),
                           "peak_allocated_MiB_above_resident": round(peak[k] / 2 ** 20, 1)})
            base = k.replace("_graph", "")
            if base in end_forms:
                e = float(np.median(times["ends_" + base]))
                nb = end_forms[base][1]
                tile = int(base[4:base.index("_")])
                res[k].update({"tile_batches": nb, "gather_stitch_launches": 2 * nb, "gather_stitch_ms_median": e,
                               "gather_stitch_share": e / res[k]["ms_per_image_median"],
                               "recompute_factor": (tile / (tile - 2.0 * halo)) ** 2})
        images.append({"lr": [H, W], "forms": res, "not_run": skipped, "largest_tolerance_used_between_two_forms": between})
    best = {}
    for im in images:
        for tile in (64, 128):
            ks = [k for k in im["forms"] if k.startswith("tile%d_" % tile)]
            best.setdefault(tile, []).append(min(im["forms"][k]["ms_per_image_median"] for k in ks))
    favoured = min(best, key=lambda t: sum(best[t]))
    out = {"what": "SRPipeline.upscale (tiles) vs the whole image in one __call__, fp32, shipped face weights, one caption of 9 words",
           "device": torch.cuda.get_device_name(0), "halo": halo, "calls_per_region": a.calls, "regions": a.regions,
           "tolerance": TOL, "reference": "oracle.tgsr_oracle.sr_forward (CPU fp32) over the whole image",
           "outputs_equal_within_tol": bool(all_equal), "images": images,
           "favoured_tile": int(favoured), "default_tile": int(T.DEFAULT_TILE),
           "verdict_over": "every form measured: upscale at tile 64 and 128 with the default tile_batch of 4, eager and graph=True, and "
                           "the whole image in one __call__",
           "note": "ms are whole calls as a caller makes them (planning, table upload, allocations of the outputs, launches), host-"
                   "inclusive where the host cost exceeds the device work; peak memory is above what was allocated before the region "
                   "(weights, packs, captured graphs' static buffers and, for the graph forms, their pools are resident)"}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not all_equal:
        sys.exit("a form is further than the tolerance from the oracle")


if __name__ == "__main__":
    main()
