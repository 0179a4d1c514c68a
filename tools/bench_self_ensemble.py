#!/usr/bin/env python3
"""Times the geometric self-ensemble (x8: ops.d8_gather / ops.d8_merge, SRPipeline.upscale(ensemble=8)) against the same result
built from torch device operators, on the shipped face weights, fp32:

    python tools/bench_self_ensemble.py [--out profiles/self_ensemble_timing.json] [--only a|b]

  (a) the two ends alone, for ONE 128 x 128 window: the gather launch (LR and blurred LR -> the 8-row variant batch) and the merge
      launch over the nine outputs of that batch (fine and fake at x2, x4, x8 with 3 channels, the attention maps at x1, x2, x4 with
      9), on resident tensors - against the composition a user writes today: torch.flip / transpose / stack for the batch, the
      inverse flips and transposes, stack and mean(0) per output.  The merge's bytes are counted from the shapes, eight reads and
      one write per output value; its rate is stated against the HBM figures of the MI355X (8.0 TB/s specified, 6.29 TB/s measured
      with a float4 copy).
  (b) upscale(ensemble=8) of a 256 x 256 LR image (tile 128, tile_batch 4, eager and graph=True) against eight upscale calls on the
      torch variants, each result mapped back, stacked and averaged - the same tree, the same pipeline.

Results first: the kernels' mean equals the ordered torch sum ((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125 bit for
bit, and is within float32 rounding of torch's mean(0).  Warm, fenced: a region is `calls` calls between two device events behind
a synchronise; a figure is the median over `regions` regions, minimum and maximum beside it, the forms alternating region by
region in one process.  No ratio is fixed in advance.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgsr_amd import custom_ops as C  # noqa: E402
from tgsr_amd.miscc.config import cfg, cfg_reset  # noqa: E402
from tgsr_amd.trainer import SRPipeline  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12          # bytes / s: the specified peak, a measured float4 copy
WIN, WORDS = 128, 9
OUTPUTS = [(3, 2), (3, 4), (3, 8)] * 2 + [(WORDS, 1), (WORDS, 2), (WORDS, 4)]      # (channels, scale): fine, fake, att


def variant(x, k):
    """Variant k of x [..., h, w] from torch operators: transpose first, then the mirrors."""
    x = x.transpose(-1, -2) if k & 4 else x
    x = torch.flip(x, [-2]) if k & 2 else x
    return torch.flip(x, [-1]) if k & 1 else x


def back(x, k):
    x = torch.flip(x, [-1]) if k & 1 else x
    x = torch.flip(x, [-2]) if k & 2 else x
    return x.transpose(-1, -2) if k & 4 else x


def fenced(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def stats(us, unit="us", scale=1.0):
    return {"median_" + unit: round(statistics.median(us) * scale, 3), "min_" + unit: round(min(us) * scale, 3),
            "max_" + unit: round(max(us) * scale, 3)}


def timed(forms, regions, calls):
    for fn in forms.values():
        fenced(fn, 2)
    times = {k: [] for k in forms}
    for _ in range(regions):
        for k, fn in forms.items():
            times[k].append(fenced(fn, calls))
    return times


def part_a(regions, calls):
    g = torch.Generator().manual_seed(0)
    lr = (torch.rand(1, 3, WIN, WIN, generator=g) * 2 - 1).cuda()
    lrb = (torch.rand(1, 3, WIN, WIN, generator=g) * 2 - 1).cuda()
    table = torch.tensor([[0, 0, 0, WIN, 0, WIN]], dtype=torch.int32)
    tdev = table.cuda()
    srcs = [torch.randn(8, c, s * WIN, s * WIN, generator=g).cuda() for c, s in OUTPUTS]
    outs = [torch.empty(1, c, s * WIN, s * WIN, device="cuda") for c, s in OUTPUTS]

    def k_gather():
        return C.d8_gather(lr, lrb, table, tdev, WIN, WIN, 0, 8)

    def k_merge():
        C.d8_merge(srcs, [], outs, table, tdev, WIN, WIN, WIN, WIN)

    def t_gather():
        return (torch.stack([variant(lr[0], k) for k in range(8)]), torch.stack([variant(lrb[0], k) for k in range(8)]))

    def t_merge():
        return [torch.stack([back(x[k], k) for k in range(8)]).mean(0) for x in srcs]

    # results first
    ka, kb = k_gather()
    ta, tb = t_gather()
    gather_equal = torch.equal(ka.flatten(0, 2), ta) and torch.equal(kb.flatten(0, 2), tb)
    k_merge()
    ordered_equal, mean_diff = True, 0.0
    for x, o, m in zip(srcs, outs, t_merge()):
        acc = back(x[0], 0)
        for k in range(1, 8):
            acc = acc + back(x[k], k)
        ordered_equal = ordered_equal and torch.equal(o[0], acc * 0.125)
        mean_diff = max(mean_diff, float((o[0] - m).abs().max()))
    again = [o.clone() for o in outs]
    k_merge()
    same_bits = all(torch.equal(x, y) for x, y in zip(again, outs))
    forms = {"kernels_gather": k_gather, "kernels_merge": k_merge, "kernels_gather_and_merge": lambda: (k_gather(), k_merge()),
             "torch_gather": t_gather, "torch_merge": t_merge, "torch_gather_and_merge": lambda: (t_gather(), t_merge())}
    t = timed(forms, regions, calls)
    values = sum(c * (s * WIN) ** 2 for c, s in OUTPUTS)
    merge_bytes = 9 * 4 * values
    res = {"window": [WIN, WIN], "outputs_channels_scale": OUTPUTS, "times": {k: stats(v) for k, v in t.items()},
           "gather_equals_torch_bit_for_bit": bool(gather_equal), "merge_equals_ordered_torch_sum_bit_for_bit": bool(ordered_equal),
           "merge_largest_difference_from_torch_mean": mean_diff, "merge_two_runs_same_bits": bool(same_bits),
           "merge_bytes_8_reads_1_write_per_value": merge_bytes}
    med = {k: statistics.median(v) for k, v in t.items()}
    rate = merge_bytes / (med["kernels_merge"] * 1e-6)
    res["merge_achieved_TB_per_s"] = round(rate / 1e12, 3)
    res["merge_share_of_HBM_spec_8.0_TB_per_s"] = round(rate / HBM_SPEC, 3)
    res["merge_share_of_measured_copy_6.29_TB_per_s"] = round(rate / HBM_COPY, 3)
    res["torch_over_kernels"] = {k: round(med["torch_" + k] / med["kernels_" + k], 2) for k in ("gather", "merge", "gather_and_merge")}
    return res


def load_pipeline():
    z = np.load(os.path.join(ROOT, "tests", "golden", "face_S8_weights.npz"))

    def sd(prefix):
        return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix) and z[k].dtype.kind in "fiub"}
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM, cfg.TREE.BRANCH_NUM = 32, 256, 4
    return SRPipeline(41, device="cuda", low="lr").load_state_dicts(sd("E."), sd("GL."), sd("GH."))


def part_b(regions, calls):
    pipe = load_pipeline()
    g = torch.Generator().manual_seed(100)
    cap = torch.zeros(18, dtype=torch.int64)
    cap[:WORDS] = torch.randint(1, 41, (WORDS,), generator=g)
    cap = cap.cuda()
    H = W = 256
    lr = (torch.rand(3, H, W, generator=g) * 2 - 1).cuda()

    def ensemble(graph):
        return lambda: pipe.upscale(lr, cap, WORDS, graph=graph, ensemble=8)

    def eight(graph):
        def run():
            rs = [pipe.upscale(variant(lr, k).contiguous(), cap, WORDS, graph=graph) for k in range(8)]
            return {name: [torch.stack([back(rs[k][name][i], k) for k in range(8)]).mean(0) for i in range(3)] for name in ("fine", "fake")}
        return run

    forms = {"upscale_ensemble8": ensemble(False), "eight_upscales_and_torch": eight(False),
             "upscale_ensemble8_graph": ensemble(True), "eight_upscales_and_torch_graph": eight(True)}
    a, b = forms["upscale_ensemble8"](), forms["eight_upscales_and_torch"]()
    diff = max(float((a[name][i] - b[name][i]).abs().max()) for name in ("fine", "fake") for i in range(3))
    ga = forms["upscale_ensemble8_graph"]()
    graph_equal = all(torch.equal(a[name][i], ga[name][i]) for name in ("fine", "fake") for i in range(3))
    del a, b, ga
    t = timed(forms, regions, calls)
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"lr": [H, W], "tile": 128, "tile_batch": 4, "times": {k: stats(v, "ms", 1e-3) for k, v in t.items()},
            "largest_difference_between_the_two_forms": diff, "graph_equals_eager_bit_for_bit": bool(graph_equal),
            "eight_upscales_over_ensemble8": round(med["eight_upscales_and_torch"] / med["upscale_ensemble8"], 2),
            "eight_upscales_over_ensemble8_graph": round(med["eight_upscales_and_torch_graph"] / med["upscale_ensemble8_graph"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_ensemble_timing.json"))
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="calls per region of (a); (b) takes 2")
    ap.add_argument("--only", choices=("a", "b"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_self_ensemble needs the GPU")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "median of %d fenced regions (device events around back-to-back calls, a synchronise behind them), the forms "
                     "alternating region by region; (a) %d calls per region, us per call; (b) 2 calls per region, ms per image"
                     % (args.regions, args.calls)}
    with torch.no_grad():
        if args.only != "b":
            res["a_one_window"] = part_a(args.regions, args.calls)
        if args.only != "a":
            res["b_upscale_256"] = part_b(args.regions, 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
