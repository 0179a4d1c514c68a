#!/usr/bin/env python3
"""Time of a retrieval gallery at the DAMSM encoders' own shape (ndf = 256, 17 x 17 regions, captions of 1..18 words): the gallery
kernel (tgsr_damsm_gallery_fwd, two short captions per MFMA tile) against the only way to score a gallery before it, the pair
kernel of the training loss (tgsr_damsm_words_fwd) on the same square problem - and the R-precision shape (100 candidates per image
out of a pool of 256), for which the pair kernel has no form: it would have to score the full grid.

    python tools/retrieval_timing.py [--out profiles/retrieval_timing.json] [--rounds 7] [--calls 5]

Each figure is the median over `rounds` fenced regions (device events around `calls` back-to-back launches, a synchronise behind
them) of the time per launch; the two kernels alternate round by round, so that whatever else the machine does falls on both.
The outputs of both kernels on the square problem are compared before anything is timed.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgsr_amd import ops, retrieval  # noqa: E402

N, NDF, TW, K = 256, 256, 18, 100


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "retrieval_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_timing needs the GPU")
    g = torch.Generator().manual_seed(0)
    regions = torch.randn(N, NDF, 17, 17, generator=g).cuda()
    words = torch.randn(N, NDF, TW, generator=g).cuda()
    lens = torch.randint(1, TW + 1, (N,), generator=g).tolist()
    cand = retrieval.sample_candidates(torch.randint(0, 50, (N,), generator=g), K, g).cuda()
    runs = {
        "pair_kernel_square": lambda: ops.damsm_words_similarity(regions, words, lens, 5.0, 5.0, need_att=False),
        "gallery_kernel_square": lambda: ops.damsm_gallery(regions, words, lens, 5.0, 5.0),
        "gallery_kernel_r_precision": lambda: ops.damsm_gallery(regions, words, lens, 5.0, 5.0, cand),
    }
    old, new = runs["pair_kernel_square"]()[0], runs["gallery_kernel_square"]()
    diff = float((old - new).abs().max())
    listed = runs["gallery_kernel_r_precision"]()
    same = bool(torch.equal(listed, torch.gather(new, 1, cand.long())))
    for fn in runs.values():                                            # warm-up of every shape
        fenced(fn, 2)
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            times[k].append(fenced(fn, args.calls))
    short = sum(n <= 16 for n in lens)
    packed = sum(lens[2 * q] <= 16 and lens[2 * q + 1] <= 16 for q in range(N // 2))
    res = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"N": N, "M": N, "ndf": NDF, "S": 289, "Tw": TW, "K_r_precision": K,
                  "captions_of_at_most_16_words": short, "column_pairs_packed_on_the_square_problem": "%d of %d" % (packed, N // 2)},
        "method": "median of %d fenced regions of %d launches each, kernels alternating; us per launch" % (args.rounds, args.calls),
        "max_abs_difference_pair_vs_gallery": diff,
        "r_precision_scores_are_the_square_scores_bit_for_bit": same,
        "times": {k: stats(v) for k, v in times.items()},
    }
    sq_old, sq_new = res["times"]["pair_kernel_square"]["median_us"], res["times"]["gallery_kernel_square"]["median_us"]
    res["speedup_square"] = round(sq_old / sq_new, 3)
    res["r_precision_note"] = ("the pair kernel has no candidate-list form: it would score the full %d x %d grid, pair_kernel_square"
                               % (N, N))
    res["speedup_r_precision_vs_full_grid"] = round(sq_old / res["times"]["gallery_kernel_r_precision"]["median_us"], 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
