#!/usr/bin/env python3
"""Time of NIQE on the device (tgsr_amd/niqe.py, csrc/tgsr_niqe.hip) in the two settings evaluation runs it in:

  batch        B = 16 images of 256 x 256 (four blocks each): a validation batch of SRTrainer.evaluate
  whole_image  one 2048 x 2048 image (441 blocks): a whole `upscale` output

  niqe_features   the two launches of torch.ops.tgsr.niqe_features against the same definition written with torch DEVICE operators
                  (niqe.features_torch on the same device tensor: conv2d, gather, roll, masked sums, searchsorted, lgamma - every
                  block of the batch at once, no block loop and no synchronisation: the kindest torch form there is)
  score           NIQEModel.score_features on the features (batched mean, covariance, eigh, quadratic form; torch fp64), and
                  torch.linalg.eigh alone on B symmetric 36 x 36 matrices - the part of it the device solver takes
  evaluate        SRTrainer.evaluate over 16 batches of 16 with and without niqe=<model>: the share the argument adds

    python tools/niqe_timing.py [--out profiles/niqe_timing.json] [--rounds 7] [--skip-evaluate] [--kernel-stats CSV ...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/niqe_timing.py --trace batch      # a run of its own per setting

Each time is the median over `rounds` fenced regions of the time per call, the forms alternating round by round, with minimum and
maximum beside it: "device_us" from device events around back-to-back calls, "wall_us" from the host clock around the same calls
and a synchronise.  KERNEL time comes from the profiler in separate runs (--trace runs only the kernels of one setting;
--kernel-stats batch=CSV whole_image=CSV merges the niqe_* rows of rocprofv3's kernel_stats files into the result).  No ratio is fixed
in advance.  Needs the GPU: there is no fallback."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgsr_amd import niqe  # noqa: E402

SETTINGS = {"batch": (16, 256), "whole_image": (1, 2048)}


def images(B, S, seed):
    """uint8 [B, 3, S, S] on the device: a smooth field plus +-6 grey levels of noise (every block has both signs)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.nn.functional.interpolate(torch.randn(B, 3, S // 16, S // 16, generator=g), size=(S, S), mode="bicubic")
    x = 128 + 40 * f + torch.randint(-6, 7, (B, 3, S, S), generator=g)
    return x.clamp(0, 255).to(torch.uint8).cuda()


def fenced(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, (time.perf_counter() - t0) * 1e6 / calls


def stats(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def alternate(runs, rounds, calls):
    for fn in runs.values():
        fenced(fn, 2)
    dev, wall = {n: [] for n in runs}, {n: [] for n in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            d, w = fenced(fn, calls)
            dev[name].append(d)
            wall[name].append(w)
    return {name: {"device_us": stats(dev[name]), "wall_us": stats(wall[name])} for name in runs}


def time_setting(name, rounds, model):
    B, S = SETTINGS[name]
    x = images(B, S, 11)
    runs = {"kernels": lambda: torch.ops.tgsr.niqe_features(x, 0), "torch_device_operators": lambda: niqe.features_torch(x, 0)}
    a, b = runs["kernels"]()[0], runs["torch_device_operators"]()[0]
    feats = a.clone()
    runs["score"] = lambda: model.score_features(feats)
    A = torch.randn(B, 36, 72, dtype=torch.float64, device="cuda")
    spd = A @ A.transpose(1, 2)
    runs["eigh_alone"] = lambda: torch.linalg.eigh(spd)                 # the part of `score` the device solver takes
    t = alternate(runs, rounds, 20 if name == "batch" else 5)
    med = lambda k: t[k]["device_us"]["median"]                       # noqa: E731
    return {"shape": {"B": B, "H": S, "W": S, "blocks_per_image": (S // 96) ** 2}, "times": t,
            "largest_relative_difference": float(((a - b).abs() / b.abs()).max()),
            "torch_over_kernels_device": round(med("torch_device_operators") / med("kernels"), 2),
            "torch_over_kernels_wall": round(t["torch_device_operators"]["wall_us"]["median"] / t["kernels"]["wall_us"]["median"], 2)}


def time_evaluate(model, nb=16, B=16):
    from tgsr_amd.miscc.config import cfg
    from tgsr_amd.synthetic import synthetic_batch
    from tgsr_amd.train import SRTrainer
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256                  # the shipped configuration, as bench.py sets it
    torch.manual_seed(3)
    tr = SRTrainer(41, device="cuda")
    data = []
    for k in range(4):                                                # four distinct batches, walked nb / 4 times
        cap, lens, LR, LRb = synthetic_batch(B, seed=100 + k)
        hr = [images(B, s, 7 + k).float() / 127.5 - 1.0 for s in (64, 128, 256)]
        data.append((cap.cuda(), lens.tolist(), LR.cuda(), LRb.cuda(), hr))
    batches = lambda: (data[k % 4] for k in range(nb))               # noqa: E731

    def wall(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.evaluate(batches(), ema=False, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    wall()
    wall(niqe=model)
    plain, full = [], []
    for _ in range(5):                                                # alternating
        plain.append(wall()[0])
        full.append(wall(niqe=model))
    p, f = statistics.median(plain), statistics.median(t for t, _r in full)
    return {"shape": {"batches": nb, "B": B, "finest": 256},
            "evaluate_wall_us": {"plain": stats([v * 1e6 for v in plain]), "niqe": stats([t * 1e6 for t, _r in full])},
            "share_added_by_niqe": round((f - p) / p, 4), "mean_scores": full[-1][1]["niqe"]["mean"]}


def kernel_rows(path):
    with open(path, newline="") as f:
        return {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                                          "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
                for r in csv.DictReader(f) if "niqe_" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "niqe_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-evaluate", action="store_true")
    ap.add_argument("--trace", choices=sorted(SETTINGS), help="run only the kernels of one setting, 50 times (under the profiler)")
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="SETTING=CSV")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("niqe_timing needs the GPU")
    if args.trace:
        x = images(*SETTINGS[args.trace], 11)
        for _ in range(50):
            torch.ops.tgsr.niqe_features(x, 0)
        torch.cuda.synchronize()
        return
    model = niqe.NIQEModel.fit([images(4, 768, 21 + k) for k in range(2)], sharpness=0.0)     # 512 blocks
    res = {"device": torch.cuda.get_device_name(0),
           "method": "median (min, max) of %d fenced regions of back-to-back calls, the forms alternating; us per call; device_us "
                     "from device events, wall_us from the host clock with a synchronise; kernel_us from rocprofv3 --kernel-trace "
                     "--stats in runs of their own" % args.rounds}
    for name in SETTINGS:
        res[name] = time_setting(name, args.rounds, model)
    for item in args.kernel_stats:
        name, path = item.split("=", 1)
        res[name]["kernel_us"] = kernel_rows(path)
    if not args.skip_evaluate:
        res["evaluate"] = time_evaluate(model)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
