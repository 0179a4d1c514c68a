#!/usr/bin/env python3
"""Time of the distribution distances (tgsr_amd/featdist.py, csrc/tgsr_featdist.hip) at the shapes evaluation runs them at:

  FeatureMoments.add      n = 48, D = 2048: the kernel (a read-modify-write of the block-upper part of the fp64 [2048, 2048] outer
                          product) against the torch form on the same DEVICE tensors, outer.addmm_(X64.T, X64) plus the column sum
                          (the widening of X to fp64 is part of the torch form: the kernel reads float32).
  poly_mmd_sums           S = 100 subsets of m = 1000 rows, D = 2048: the kernel against bmm + pow + sum on fp64 tensors (the torch form
                          gathers and widens the subsets, forms the three [S, m, m] kernel matrices and reduces them).
  evaluate(fid, kid)      SRTrainer.evaluate over 64 batches of 16 with the Inception-v3 topology (seeded random weights) as the trunk:
                          per batch the device time of one trunk walk against the statistics' (two adds), the wall time of the whole
                          call with and without fid / kid, and the two finishes (the eigendecompositions, the kernel sums).

    python tools/featdist_timing.py [--out profiles/featdist_timing.json] [--rounds 7] [--skip-evaluate]

Each figure is the median over `rounds` fenced regions (device events around back-to-back calls, a synchronise behind them) of the
time per call; the forms alternate round by round, and minimum and maximum are recorded beside the median.  No ratio is fixed in
advance.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgsr_amd import featdist, ops  # noqa: E402

D = 2048


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


def alternate(runs, rounds, calls):
    for fn in runs.values():
        fenced(fn, 2)
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(fenced(fn, calls[name] if isinstance(calls, dict) else calls))
    return {name: stats(v) for name, v in times.items()}


def feats(n, seed, scale=0.5, shift=0.3):
    g = torch.Generator().manual_seed(seed)
    return torch.clamp(scale * torch.randn(n, D, generator=g) + shift, min=0).cuda()


def time_moments(rounds):
    x = feats(48, 1)
    s, o = torch.zeros(D, dtype=torch.float64, device="cuda"), torch.zeros(D, D, dtype=torch.float64, device="cuda")
    s2, o2 = torch.zeros_like(s), torch.zeros_like(o)

    def torch_form():
        X = x.to(torch.float64)
        s2.add_(X.sum(0))
        o2.addmm_(X.t(), X)
    runs = {"kernel": lambda: ops.feat_moments_add(x, s, o), "torch_addmm": torch_form}
    runs["kernel"](); runs["torch_addmm"]()
    diff = float((torch.triu(o) - torch.triu(o2)).abs().max() / o2.abs().max())
    t = alternate(runs, rounds, 200)
    nb = D // 64
    rmw = 2 * 8 * 64 * 64 * nb * (nb + 1) // 2
    return {"shape": {"n": 48, "D": D}, "times": t, "largest_relative_difference": diff,
            "kernel_read_modify_write_MB": round(rmw / 1e6, 1),
            "kernel_GB_per_s": round(rmw / t["kernel"]["median_us"] / 1e3, 1),
            "torch_over_kernel": round(t["torch_addmm"]["median_us"] / t["kernel"]["median_us"], 2)}


def time_mmd(rounds, S=100, m=1000, n=1024):
    x, y = feats(n, 2), feats(n, 3, 0.6, 0.35)
    ix, iy = (t.cuda() for t in featdist.subset_tables(n, n, S, m, torch.Generator().manual_seed(4)))

    def torch_form():
        X, Y = x.to(torch.float64)[ix.long()], y.to(torch.float64)[iy.long()]
        kxx, kyy, kxy = ((torch.bmm(P, Q.transpose(1, 2)) / D + 1.0).pow(3) for P, Q in ((X, X), (Y, Y), (X, Y)))
        dg = lambda k: k.diagonal(dim1=1, dim2=2).sum(1)                                 # noqa: E731
        return torch.stack([kxx.sum((1, 2)) - dg(kxx), kyy.sum((1, 2)) - dg(kyy), kxy.sum((1, 2))], 1)
    runs = {"kernel": lambda: ops.poly_mmd_sums(x, y, ix, iy), "torch_bmm_pow_sum": torch_form}
    a, b = runs["kernel"](), runs["torch_bmm_pow_sum"]()
    t = alternate(runs, rounds, 3)
    T = (m + 63) // 64
    flops = 2.0 * D * 64 * 64 * S * (T * T + T * (T + 1))            # the tiles the kernel runs
    return {"shape": {"S": S, "m": m, "D": D, "rows": n}, "times": t,
            "largest_relative_difference": float(((a - b).abs() / b.abs()).max()),
            "kernel_fp64_TFLOP_per_s": round(flops / t["kernel"]["median_us"] / 1e6, 2),
            "torch_over_kernel": round(t["torch_bmm_pow_sum"]["median_us"] / t["kernel"]["median_us"], 2)}


def time_evaluate(rounds, nb=64, B=16):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from inception_v3_arch import InceptionV3Arch
    from tgsr_amd.miscc.config import cfg
    from tgsr_amd.synthetic import synthetic_batch
    from tgsr_amd.train import SRTrainer
    from tgsr_amd.util import CNN_ENCODER
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256                  # the shipped configuration, as bench.py sets it
    torch.manual_seed(3)
    enc = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM, inception=InceptionV3Arch(seed=1)).cuda().eval()
    for p in enc.parameters():
        p.requires_grad = False
    tr = SRTrainer(41, device="cuda", image_encoder=enc)
    data = []
    for k in range(4):                                                # four distinct batches, walked nb / 4 times
        cap, lens, LR, LRb = synthetic_batch(B, seed=100 + k)
        g = torch.Generator().manual_seed(7 + k)
        hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).cuda() for s in (64, 128, 256)]
        data.append((cap.cuda(), lens.tolist(), LR.cuda(), LRb.cuda(), hr))
    batches = lambda: (data[k % 4] for k in range(nb))               # noqa: E731
    img = data[0][4][-1]
    with torch.no_grad():
        pooled = enc.run_trunk(img)[1]
        mom = [featdist.FeatureMoments(D, "cuda"), featdist.FeatureMoments(D, "cuda")]

        def add2():
            mom[0].add(pooled); mom[1].add(pooled)
        per_batch = alternate({"trunk_walk": lambda: enc.run_trunk(img), "statistics_two_adds": add2}, rounds, 20)

        def wall(**kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tr.evaluate(batches(), ema=False, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res
        wall()
        wall(fid=True, kid=True)
        plain = [wall()[0] for _ in range(3)]
        full = [wall(fid=True, kid=True, generator=torch.Generator().manual_seed(1)) for _ in range(3)]
        res = full[-1][1]
        bank = feats(nb * B, 5)
        m2 = featdist.FeatureMoments(D, "cuda").add(bank)
        m3 = featdist.FeatureMoments(D, "cuda").add(feats(nb * B, 6, 0.6, 0.35))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fd = featdist.frechet_distance(m2, m3)
        t_fid = time.perf_counter() - t0
        t0 = time.perf_counter()
        featdist.kernel_distance(bank, feats(nb * B, 6, 0.6, 0.35), generator=torch.Generator().manual_seed(2))
        t_kid = time.perf_counter() - t0
    return {"shape": {"batches": nb, "B": B, "trunk": "Inception-v3 topology, seeded random weights, the library's own kernels"},
            "per_batch_device_time": per_batch,
            "statistics_over_trunk": round(per_batch["statistics_two_adds"]["median_us"] / per_batch["trunk_walk"]["median_us"], 4),
            "evaluate_wall_s": {"plain_median": round(statistics.median(plain), 3),
                                "fid_kid_median": round(statistics.median(t for t, _r in full), 3)},
            "finish_wall_s": {"frechet_distance": round(t_fid, 3), "kernel_distance_100x1000": round(t_kid, 3),
                              "eigh_on": str(featdist.solver_device("cuda"))},
            "scores": {"fid": res["fid"], "kid_mean": res["kid"]["mean"], "kid_std": res["kid"]["std"], "fid_of_two_random_sets": fd}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "featdist_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-evaluate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("featdist_timing needs the GPU")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "median of %d fenced regions (device events around back-to-back calls), the forms alternating; us per call"
                     % args.rounds,
           "moments_add": time_moments(args.rounds), "poly_mmd_sums": time_mmd(args.rounds)}
    if not args.skip_evaluate:
        res["evaluate"] = time_evaluate(args.rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
