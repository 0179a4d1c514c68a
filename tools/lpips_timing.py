#!/usr/bin/env python3
"""Time of LPIPS on the device (tgsr_amd/lpips.py, csrc/tgsr_lpips.hip) where evaluation and training run it: B = 16 pairs of 256 x 256.

  tail       per VGG tap shape of a 256 x 256 image (64 x 256^2, 128 x 128^2, 256 x 64^2, 512 x 32^2, 512 x 16^2): tgsr::lpips_layer and
             tgsr::lpips_layer_bwd against the same definition written with torch DEVICE operators in float32 (normalise both, square the
             difference, weight, sum, mean - and autograd for the gradient), and all five taps + tgsr::lpips_finish against the torch
             form of all five.  "bytes" are what the definition has to move: both features once (forward), both features and df0
             (backward); achieved bytes/s = bytes / device time of back-to-back calls, against the float4 copy figure of this card
             (6.29 TB/s, README).
  forward    LPIPS.forward on 16 pairs without a gradient (scaling, thirteen tgsr::gconv, four pools, the tails)
  train      forward + backward to x (the tape in reverse)
  evaluate   SRTrainer.evaluate over 8 batches of 16 with and without lpips=<model>: the share the argument adds
  step       SRTrainer.step (generators only, B = 16) with and without perceptual=(model, 1.0)

    python tools/lpips_timing.py [--out profiles/lpips_timing.json] [--rounds 7] [--skip-trainer]

Each time is the median over `rounds` fenced regions of the time per call, the forms alternating round by round, with minimum and
maximum beside it: "device_us" from device events around back-to-back calls, "wall_us" from the host clock around the same calls and
a synchronise.  The weights are LPIPS.random's: the times do not depend on them.  No ratio is fixed in advance.  Needs the GPU: there is
no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgsr_amd import lpips  # noqa: E402

B, SIDE = 16, 256
TAPS = [(64, 256), (128, 128), (256, 64), (512, 32), (512, 16)]
COPY_BYTES_PER_S = 6.29e12


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


def tail_torch(f0, f1, w):
    """One tap by torch operators in float32 (the lpips package's form)."""
    n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
    return (w.view(1, -1, 1, 1) * (n0 - n1) ** 2).sum(1).mean((1, 2))


def time_tail(rounds):
    g = torch.Generator().manual_seed(5)
    feats = []
    for C, S in TAPS:
        f0 = torch.relu(torch.randn(B, C, S, S, generator=g)).cuda()
        f1 = torch.relu(f0 + 0.3 * torch.randn(B, C, S, S, generator=g).cuda())
        feats.append((f0, f1, (torch.rand(C, generator=g) * 0.1).cuda()))
    gb = torch.ones(B, device="cuda")
    res = {}
    for (C, S), (f0, f1, w) in zip(TAPS, feats):
        df = torch.empty_like(f0)
        fr = f0.clone().requires_grad_(True)

        def torch_bwd():
            fr.grad = None
            tail_torch(fr, f1, w).sum().backward()
        runs = {"kernel_fwd": lambda: torch.ops.tgsr.lpips_layer(f0, f1, w), "torch_fwd": lambda: tail_torch(f0, f1, w),
                "kernel_bwd": lambda: torch.ops.tgsr.lpips_layer_bwd(gb, f0, f1, w, df, False, f0), "torch_fwd_bwd": torch_bwd}
        t = alternate(runs, rounds, 20)
        med = lambda k: t[k]["device_us"]["median"]                     # noqa: E731
        nbytes = {"kernel_fwd": 2 * f0.numel() * 4, "kernel_bwd": 4 * f0.numel() * 4}      # bwd: f0, f1, the mask (= f0, cached), df0
        res["%dx%dx%d" % (C, S, S)] = {
            "times": t, "bytes": nbytes,
            "achieved_TB_per_s": {k: round(nbytes[k] / med(k) / 1e6, 3) for k in nbytes},
            "share_of_copy_rate": {k: round(nbytes[k] / med(k) * 1e6 / COPY_BYTES_PER_S, 3) for k in nbytes},
            "torch_over_kernel_fwd": round(med("torch_fwd") / med("kernel_fwd"), 2),
            "torch_fwd_bwd_over_kernel_bwd": round(med("torch_fwd_bwd") / med("kernel_bwd"), 2)}

    def kernels():
        parts = [torch.ops.tgsr.lpips_layer(f0, f1, w) for f0, f1, w in feats]
        return torch.ops.tgsr.lpips_finish(parts, [S * S for _c, S in TAPS])[1]

    def torch_all():
        return sum(tail_torch(f0, f1, w) for f0, f1, w in feats)
    a, b = kernels(), torch_all()
    t = alternate({"kernels": kernels, "torch_device_operators": torch_all}, rounds, 20)
    total = sum(2 * f0.numel() * 4 for f0, _f1, _w in feats)
    med = t["kernels"]["device_us"]["median"]
    res["all_five"] = {"times": t, "bytes": total, "achieved_TB_per_s": round(total / med / 1e6, 3),
                       "share_of_copy_rate": round(total / med * 1e6 / COPY_BYTES_PER_S, 3),
                       "torch_over_kernels_device": round(t["torch_device_operators"]["device_us"]["median"] / med, 2),
                       "largest_relative_difference": float(((a - b).abs() / b.abs()).max())}
    return res


def pairs(seed):
    g = torch.Generator().manual_seed(seed)
    hr = torch.nn.functional.interpolate(torch.randn(B, 3, SIDE // 8, SIDE // 8, generator=g), size=(SIDE, SIDE), mode="bicubic").tanh()
    sr = (hr + 0.1 * torch.randn(B, 3, SIDE, SIDE, generator=g)).clamp(-1, 1)
    return sr.cuda(), hr.cuda()


def time_module(model, rounds):
    x, y = pairs(3)
    xg = x.clone().requires_grad_(True)

    def train():
        xg.grad = None
        model(xg, y).sum().backward()

    with torch.no_grad():
        fwd = lambda: model(x, y)                                       # noqa: E731
        t = alternate({"forward": fwd}, rounds, 5)
    t.update(alternate({"forward_backward": train}, rounds, 5))
    return {"shape": {"B": B, "H": SIDE, "W": SIDE}, "times": t, "d": model(x, y).tolist()[:4]}


def trainer_setup(nb):
    from tgsr_amd.miscc.config import cfg
    from tgsr_amd.synthetic import synthetic_batch
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256                  # the shipped configuration, as bench.py sets it
    data = []
    for k in range(nb):
        cap, lens, LR, LRb = synthetic_batch(B, seed=100 + k)
        g = torch.Generator().manual_seed(7 + k)
        hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).cuda() for s in (64, 128, 256)]
        data.append((cap.cuda(), lens.tolist(), LR.cuda(), LRb.cuda(), hr))
    return data


def time_evaluate(model, nb=8):
    from tgsr_amd.train import SRTrainer
    data = trainer_setup(4)
    torch.manual_seed(3)
    tr = SRTrainer(41, device="cuda")
    batches = lambda: (data[k % 4] for k in range(nb))               # noqa: E731

    def wall(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.evaluate(batches(), ema=False, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    wall()
    wall(lpips=model)
    plain, full = [], []
    for _ in range(5):                                                # alternating
        plain.append(wall()[0])
        full.append(wall(lpips=model))
    p, f = statistics.median(plain), statistics.median(t for t, _r in full)
    return {"shape": {"batches": nb, "B": B, "finest": 256},
            "evaluate_wall_us": {"plain": stats([v * 1e6 for v in plain]), "lpips": stats([t * 1e6 for t, _r in full])},
            "added_per_batch_us": round((f - p) / nb * 1e6, 1), "share_added_by_lpips": round((f - p) / p, 4),
            "mean_score": full[-1][1]["lpips"]["mean"]}


def time_step(model, rounds):
    from tgsr_amd.train import SRTrainer
    batch = trainer_setup(1)[0]
    trs = {}
    for name, kw in (("plain", {}), ("perceptual", {"perceptual": (model, 1.0)})):
        torch.manual_seed(3)
        trs[name] = SRTrainer(41, device="cuda", **kw)
        trs[name]._graph_g = False                                    # both eager: the same form on both sides
    runs = {name: (lambda tr=tr: tr.step(*batch)) for name, tr in trs.items()}
    t = alternate(runs, rounds, 5)
    p, f = t["plain"]["wall_us"]["median"], t["perceptual"]["wall_us"]["median"]
    return {"shape": {"B": B, "finest": 256, "form": "eager generator-only step"}, "times": t, "added_us": round(f - p, 1),
            "share_added_by_perceptual": round((f - p) / p, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-trainer", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_timing needs the GPU")
    model = lpips.LPIPS.random(1, "cuda")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "median (min, max) of %d fenced regions of back-to-back calls, the forms alternating; us per call; device_us from "
                     "device events, wall_us from the host clock with a synchronise; bytes/s = the bytes the definition moves over "
                     "device_us, against the float4 copy figure %.2f TB/s" % (args.rounds, COPY_BYTES_PER_S / 1e12)}
    res["tail"] = time_tail(args.rounds)
    res["module"] = time_module(model, args.rounds)
    if not args.skip_trainer:
        res["evaluate"] = time_evaluate(model)
        res["step"] = time_step(model, args.rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
