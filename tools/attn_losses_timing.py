#!/usr/bin/env python3
"""Time of the attention-guided objectives at the training shape (B = 16, T = 18; maps 32^2 / 64^2 / 128^2 under images 64^2 /
128^2 / 256^2; DAMSM: nef 256, 17 x 17 regions):

  weight_MSE, forward + backward   the fused form (autograd.WeightMSE: one forward and one backward launch per scale, plus the finish
                                   kernel) against the torch composition of the reference's expression on the same DEVICE tensors
                                   (max, Upsample, scale, sub, pow, mul, sum, div and autograd's walk back through them).  The
                                   composition is the baseline, not the code under test.  Twice: the gradient into the images only
                                   (what SRTrainer asks for: its maps carry no gradient) and into images and maps.
  words_reweight_loss              forward + backward against words_loss on the same inputs: what the re-weighting adds (one
                                   tgsr_attn_confidence launch and a multiply); and that launch alone.

    python tools/attn_losses_timing.py [--out profiles/attn_losses_timing.json] [--rounds 7] [--calls 400]

Each figure is the median over `rounds` fenced regions (device events around `calls` back-to-back calls, a synchronise behind them)
of the time per call - 400 calls of 0.35-0.6 ms make a region of 0.15-0.25 s; the forms alternate round by round, so that whatever
else the machine does falls on all of them, and minimum and maximum over the regions are recorded beside the median.  The bytes
are the ones the algorithm needs, counted from the shapes.  No threshold is fixed in advance.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgsr_amd.miscc import losses  # noqa: E402
from tgsr_amd.miscc.config import cfg  # noqa: E402

B, T, NEF = 16, 18, 256
MAPS, IMAGES = (32, 64, 128), (64, 128, 256)


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


def wmse_bytes(att_grad):
    """Bytes one fused forward + backward over the three scales has to move: forward reads fake, label, att and writes the maximum and
    its index; backward reads fake, label, maximum and index and writes d_fake (and d_att)."""
    n = 0
    for m, s in zip(MAPS, IMAGES):
        img, mp = 4 * B * 3 * s * s, B * m * m
        n += 2 * img + 4 * T * mp + 5 * mp              # forward
        n += 2 * img + 5 * mp + img                      # backward, d_fake
        if att_grad:
            n += 4 * T * mp
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "attn_losses_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=400)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_losses_timing needs the GPU")
    g = torch.Generator().manual_seed(0)
    fake = [torch.tanh(torch.randn(B, 3, s, s, generator=g)).cuda().requires_grad_(True) for s in IMAGES]
    label = [torch.tanh(torch.randn(B, 3, s, s, generator=g)).cuda() for s in IMAGES]
    att = [torch.softmax(3.0 * torch.randn(B, T, m, m, generator=g), dim=1).cuda() for m in MAPS]
    att_g = [a.clone().requires_grad_(True) for a in att]

    def wmse(maps, fused):
        def run():
            for t in fake + att_g:
                t.grad = None
            loss, _ = losses.weight_MSE(fake, label, maps, fused=fused)
            loss.backward()
            return loss.detach()
        return run

    lens = [T, 16, 14, 12] * (B // 4)
    lens.sort(reverse=True)
    regions = torch.randn(B, NEF, 17, 17, generator=g).cuda().requires_grad_(True)
    words = torch.randn(B, NEF, T, generator=g).cuda().requires_grad_(True)
    sharp = torch.softmax(12.0 * torch.randn(B, T, 128, 128, generator=g), dim=1).cuda()      # peaked: words pass their thresholds
    labels = torch.arange(B).cuda()

    def ranking(fn):
        def run():
            regions.grad = words.grad = None
            w0, w1, _ = fn()
            (w0 + w1).backward()
            return (w0 + w1).detach()
        return run

    runs = {
        "weight_mse_fused_image_grad": wmse(att, None),
        "weight_mse_torch_composition_image_grad": wmse(att, False),
        "weight_mse_fused_image_and_map_grad": wmse(att_g, None),
        "weight_mse_torch_composition_image_and_map_grad": wmse(att_g, False),
        "words_loss": ranking(lambda: losses.words_loss(regions, words, labels, lens, None, B)),
        "words_reweight_loss": ranking(lambda: losses.words_reweight_loss(regions, words, labels, lens, None, B, sharp)),
        "confidence_kernel": lambda: losses.attn_confidence(sharp, lens),
    }
    # results first: faster and different is not faster
    a, b = float(runs["weight_mse_fused_image_and_map_grad"]()), float(runs["weight_mse_torch_composition_image_and_map_grad"]())
    fused_grads = [t.grad.clone() for t in fake + att_g]
    runs["weight_mse_torch_composition_image_and_map_grad"]()
    grad_diff = max(float((x - t.grad).abs().max() / t.grad.abs().max()) for x, t in zip(fused_grads, fake + att_g))
    conf = runs["confidence_kernel"]()
    comp = losses.attn_confidence(sharp, lens, fused=False)
    conf_diff = float(((conf - comp).abs() / comp.clamp_min(1e-30)).max())
    for name, fn in runs.items():
        fenced(fn, 2)
    times = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            times[name].append(fenced(fn, args.calls))
    res = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"B": B, "T": T, "maps": list(MAPS), "images": list(IMAGES), "nef": NEF, "regions": [17, 17], "cap_lens": lens,
                  "gamma": [cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3]},
        "method": "median of %d fenced regions of %d calls each, the forms alternating; us per call: forward + backward over the "
                  "three scales for weight_MSE, forward + backward for the ranking losses, forward for the confidences"
                  % (args.rounds, args.calls),
        "times": {name: stats(v) for name, v in times.items()},
        "weight_mse_value": {"fused": a, "torch_composition": b, "relative_difference": abs(a - b) / abs(b)},
        "weight_mse_largest_gradient_difference_over_largest_gradient": grad_diff,
        "confidence_largest_relative_difference_kernel_vs_torch_composition": conf_diff,
        "words_above_their_threshold": int((conf > 0).sum()),
    }
    t = res["times"]
    for tag, att_grad in (("image_grad", False), ("image_and_map_grad", True)):
        us = t["weight_mse_fused_" + tag]["median_us"]
        res["weight_mse_speedup_" + tag] = round(t["weight_mse_torch_composition_" + tag]["median_us"] / us, 2)
        res["weight_mse_fused_%s_algorithmic_GB_per_s" % tag] = round(wmse_bytes(att_grad) / us / 1e3, 1)
    res["weight_mse_algorithmic_MB"] = {"image_grad": round(wmse_bytes(False) / 1e6, 1), "image_and_map_grad": round(wmse_bytes(True) / 1e6, 1)}
    res["words_reweight_loss_over_words_loss"] = round(t["words_reweight_loss"]["median_us"] / t["words_loss"]["median_us"], 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
