#!/usr/bin/env python3
"""Time of the cycle-consistency objective at the training shape (B = 16, SR images 64^2 / 128^2 / 256^2 resized back to the
32^2 LR input):

  CycleMSE, forward + backward     the fused form (autograd.CycleMSE: one forward launch for the three scales, the finish kernel, one
                                   gather-form backward launch) against the torch composition of the reference's expression on the
                                   same DEVICE tensors (three bicubic interpolations, sub, pow, mean, add and autograd's walk back
                                   through them, whose interpolation backward scatters with atomic adds into a zero-filled
                                   grad_input).  The composition is the baseline, not the code under test.  The gradient goes into
                                   the images, as in SRTrainer (the LR input carries none).
  SRTrainer step (--trainer)       one generator-only step with cycle=0.5 against cycle=0 on this commit: what the term costs a step.

    python tools/cycle_mse_timing.py [--out profiles/cycle_mse_timing.json] [--rounds 7] [--calls 400] [--trainer]

Each figure is the median over `rounds` fenced regions (device events around `calls` back-to-back calls, a synchronise behind them)
of the time per call; the forms alternate round by round, so that whatever else the machine does falls on both, and minimum and
maximum over the regions are recorded beside the median.  The bytes are the ones the algorithm needs, counted from the shapes.  No
threshold is fixed in advance.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgsr_amd.miscc import losses  # noqa: E402

B, C, LR_SIZE, IMAGES = 16, 3, 32, (64, 128, 256)


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


def fused_bytes():
    """Bytes one fused forward + backward has to move.  Forward: 4 x 4 taps per LR pixel - at ratio r >= 4 disjoint windows, (4 / r)^2
    of the image, the whole image at ratio 2 - the LR input once per scale, diff written.  Backward: diff read, d_sr written whole."""
    per = 4 * B * C * LR_SIZE * LR_SIZE
    n = 0
    for s in IMAGES:
        r = s // LR_SIZE
        img = 4 * B * C * s * s
        n += int(img * min(1.0, (4.0 / r) ** 2)) + 2 * per        # forward: touched SR values, lr, diff
        n += per + img                                            # backward: diff, d_sr
    return n


def composed_bytes():
    """Bytes the composition moves at the least: per scale the interpolation (touched SR values in, resized out), the difference
    (two in, one out), its square and mean (read), and backward the gradient of the difference (two passes over LR-sized tensors),
    a memset of grad_input and the scatter into it (read-modify-write of the touched values)."""
    per = 4 * B * C * LR_SIZE * LR_SIZE
    n = 0
    for s in IMAGES:
        r = s // LR_SIZE
        img = 4 * B * C * s * s
        touched = int(img * min(1.0, (4.0 / r) ** 2))
        n += touched + per + 3 * per + per                        # forward
        n += 3 * per + img + 2 * touched                          # backward
    return n


def trainer_steps(cycle, steps, warm):
    from tgsr_amd.miscc.config import cfg
    from tgsr_amd.synthetic import synthetic_batch
    from tgsr_amd.train import SRTrainer
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256          # the shipped configuration, as bench.py sets it
    torch.manual_seed(3)
    tr = SRTrainer(41, device="cuda", cycle=cycle)
    cap, lens, LR, LRb = synthetic_batch(B, seed=100)
    g = torch.Generator().manual_seed(7)
    hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).cuda() for s in IMAGES]
    batch = (cap.cuda(), lens.tolist(), LR.cuda(), LRb.cuda(), hr)
    for _ in range(warm):
        tr.step(*batch)
    return tr, lambda: tr.step(*batch), steps


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "cycle_mse_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--trainer", action="store_true", help="also time an SRTrainer step with cycle=0.5 against cycle=0")
    ap.add_argument("--trainer-steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cycle_mse_timing needs the GPU")
    g = torch.Generator().manual_seed(0)
    sr = [torch.tanh(torch.randn(B, C, s, s, generator=g)).cuda().requires_grad_(True) for s in IMAGES]
    lr = torch.tanh(torch.randn(B, C, LR_SIZE, LR_SIZE, generator=g)).cuda()

    def cycle(fused):
        def run():
            for t in sr:
                t.grad = None
            loss = losses.CycleMSE(sr, lr, fused=fused)
            loss.backward()
            return loss.detach()
        return run

    runs = {"cycle_mse_fused": cycle(None), "cycle_mse_torch_composition": cycle(False)}
    # results first: faster and different is not faster
    a = float(runs["cycle_mse_fused"]())
    fused_grads = [t.grad.clone() for t in sr]
    again = float(runs["cycle_mse_fused"]())
    same_bits = again == a and all(torch.equal(x, t.grad) for x, t in zip(fused_grads, sr))
    b = float(runs["cycle_mse_torch_composition"]())
    grad_diff = max(float((x - t.grad).abs().max() / t.grad.abs().max()) for x, t in zip(fused_grads, sr))
    for fn in runs.values():
        fenced(fn, 2)
    times = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            times[name].append(fenced(fn, args.calls))
    res = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"B": B, "C": C, "lr": [LR_SIZE, LR_SIZE], "images": list(IMAGES)},
        "method": "median of %d fenced regions of %d calls each, the forms alternating; us per call: forward + backward over the "
                  "three scales, gradient into the images" % (args.rounds, args.calls),
        "times": {name: stats(v) for name, v in times.items()},
        "value": {"fused": a, "torch_composition": b, "relative_difference": abs(a - b) / abs(b)},
        "largest_gradient_difference_over_largest_gradient": grad_diff,
        "fused_two_runs_same_bits": bool(same_bits),
        "algorithmic_MB": {"fused": round(fused_bytes() / 1e6, 1), "torch_composition_at_least": round(composed_bytes() / 1e6, 1)},
    }
    t = res["times"]
    res["composition_over_fused"] = round(t["cycle_mse_torch_composition"]["median_us"] / t["cycle_mse_fused"]["median_us"], 2)
    res["fused_algorithmic_GB_per_s"] = round(fused_bytes() / t["cycle_mse_fused"]["median_us"] / 1e3, 1)
    if args.trainer:
        steps = {}
        trainers = {"cycle_0": trainer_steps(0.0, args.trainer_steps, 12), "cycle_0.5": trainer_steps(0.5, args.trainer_steps, 12)}
        times = {k: [] for k in trainers}
        for _ in range(args.rounds):
            for k, (_tr, fn, n) in trainers.items():
                times[k].append(fenced(fn, n) / 1e3)
        for k, v in times.items():
            steps[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                        "form": "replay" if trainers[k][0]._graph_g else "eager"}
        res["srtrainer_step"] = dict(steps, method="generator-only SRTrainer.step at B = %d after 12 warm-up steps (the measured graph "
                                                   "policy has settled); median of %d fenced regions of %d steps, the two trainers "
                                                   "alternating" % (B, args.rounds, args.trainer_steps))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
