#!/usr/bin/env python3
"""DAMSM pre-training's image side (pretrain_DAMSM.py:49-51, 70): the frozen Inception-v3 trunk in TRAINING mode (batch-statistics
BatchNorm, running statistics updated) on the library's kernels against the torch modules (TGSR_TRUNK=torch: MIOpen conv + BN + ReLU
per layer) on the same box, at B = 16 and B = 48 (cfg/DAMSM/bird.yml: BATCH_SIZE 48), and one full DAMSMTrainer.step from images
at B = 48 with the trunk's share of it.  Device events around fenced windows (a synchronise before and after), the two walks
alternated, the median of the repeats.  Prints one JSON line.
    python tools/bench_damsm_trunk.py [--reps 7] [--iters 5]          (on the GPU box)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def window(fn, iters):
    """ms per call of fn over a fenced window of `iters` calls."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def set_trunk(mode):
    if mode == "torch":
        os.environ["TGSR_TRUNK"] = "torch"
    else:
        os.environ.pop("TGSR_TRUNK", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_damsm_trunk needs a GPU"
    from inception_v3_arch import InceptionV3Arch
    from tgsr_amd import _lib
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import DAMSMTrainer
    from tgsr_amd.util import CNN_ENCODER
    _lib.lib()
    cfg_reset()
    cfg.TRAIN.FLAG = True
    dev = torch.device("cuda")
    res = {"tool": "bench_damsm_trunk", "device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters,
           "trunk_train_fwd_ms": {}}
    enc = CNN_ENCODER(256, inception=InceptionV3Arch(seed=1)).to(dev).train()
    for p in enc.frozen_parameters():
        p.requires_grad = False
    g = torch.Generator().manual_seed(0)
    for B in (16, 48):
        x = (torch.rand(B, 3, 256, 256, generator=g) * 2 - 1).to(dev)

        def walk():
            with torch.no_grad():
                enc.run_trunk(x)
        times = {"hip": [], "torch": []}
        for mode in ("hip", "torch"):                      # warm-up: code objects, MIOpen's algorithm choice, the allocator
            set_trunk(mode)
            window(walk, 2)
        for _ in range(args.reps):
            for mode in ("hip", "torch"):
                set_trunk(mode)
                assert enc._hip_trunk_ok(x) == (mode == "hip")
                times[mode].append(window(walk, args.iters))
        set_trunk("hip")
        med = {k: statistics.median(v) for k, v in times.items()}
        res["trunk_train_fwd_ms"][str(B)] = {"hip": round(med["hip"], 3), "torch": round(med["torch"], 3),
                                             "hip_spread": [round(min(times["hip"]), 3), round(max(times["hip"]), 3)],
                                             "torch_spread": [round(min(times["torch"]), 3), round(max(times["torch"]), 3)],
                                             "speedup": round(med["torch"] / med["hip"], 3)}
    # one DAMSMTrainer.step from images at B = 48 (the HIP walk), and the trunk's share of it
    B, T, n_words = 48, cfg.TEXT.WORDS_NUM, 5450
    tr = DAMSMTrainer(n_words, device=dev, inception=InceptionV3Arch(seed=1))
    lens = sorted((int(v) for v in torch.randint(2, T + 1, (B,), generator=g)), reverse=True)
    cap = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        cap[b, :n] = torch.randint(1, n_words, (n,), generator=g)
    cap = cap.to(dev)
    imgs = (torch.rand(B, 3, 256, 256, generator=g) * 2 - 1).to(dev)
    step = lambda: tr.step(imgs, cap, lens)                # noqa: E731
    window(step, 2)
    st = [window(step, args.iters) for _ in range(args.reps)]
    res["damsm_step_from_images_ms_b48"] = round(statistics.median(st), 3)
    res["damsm_step_spread"] = [round(min(st), 3), round(max(st), 3)]
    res["trunk_share_of_step_b48"] = round(res["trunk_train_fwd_ms"]["48"]["hip"] / res["damsm_step_from_images_ms_b48"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
