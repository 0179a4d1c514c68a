#!/usr/bin/env python3
"""Pinned training steps: what SRTrainer's first GRAPH_G_WARMUP + 3 steps return and leave behind, in its four forms - generators
only and the G/D alternation, each eager and replayed from hipGraphs - on the smallest configuration the trainer has (GF_DIM 32,
EMBEDDING_DIM 256, DF_DIM 16, B = 4, LR 32 x 32, HR 64 / 128 / 256, two caption widths in turn).  Stored in
tests/golden/train_steps.json: `float.hex()` of every returned loss, and after the last step the sha256 over the bytes of every
state_dict tensor of both generators and each discriminator, and of the EMA copies.
TEST INFRASTRUCTURE - needs the device.  It touches the trainer through the names its tests and the benchmark already rely on
(`_graph_g`, `_dsteps`, `step`, `step_gan`, ...), so one recorded file pins the steps ACROSS changes of the trainer's insides;
tests/test_train_steps.py runs `run_cases()` again and compares.
"""
import hashlib
import json
import os
import sys

import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

CASES = (("g_eager", False, False), ("g_replay", False, True), ("gd_eager", True, False), ("gd_replay", True, True))
B = 4


def _sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run_case(gan, graphs, device="cuda"):
    from tgsr_amd import train
    from tgsr_amd.synthetic import synthetic_batch
    torch.manual_seed(5)
    tr = train.SRTrainer(41, device=device, discriminators=gan)
    tr._graph_g = graphs                                     # pinned: replay from step GRAPH_G_WARMUP on | never
    if gan and not graphs:
        tr._dsteps = -10 ** 9                                # the discriminator updates stay eager too
    losses = []
    for step in range(train.GRAPH_G_WARMUP + 3):
        cap, lens, LR, LRb = synthetic_batch(B, seed=40 + step % 2)
        g = torch.Generator().manual_seed(step)
        hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).to(device) for s in (64, 128, 256)]
        torch.manual_seed(100 + step)                        # CA_NET's noise
        args = (cap.to(device), lens.tolist(), LR.to(device), LRb.to(device), hr)
        if gan:
            errG, errsD = tr.step_gan(*args)
            losses.append({"errG": float(errG).hex(), "errD": [float(e).hex() for e in errsD]})
        else:
            losses.append({"errG": float(tr.step(*args)).hex()})
    torch.cuda.synchronize()
    assert bool(tr._ggraphs) == bool(graphs), "the replaying case must have captured, the eager one must not"
    state = {"netGL": _sha(tr.netGL.state_dict().values()), "netGH": _sha(tr.netGH.state_dict().values()),
             "avg_param_G": _sha(tr.avg_param_G)}
    for i, d in enumerate(tr.netsD):
        state["netD%d" % i] = _sha(d.state_dict().values())
    return {"losses": losses, "state": state}


def run_cases(device="cuda"):
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM, cfg.GAN.DF_DIM = 32, 256, 16
    try:
        return {name: run_case(gan, graphs, device) for name, gan, graphs in CASES}
    finally:
        cfg_reset()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(OUT, "train_steps.json")
    with open(path, "w") as f:
        json.dump(run_cases(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
