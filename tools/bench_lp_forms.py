#!/usr/bin/env python3
"""NetG_highweight's four forms (weightmap x use_act, model.py:212-298) on the reduced-precision path: graph-replayed steps
of SRPipeline at batch B, one lane, the forms alternated round by round so that they share the host's noise; and the PSNR of
the finest image of each form against the fp32 pipeline of the same form (shipped face checkpoint, tests/golden; the maps
0.5 + 0.2 randn, fixed seed).  One JSON line per form.
    python tools/bench_lp_forms.py [--dtype bf16] [--batch 16] [--steps 200] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import tgsr_oracle as O  # noqa: E402
from oracle import tgsr_oracle_lp as OL  # noqa: E402
from tgsr_amd.miscc.config import cfg, cfg_reset  # noqa: E402
from tgsr_amd.trainer import SRPipeline  # noqa: E402

FORMS = [("shipped", False, True), ("map-tanh", True, True), ("scalar-identity", False, False), ("map-identity", True, False)]


def weights(weightmap):
    z = np.load(os.path.join(ROOT, "tests", "golden", "face_S8_weights.npz"))

    def part(prefix):
        return {k[len(prefix):]: torch.from_numpy(np.asarray(z[k])) for k in z.files
                if k.startswith(prefix) and np.asarray(z[k]).dtype.kind in "fiub"}
    sdE, sdL, sdH = part("E."), part("GL."), part("GH.")
    sdH = {k: v for k, v in sdH.items() if k != "a"}
    if weightmap:
        g = torch.Generator().manual_seed(11)
        sdH.update({"a%d" % (k + 1): 0.5 + 0.2 * torch.randn(n, n, generator=g) for k, n in enumerate((64, 128, 256))})
    return sdE, sdL, sdH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lp_forms: no GPU")
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM, cfg.TREE.BRANCH_NUM = 32, 256, 4
    cap, lens, LR, LRb = O.synthetic_batch(a.batch)
    args = (cap.cuda(), lens.tolist(), LR.cuda(), LRb.cuda())
    pipes, res = {}, {}
    for name, wm, act in FORMS:
        sd = weights(wm)
        p = SRPipeline(41, device="cuda", dtype=a.dtype, weightmap=wm, use_act=act).load_state_dicts(*sd)
        ref = SRPipeline(41, device="cuda", dtype="fp32", weightmap=wm, use_act=act).load_state_dicts(*sd)
        with torch.no_grad():
            fine = p(*args)["fine"][2].cpu()
            fine32 = ref(*args)["fine"][2].cpu()
        del ref
        p.capture(*args)
        pipes[name] = p
        res[name] = {"form": name, "weightmap": wm, "use_act": act, "dtype": a.dtype, "batch": a.batch,
                     "psnr_fine256_vs_fp32_db": round(OL.psnr(fine, fine32), 2), "ms_per_step": []}
    for p in pipes.values():                           # warm every graph
        for _ in range(10):
            p.replay()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, p in pipes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                p.replay()
            e1.record()
            torch.cuda.synchronize()
            res[name]["ms_per_step"].append(round(e0.elapsed_time(e1) / a.steps, 4))
    for name in pipes:
        r = res[name]
        best = min(r["ms_per_step"])
        r["images_per_s_best"] = round(a.batch * 1000.0 / best, 1)
        r["vs_shipped_best"] = round(best / min(res["shipped"]["ms_per_step"]), 4)
        print(json.dumps(r))


if __name__ == "__main__":
    main()
