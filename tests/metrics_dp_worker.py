"""Child process of tests/test_hip_metrics_dp.py: one data-parallel rank (gloo, every rank on cuda:0) that evaluates its share of
the validation batches with SRTrainer.evaluate.  Not a test module."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBATCH, B = 4, 2


def make_trainer(device="cuda:0"):
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import SRTrainer
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 64
    torch.manual_seed(1234)                                   # identical weights on every rank and in the one-process run
    tr = SRTrainer(41, device=device)
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():                                     # EMA weights that are not the current ones
        for a in tr.avg_param_G:
            a.add_((0.01 * torch.randn(a.shape, generator=g)).to(a.device))
    return tr


def batches(device="cuda:0", which=range(NBATCH)):
    """Validation batch k (LR 16 x 16 -> 32 / 64 / 128): the same tensors whoever builds them."""
    from oracle import tgsr_oracle as O
    for k in which:
        cap, lens, LR, LRb = O.synthetic_batch(B, lr=16, seed=300 + k)
        g = torch.Generator().manual_seed(400 + k)
        hr = [(torch.rand(B, 3, 16 * s, 16 * s, generator=g) * 2 - 1).to(device) for s in (2, 4, 8)]
        yield cap.to(device), lens.tolist(), LR.to(device), LRb.to(device), hr


def main():
    out = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    tr = make_trainer()
    per = NBATCH // world
    res = tr.evaluate(batches(which=range(rank * per, (rank + 1) * per)), ema=True, shave=2)
    torch.cuda.synchronize()
    torch.save(res, "%s.rank%d.pt" % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
