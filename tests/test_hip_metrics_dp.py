"""GPU: SRTrainer.evaluate under data parallelism, rehearsed as 2 ranks on ONE GPU (gloo; each rank a fresh child process with a
time limit of its own): each rank scores its half of four validation batches, the rows are gathered in rank order, both ranks
return the same dict, and its per-image rows are those of one process evaluating all four batches."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
KEYS = ("psnr", "rmse", "psnr_y", "rmse_y", "ssim_y")


def _run_ranks(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "ev")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "metrics_dp_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=420)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return [torch.load("%s.rank%d.pt" % (out, k), weights_only=False) for k in range(2)]


def test_two_ranks_return_the_one_process_evaluation(tmp_path):
    r = _run_ranks(tmp_path)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import metrics_dp_worker as W
    from tgsr_amd.miscc.config import cfg_reset
    try:
        tr = W.make_trainer("cuda:0")
        one = tr.evaluate(W.batches("cuda:0"), ema=True, shave=2)
    finally:
        cfg_reset()
    for name in ("fine", "fake"):
        assert len(r[0][name]) == len(r[1][name]) == len(one[name]) == 3
        for i in range(3):
            a, b, c = r[0][name][i], r[1][name][i], one[name][i]
            assert a["n"] == b["n"] == c["n"] == W.NBATCH * W.B
            for k in KEYS:
                assert a[k].tobytes() == b[k].tobytes(), (name, i, k)                     # both ranks: the same dict
                assert a["mean"][k] == b["mean"][k] == c["mean"][k]
                assert np.array_equal(a[k], c[k]), (name, i, k, a[k], c[k])              # rank order = batch order
            assert np.all(np.isfinite(a["psnr"])) and np.all(a["ssim_y"] < 1.0)
