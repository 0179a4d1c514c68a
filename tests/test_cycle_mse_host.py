"""CPU: the cycle-consistency objective (miscc.losses.CycleMSE) on CPU tensors - its torch composition - against
tests/golden/cycle_mse.npz (the reference's own function, make_cycle_mse_golden.py), the host checks of the new ops wrappers, the
drop-in import line, SRTrainer's refusal and the header's documentation of the three C entries."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import ROOT, load_npz
from cycle_mse_cases import FIXTURE_CASES, cycle_mse_fp64, fixture_inputs

RTOL = 1e-6         # the composition is the reference's arithmetic on the same torch build


@pytest.fixture(scope="module")
def golden():
    return load_npz("cycle_mse.npz")


def _close(a, ref, what):
    a, ref = a.detach().double(), torch.from_numpy(np.asarray(ref)).double()
    err, scale = float((a - ref).abs().max()), float(ref.abs().max())
    assert err <= RTOL * scale, (what, err, scale)


def test_cycle_mse_imports_through_the_dropin():
    code = """
        import tgsr_amd
        tgsr_amd.install_dropin()
        from miscc.losses import CycleMSE
        import miscc.losses
        assert miscc.losses.__name__ == "tgsr_amd.miscc.losses" and callable(CycleMSE)
        print("ok")
    """
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd="/", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_cycle_mse_reproduces_the_reference_on_cpu(golden, name):
    from tgsr_amd.miscc import losses
    g = golden
    srs, lr = fixture_inputs(g, name)
    for t in srs + [lr]:
        t.requires_grad_(True)
    loss = losses.CycleMSE(srs, lr)
    _close(loss, g[name + ".loss"], "loss")
    loss.backward()
    for i, s in enumerate(srs):
        _close(s.grad, g["%s.g_sr%d" % (name, i)], "d_sr%d" % i)
        _close(losses.CycleMSE([s.detach()], lr.detach(), fused=False), g[name + ".terms"][i], "term%d" % i)
    _close(lr.grad, g[name + ".g_lr"], "d_lr")
    # the fixture itself sits where the issue's table puts the reference: within 1e-5 of the fp64 model
    l64, t64, _gs, _gl = cycle_mse_fp64(srs, lr)
    assert abs(float(g[name + ".loss"]) - float(l64)) <= 1e-5 * float(l64)
    np.testing.assert_allclose(g[name + ".terms"], t64.numpy(), rtol=1e-5)


def test_check_cycle_mse_names_each_refusal():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    lr = torch.zeros(2, 3, 4, 5)
    sr = [torch.zeros(2, 3, 8, 10), torch.zeros(2, 3, 10, 14)]
    assert ops.check_cycle_mse([s.shape for s in sr], lr.shape) == (2, 2, 3, 4, 5, (8, 10, 10, 14))
    g, d = torch.ones(()), torch.zeros(2, 2, 3, 4, 5)
    cases = [
        ("0 scales", lambda: ops.check_cycle_mse([], lr.shape)),
        ("9 scales", lambda: ops.check_cycle_mse([sr[0].shape] * 9, lr.shape)),
        (r"lr \[B, C, h, w\]", lambda: ops.check_cycle_mse([sr[0].shape], (2, 3, 4))),
        (r"lr \[B, C, h, w\]", lambda: ops.check_cycle_mse([sr[0].shape], (2, 3, 0, 5))),
        (r"sr\[1\] \[B, C, H, W\]", lambda: ops.check_cycle_mse([sr[0].shape, (2, 3, 8)], lr.shape)),
        (r"sr\[0\] \[B, C, H, W\]", lambda: ops.check_cycle_mse([(2, 3, 0, 10)], lr.shape)),
        (r"sr\[1\].*differ in batch or channels", lambda: ops.check_cycle_mse([sr[0].shape, (2, 1, 8, 10)], lr.shape)),
        (r"sr\[0\].*differ in batch or channels", lambda: ops.check_cycle_mse([(1, 3, 8, 10)], lr.shape)),
        ("at most 65536", lambda: ops.check_cycle_mse([(2, 3, 65537, 1)], lr.shape)),
        ("float32", lambda: ops.cycle_mse([sr[0].double()], lr)),
        ("float32", lambda: ops.cycle_mse(sr, lr.half())),
        ("empty", lambda: ops.cycle_mse([torch.zeros(2, 3, 0, 10)], lr)),
        ("9 scales", lambda: ops.cycle_mse([sr[0]] * 9, lr)),
        ("only on HIP tensors", lambda: ops.cycle_mse(sr, lr)),
        ("one float32 value", lambda: ops.cycle_mse_bwd(torch.ones(2), d, (8, 10, 10, 14))),
        ("one float32 value", lambda: ops.cycle_mse_bwd(torch.ones((), dtype=torch.float64), d, (8, 10, 10, 14))),
        (r"\[n, B, C, h, w\]", lambda: ops.cycle_mse_bwd(g, d[0], (8, 10))),
        ("3 sizes for the 2 scales", lambda: ops.cycle_mse_bwd(g, d, (8, 10, 10))),
        ("1 need_sr flags for 2 scales", lambda: ops.cycle_mse_bwd(g, d, (8, 10, 10, 14), [True])),
        ("no gradient asked for", lambda: ops.cycle_mse_bwd(g, d, (8, 10, 10, 14), [False, False], False)),
        (r"sr\[1\] \[B, C, H, W\]", lambda: ops.cycle_mse_bwd(g, d, (8, 10, 0, 14))),
        ("only on HIP tensors", lambda: ops.cycle_mse_bwd(g, d, (8, 10, 10, 14))),
    ]
    for text, call in cases:
        with pytest.raises(TgsrError, match=text):
            call()
    for op, args in ((torch.ops.tgsr.cycle_mse, (sr, lr)), (torch.ops.tgsr.cycle_mse_bwd, (g, d, [8, 10, 10, 14], [True, True], False))):
        with pytest.raises(TgsrError, match="CPU tensors"):
            op(*args)


def test_cycle_mse_takes_the_composition_where_the_kernels_do_not_apply():
    """CPU tensors, float64 and fused=False all reach the reference's expression; fused=True on CPU tensors is an error, not a
    quiet fall-back."""
    import torch.nn.functional as F
    from tgsr_amd.miscc import losses
    from tgsr_amd._lib import TgsrError
    g = torch.Generator().manual_seed(4)
    sr, lr = [torch.randn(1, 2, 7, 9, generator=g), torch.randn(1, 2, 3, 2, generator=g)], torch.randn(1, 2, 4, 3, generator=g)
    want = sum(F.mse_loss(F.interpolate(s, size=[4, 3], mode="bicubic"), lr) for s in sr)
    assert torch.equal(losses.CycleMSE(sr, lr), want) and torch.equal(losses.CycleMSE(sr, lr, fused=False), want)
    assert losses.CycleMSE([s.double() for s in sr], lr.double()).dtype == torch.float64
    with pytest.raises(TgsrError, match="HIP tensors"):
        losses.CycleMSE(sr, lr, fused=True)


def test_srtrainer_refuses_a_negative_cycle_weight():
    from tgsr_amd import train
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cycle"):
            train.SRTrainer(10, device="cpu", cycle=bad)
    tr = train.SRTrainer(10, device="cpu")
    assert tr.cycle == 0.0 and tr._lr_in is None


def test_header_documents_the_three_entries():
    src = open(os.path.join(ROOT, "include", "tgsr_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", src, flags=re.S))
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("tgsr_cycle_mse_ws_elems", "tgsr_cycle_mse_fwd", "tgsr_cycle_mse_bwd"):
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
        assert name in comments, name + " is not documented"
    for word in ("TGSR_EINVAL", "bicubic", "No atomics", "ON THE DEVICE"):
        assert word in comments[comments.index("tgsr_cycle_mse_fwd -") - 2000:comments.index("tgsr_cycle_mse_fwd -") + 3000], word
