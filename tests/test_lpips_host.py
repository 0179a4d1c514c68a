"""Host: tgsr_amd/lpips.py without a GPU - the CPU path of LPIPS against the fp64 model of the definition (tests/lpips_model.py), the
three state-dict layouts, save / load, the refusals, and the slot planner's promise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_model as M          # noqa: E402
import vgg16_arch as A           # noqa: E402


def pair(B, H, W, seed, noise=0.2):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    y = (x + noise * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)
    return x, y


def test_the_restated_layer_list_is_the_modules():
    from tgsr_amd import lpips
    m = lpips.LPIPS()
    convs = [(i, mod.in_channels, mod.out_channels) for i, mod in enumerate(m.features) if isinstance(mod, torch.nn.Conv2d)]
    assert convs == [(i, cin, cout) for i, kind, cin, cout in A.layers() if kind == "conv"]
    assert len(m.features) == 30 and tuple(i for i, _a, _b in convs) == A.CONV_INDICES == (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
    assert [i for i, mod in enumerate(m.features) if isinstance(mod, torch.nn.MaxPool2d)] == [i for i, k, _a, _b in A.layers() if k == "pool"]
    assert lpips.TAPS == A.LPIPS_TAPS and lpips.WIDTHS == A.LPIPS_WIDTHS
    for mod in m.features:
        if isinstance(mod, torch.nn.Conv2d):
            assert mod.kernel_size == (3, 3) and mod.stride == (1, 1) and mod.padding == (1, 1) and mod.bias is not None
    assert sorted(m.state_dict()) == sorted(A.random_state(0)) and not any(p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("H,W", [(32, 32), (48, 40), (16, 19)])
def test_the_cpu_path_against_the_model(H, W):
    from tgsr_amd.lpips import LPIPS
    m = LPIPS.random(5)
    x, y = pair(2, H, W, 11)
    d, layers = m(x, y, per_layer=True)
    ref = M.distance(m.state_dict(), x, y, grad=True)
    assert d.dtype == torch.float32 and tuple(d.shape) == (2,) and tuple(layers.shape) == (5, 2)
    assert float(ref["d"].min()) > 0
    assert torch.allclose(d.double(), ref["d"], rtol=1e-4, atol=0) and torch.allclose(layers.double(), ref["per_layer"], rtol=1e-4, atol=0)
    assert torch.equal(m(x, y), d)
    assert float(m(x, x).abs().max()) == 0.0
    xg = x.clone().requires_grad_(True)
    m(xg, y).sum().backward()
    err = float((xg.grad.double() - ref["grad"]).norm() / ref["grad"].norm())
    assert err < 1e-4, err


def test_a_zero_column_gives_no_gradient_and_no_nan_in_the_model():
    g = torch.Generator().manual_seed(3)
    f0, f1 = torch.relu(torch.randn(1, 6, 2, 2, generator=g)), torch.relu(torch.randn(1, 6, 2, 2, generator=g))
    f0[0, :, 0, 0] = 0
    f1[0, :, 0, 1] = 0
    f0[0, :, 1, 1] = 0
    f1[0, :, 1, 1] = 0
    d, grad = M.tail64(f0, f1, torch.rand(6, generator=g))
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(grad).all())
    assert float(grad[0, :, 0, 0].abs().max()) == 0 and float(grad[0, :, 1, 1].abs().max()) == 0 and float(grad[0, :, 0, 1].abs().max()) > 0


def test_the_three_state_dict_layouts_load_to_the_same_module(tmp_path):
    from tgsr_amd.lpips import LPIPS
    src = LPIPS.random(7)
    own = src.state_dict()
    slices = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
    lins_file = {"lin%d.model.1.weight" % k: own["lin%d" % k] for k in range(5)}
    full = {"scaling_layer.shift": torch.tensor(M.SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(M.SCALE).view(1, 3, 1, 1)}
    for i, s in slices.items():
        for part in ("weight", "bias"):
            full["net.slice%d.%d.%s" % (s, i, part)] = own["features.%d.%s" % (i, part)]
    for k in range(5):
        full["lin%d.model.1.weight" % k] = full["lins.%d.model.1.weight" % k] = own["lin%d" % k]
    a, b, c = LPIPS(), LPIPS(), LPIPS()
    a.load_state_dict(own)
    b.load_state_dict({k: v for k, v in own.items() if k.startswith("features.")}, strict=False)
    b.load_state_dict(lins_file)                                    # the linear layers alone: the trunk keeps its weights
    c.load_state_dict(full)
    for m in (a, b, c):
        assert all(torch.equal(v, own[k]) for k, v in m.state_dict().items()) and sorted(m.state_dict()) == sorted(own)
    with pytest.raises(RuntimeError):
        LPIPS().load_state_dict({k: v for k, v in lins_file.items() if not k.startswith("lin4")})
    with pytest.raises(RuntimeError):
        LPIPS().load_state_dict(dict(own, extra=torch.zeros(1)))
    path = src.save(str(tmp_path / "lpips.pth"))
    assert path == str(tmp_path / "lpips.pth") and os.path.exists(path)
    back = LPIPS.load(path, device="cpu")
    assert all(torch.equal(v, own[k]) for k, v in back.state_dict().items())
    torch.save(full, str(tmp_path / "full.pth"))
    x, y = pair(1, 16, 16, 2)
    assert torch.equal(LPIPS.load(str(tmp_path / "full.pth"), device="cpu")(x, y), src(x, y))
    assert all(torch.equal(p, q) for p, q in zip(LPIPS.random(7).parameters(), src.parameters()))
    assert not all(torch.equal(p, q) for p, q in zip(LPIPS.random(8).parameters(), src.parameters()))


def test_refusals(tmp_path):
    from tgsr_amd.lpips import LPIPS, PerceptualScores
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import SRTrainer
    m = LPIPS.random(1)
    with pytest.raises(ValueError, match="16"):
        m(torch.zeros(1, 3, 15, 32), torch.zeros(1, 3, 15, 32))
    with pytest.raises(ValueError, match="16"):
        m(torch.zeros(1, 3, 32, 8), torch.zeros(1, 3, 32, 8))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 32, 32), torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 32, 32, dtype=torch.float64), torch.zeros(1, 3, 32, 32, dtype=torch.float64))
    with pytest.raises(ValueError, match="lpips"):
        PerceptualScores(3, "cpu")
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    try:
        torch.manual_seed(2)
        tr = SRTrainer(41, device="cpu")
        assert tr.perceptual is None and tr.perceptual_weight == 0.0
        for bad in (3, 0.5, True, {"w": 1}, [m]):
            with pytest.raises(ValueError, match="lpips"):
                tr.evaluate(iter(()), lpips=bad)
        with pytest.raises(FileNotFoundError):
            tr.evaluate(iter(()), lpips=str(tmp_path / "absent.pth"))
        for bad in (-1.0, float("nan"), float("inf"), "much", None):
            with pytest.raises(ValueError, match="perceptual"):
                SRTrainer(41, device="cpu", perceptual=(m, bad))
        for bad in (m, (m,), (m, 1.0, 2.0), (3, 1.0)):
            with pytest.raises(ValueError, match="perceptual"):
                SRTrainer(41, device="cpu", perceptual=bad)
    finally:
        cfg_reset()


def test_the_scores_accumulator_on_the_host():
    from tgsr_amd.lpips import LPIPS, PerceptualScores, quantised
    m = LPIPS.random(4)
    acc = PerceptualScores(m, "cpu")
    with pytest.raises(ValueError):
        acc.result()
    rows = []
    for k, B in enumerate((2, 1)):
        x, y = pair(B, 16, 24, 20 + k)
        acc.add(x, y)
        xq = torch.clamp((x + 1.0) * 127.5, 0, 255).round() / 127.5 - 1.0
        assert torch.equal(quantised(x), xq) and torch.equal(quantised(quantised(x)), xq)
        assert torch.equal(quantised(((x + 1.0) * 127.5).clamp(0, 255).round().to(torch.uint8)), xq)
        rows.append(m(quantised(x), quantised(y), per_layer=True))
    res = acc.result()
    assert sorted(res) == ["fine", "mean", "n", "per_layer"] and res["n"] == 3
    assert res["fine"].dtype == np.float64 and np.array_equal(res["fine"], torch.cat([r[0] for r in rows]).double().numpy())
    assert res["per_layer"].shape == (5, 3) and np.array_equal(res["per_layer"], torch.cat([r[1] for r in rows], 1).double().numpy())
    assert res["mean"] == float(np.mean(res["fine"]))


def test_nslots_is_what_the_docstring_promises():
    from tgsr_amd import ops
    for C, HW in ((64, 65536), (128, 16384), (256, 4096), (512, 1024), (512, 256), (1, 1), (67, 35), (64, 1025), (3, 32768 + 1), (8, 1 << 24)):
        tile = 16 if HW <= 1024 else 64
        tiles = -(-HW // tile)
        per = max(-(-tiles // 512), 4 if HW >= 32768 else 1)
        assert ops.lpips_nslots(C, HW) == -(-tiles // per) <= 512, (C, HW)
    assert [ops.lpips_nslots(64, hw) for hw in (147456, 65536, 16384, 16383, 4096, 1024, 256, 1)] == [461, 256, 256, 256, 64, 64, 16, 1]
    assert ops.lpips_nslots(0, 16) == 0 and ops.lpips_nslots(16, 0) == 0 and ops.lpips_nslots(-1, -1) == 0
