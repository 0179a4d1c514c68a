"""CPU: the attention-guided objectives (miscc.losses.weight_MSE / words_reweight_loss / generator_re_weight_loss) on CPU tensors -
their torch compositions - against tests/golden/attn_losses.npz (the reference's own functions, make_attn_losses_golden.py), the
host checks of the new ops wrappers, the drop-in import line and SRTrainer's refusals."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from attn_losses_cases import u8_image, wmse_inputs
from conftest import GOLDEN, ROOT, load_npz

TOL = 2e-5          # the bound test_damsm_words_and_sent_loss_golden holds the DAMSM losses to


@pytest.fixture(scope="module")
def golden():
    return load_npz("attn_losses.npz")


@pytest.fixture()
def cfg_golden(golden):
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    sm = cfg.TRAIN.SMOOTH
    sm.GAMMA1, sm.GAMMA2, sm.GAMMA3 = (float(v) for v in golden["gamma"])
    sm.LAMBDA = float(load_npz("gan_losses.npz")["lambda"])
    yield cfg
    cfg_reset()


def _close(a, ref, what):
    ref = torch.from_numpy(np.asarray(ref))
    scale = max(1.0, float(ref.abs().max()))
    err = float((a.detach().cpu() - ref).abs().max())
    assert err <= TOL * scale, (what, err, scale)


def test_attention_loss_names_import_through_the_dropin():
    code = """
        import tgsr_amd
        tgsr_amd.install_dropin()
        from miscc.losses import weight_MSE, words_reweight_loss, generator_re_weight_loss
        import miscc.losses
        assert miscc.losses.__name__ == "tgsr_amd.miscc.losses" and callable(weight_MSE)
        print("ok")
    """
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd="/", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["wmse", "wmse1"])
def test_weight_mse_reproduces_the_reference_on_cpu(golden, name):
    from tgsr_amd.miscc import losses
    g = golden
    fake, label, att = wmse_inputs(g, name)
    for t in fake + label + att:
        t.requires_grad_(True)
    loss, wlast = losses.weight_MSE(fake, label, att)
    _close(loss, g[name + ".loss"], "loss")
    assert torch.equal(wlast.detach(), torch.from_numpy(g[name + ".wlast"]))
    loss.backward()
    for i in range(len(fake)):
        _close(fake[i].grad, g["%s.g_fake%d" % (name, i)], "d_fake%d" % i)
        _close(label[i].grad, -g["%s.g_fake%d" % (name, i)], "d_label%d" % i)
        _close(att[i].grad, g["%s.g_att%d" % (name, i)], "d_att%d" % i)


def test_weight_mse_takes_any_ratio_through_the_composition():
    from tgsr_amd.miscc import losses
    g = torch.Generator().manual_seed(3)
    f, l = torch.randn(1, 3, 7, 9, generator=g), torch.randn(1, 3, 7, 9, generator=g)
    a = torch.softmax(torch.randn(1, 4, 3, 4, generator=g), 1)
    loss, wlast = losses.weight_MSE([f], [l], [a])
    wups = F.interpolate(a.max(1, keepdim=True)[0], size=(7, 9))
    assert torch.equal(wlast, wups)
    assert torch.allclose(loss, (4 * wups * (f - l) ** 2).sum() / f.numel(), rtol=1e-6)


def test_words_reweight_loss_reproduces_the_reference_on_cpu(golden, cfg_golden):
    from tgsr_amd.miscc import losses
    g = golden
    lens = g["wrw.cap_lens"].tolist()
    attn = torch.from_numpy(g["wrw.attn"])
    conf = losses.attn_confidence(attn, lens)
    _close(conf, g["wrw.conf"], "conf")
    assert float(conf[2].abs().max()) == 0 and float(conf[1, 5]) == 0
    for tag, cls in (("cls", g["wrw.class_ids"]), ("nocls", None)):
        feats = (torch.from_numpy(g["wrw.feats.i8"]).float() / 4.0).requires_grad_(True)
        words = torch.from_numpy(g["wrw.words"]).requires_grad_(True)
        # the maps as a tensor and as a list of per-image maps
        for maps in (attn, [attn[i:i + 1] for i in range(3)]):
            w0, w1, att = losses.words_reweight_loss(feats, words, torch.arange(3), torch.tensor(lens), cls, 3, maps)
            _close(w0, g["wrw.%s.w0" % tag], tag + ".w0")
            _close(w1, g["wrw.%s.w1" % tag], tag + ".w1")
        for i, a in enumerate(att):
            _close(a.reshape(1, a.shape[1], -1)[:, :, ::2], g["wrw.att_map%d.sub2" % i], "att_map%d" % i)
        (w0 + w1).backward()
        _close(words.grad, g["wrw.%s.g_words" % tag], tag + ".g_words")
        _close(feats.grad[:, ::16], g["wrw.%s.g_feats.sub16" % tag], tag + ".g_feats")
        assert bool(torch.isfinite(w0)) and bool(torch.isfinite(w1)) and float(words.grad[2].abs().max()) == 0


def test_confidence_composition_keeps_the_kernels_rules():
    """The torch composition against the fp64 model the kernel is held to: the planted values at and just above float32(4 / n), zeros
    behind a caption's length, a zero row for a length outside [1, T]."""
    from attn_losses_cases import confidence_fp64, confidence_maps
    from tgsr_amd.miscc import losses
    for lens in ((6, 4, 5), (0, 7, 3)):
        att = confidence_maps(3, 6, 64, lens, seed=1)
        got = losses.attn_confidence(torch.from_numpy(att), lens).double().numpy()
        np.testing.assert_allclose(got, confidence_fp64(att, lens), rtol=1e-5, atol=0)


def test_generator_re_weight_loss_reproduces_the_reference_on_cpu(golden, cfg_golden):
    """On the plain-torch discriminators and the stub encoder of gan_losses.npz (tests/golden/make_golden.py builds the former)."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden
    finally:
        sys.path.remove(GOLDEN)
    from tgsr_amd.miscc import losses
    g, gan = golden, load_npz("gan_losses.npz")
    T = lambda k: torch.from_numpy(np.asarray(gan[k]))                               # noqa: E731
    ds = []
    for k in range(2):
        d = make_golden._plain_d_net(int(gan["ndf"]), int(gan["nef"]), k, torch.Generator().manual_seed(0))
        d.load_state_dict({n[3:]: T(n) for n in gan if n.startswith("D%d." % k)}, strict=True)
        ds.append(d.train())
    enc = lambda x: (F.conv2d(F.adaptive_avg_pool2d(x, 17), T("enc.f.weight"), T("enc.f.bias")),          # noqa: E731
                     F.linear(x.mean((2, 3)), T("enc.p.weight"), T("enc.p.bias")))
    fakes = [u8_image(gan, "fake%d.u8" % k).requires_grad_(True) for k in range(2)]
    sent, words = T("sent").requires_grad_(True), T("words").requires_grad_(True)
    attn = torch.from_numpy(g["grw.attn"])
    rl, ml = torch.ones(3), torch.arange(3)
    errG, log = losses.generator_re_weight_loss(ds, enc, fakes, rl, words, sent, ml, gan["cap_lens"].tolist(), gan["class_ids"],
                                                attn=attn)
    _close(errG, g["grw.errG"], "errG")
    num = r"-?\d+\.\d{5}"
    ref_log = str(g["grw.logs"])
    assert isinstance(log, str) and re.sub(num, "#", log) == re.sub(num, "#", ref_log), (log, ref_log)
    for a_, b_ in zip(re.findall(num, log), re.findall(num, ref_log)):
        assert abs(float(a_) - float(b_)) <= 2e-5 * max(1.0, abs(float(b_))) + 1e-5, (log, ref_log)       # five printed decimals
    errG.backward()
    _close(fakes[0].grad[:, :, ::8, ::8], g["grw.gG.fake0.sub8"], "g fake0")
    _close(fakes[1].grad[:, :, ::16, ::16], g["grw.gG.fake1.sub16"], "g fake1")
    _close(sent.grad, g["grw.gG.sent"], "g sent")
    _close(words.grad, g["grw.gG.words"], "g words")
    err2, _ = losses.generator_re_weight_loss(ds, enc, [f.detach() for f in fakes], rl, words, sent, ml, gan["cap_lens"].tolist(),
                                              None, w=0.5, s=2.0, g=3.0, attn=attn)
    _close(err2, g["grw.errG.nocls.w05.s2.g3"], "errG nocls")
    with pytest.raises(ValueError, match="attn"):
        losses.generator_re_weight_loss(ds, enc, fakes, rl, words, sent, ml, gan["cap_lens"].tolist(), None)


def test_ops_wrappers_refuse_on_the_host_with_messages():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    f, a = torch.zeros(2, 3, 6, 10), torch.zeros(2, 5, 3, 5)
    assert ops.check_weight_mse(f.shape, f.shape, a.shape) == (2, 3, 5, 6, 10, 3, 5, 2)
    cases = [
        ("no integer ratio", lambda: ops.weight_mse(f, f, torch.zeros(2, 5, 4, 5))),
        ("no integer ratio", lambda: ops.weight_mse(f, f, torch.zeros(2, 5, 3, 10))),           # r = 2 down, 1 across
        ("at most 255", lambda: ops.weight_mse(f, f, torch.zeros(2, 256, 3, 5))),
        ("float32", lambda: ops.weight_mse(f.double(), f, a)),
        ("float32", lambda: ops.weight_mse(f, f, a.half())),
        ("differ in shape", lambda: ops.weight_mse(f, torch.zeros(2, 3, 6, 12), a)),
        ("2 images against the maps of 3", lambda: ops.weight_mse(f, f, torch.zeros(3, 5, 3, 5))),
        (r"\[B, T, h, w\]", lambda: ops.weight_mse(f, f, torch.zeros(2, 5, 15))),
        ("empty", lambda: ops.weight_mse(torch.zeros(0, 3, 6, 10), torch.zeros(0, 3, 6, 10), a)),
        ("only on HIP tensors", lambda: ops.weight_mse(f, f, a)),
        ("uint8", lambda: ops.weight_mse_bwd(torch.ones(()), f, f, torch.zeros(2, 3, 5), torch.zeros(2, 3, 5), 5)),
        ("one float32 value", lambda: ops.weight_mse_bwd(torch.ones(2), f, f, torch.zeros(2, 3, 5), torch.zeros(2, 3, 5, dtype=torch.uint8), 5)),
        ("at most 255", lambda: ops.weight_mse_bwd(torch.ones(()), f, f, torch.zeros(2, 3, 5), torch.zeros(2, 3, 5, dtype=torch.uint8), 300)),
        ("no integer ratio", lambda: ops.weight_mse_bwd(torch.ones(()), f, f, torch.zeros(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.uint8), 5)),
        ("no gradient asked for", lambda: ops.weight_mse_bwd(torch.ones(()), f, f, torch.zeros(2, 3, 5), torch.zeros(2, 3, 5, dtype=torch.uint8),
                                                             5, need_fake=False)),
        ("only on HIP tensors", lambda: ops.weight_mse_bwd(torch.ones(()), f, f, torch.zeros(2, 3, 5), torch.zeros(2, 3, 5, dtype=torch.uint8), 5)),
        ("float32", lambda: ops.attn_confidence(torch.zeros(2, 5, 9, dtype=torch.float64), torch.zeros(2, dtype=torch.int32))),
        (r"int32 \[2\]", lambda: ops.attn_confidence(torch.zeros(2, 5, 9), torch.tensor([1, 2]))),
        (r"int32 \[2\]", lambda: ops.attn_confidence(torch.zeros(2, 5, 9), torch.zeros(3, dtype=torch.int32))),
        ("at most 65535 of 255", lambda: ops.attn_confidence(torch.zeros(2, 256, 9), torch.zeros(2, dtype=torch.int32))),
        ("only on HIP tensors", lambda: ops.attn_confidence(torch.zeros(2, 5, 9), torch.zeros(2, dtype=torch.int32))),
    ]
    for text, call in cases:
        with pytest.raises(TgsrError, match=text):
            call()
    for op, args in ((torch.ops.tgsr.attn_confidence, (torch.zeros(2, 5, 9), torch.zeros(2, dtype=torch.int32))),
                     (torch.ops.tgsr.weight_mse, (f, f, a, False))):
        with pytest.raises(TgsrError, match="CPU tensors"):
            op(*args)


def test_srtrainer_refuses_what_the_new_options_cannot_do(monkeypatch):
    from tgsr_amd import train
    with pytest.raises(ValueError, match="pixel_loss"):
        train.SRTrainer(10, device="cpu", pixel_loss="l1")
    with pytest.raises(ValueError, match="image_encoder"):
        train.SRTrainer(10, device="cpu", reweight=True)
    monkeypatch.setattr(train, "dp_world", lambda: 2)
    with pytest.raises(ValueError, match="confidences gathered"):
        train.SRTrainer(10, device="cpu", reweight=True, gather_negatives=True, image_encoder=torch.nn.Identity())
