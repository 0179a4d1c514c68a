"""GPU: CNN_ENCODER's Inception trunk in TRAINING mode on the library's kernels (pretrain_DAMSM.py:49-51, 70: the frozen trunk runs with
batch-statistics BatchNorm and its running statistics drift into the saved image encoder).  Each conv + BN + ReLU layer is
tgsr::gconv_stats (the raw convolution into its channel slice + per-channel statistics partials) followed by
tgsr::bn_train_relu_slice_from_stats (BN with the batch statistics + ReLU in place, running statistics updated): the operators against
fp64 torch, the whole walk against the same modules run by torch in float64 on the CPU, determinism, routing and DAMSMTrainer from
images against the torch-module trunk."""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tgsr_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()


def rel(a, b):
    b = b.double()
    return float((a.detach().cpu().double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# the layer kinds of test_hip_inception.GEOM (image layer, 1x1, 1x7 / 7x1, 5x5, stride 2, M > 128, split over K, ragged)
GEOM = [
    (2, 3, 39, 39, 32, 3, 3, 2, 0, 0),
    (2, 32, 19, 19, 32, 3, 3, 1, 0, 0),
    (2, 32, 17, 17, 64, 3, 3, 1, 1, 1),
    (3, 64, 9, 9, 80, 1, 1, 1, 0, 0),
    (2, 48, 12, 12, 64, 5, 5, 1, 2, 2),
    (2, 128, 17, 17, 128, 1, 7, 1, 0, 3),
    (2, 128, 17, 17, 192, 7, 1, 1, 3, 0),
    (2, 192, 17, 17, 320, 3, 3, 2, 0, 0),
    (4, 384, 8, 8, 384, 1, 3, 1, 0, 1),
    (4, 448, 8, 8, 384, 3, 3, 1, 1, 1),
    (4, 1280, 8, 8, 320, 1, 1, 1, 0, 0),
    (1, 5, 7, 11, 7, 3, 1, 1, 1, 0),
    (2, 288, 35, 35, 384, 3, 3, 2, 0, 0),
    (2, 96, 35, 35, 96, 3, 3, 2, 0, 0),
    (1, 3, 299, 299, 32, 3, 3, 2, 0, 0),
    (2, 192, 35, 35, 48, 1, 1, 1, 0, 0),
]


def test_geometries_cover_split_and_unsplit_reductions():
    from tgsr_amd import ops
    splits = [ops._lib.lib().tgsr_gconv_nsplit(Co, B * ((H + 2 * ph - kh) // st + 1) * ((W + 2 * pw - kw) // st + 1), Ci * kh * kw)
              for B, Ci, H, W, Co, kh, kw, st, ph, pw in GEOM]
    assert any(s > 1 for s in splits) and any(s == 1 for s in splits)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("B,Cin,H,W,Cout,kh,kw,st,ph,pw", GEOM)
def test_gconv_stats_and_bn_relu_slice(B, Cin, H, W, Cout, kh, kw, st, ph, pw, split):
    """The stats mode's raw slice is bit-identical to gconv without bias / ReLU in the same form; its partials sum to the fp64
    per-channel sums; the apply is relu(batch_norm(training=True)) with torch's running-statistics update; other channels untouched."""
    from tgsr_amd import custom_ops as C
    from tgsr_amd import ops
    was = ops.gconv_set_form(split)
    try:
        g = torch.Generator().manual_seed(Cin + 7 * Cout + kh)
        x = torch.rand(B, Cin, H, W, generator=g)                    # non-negative like the ReLU outputs the layers read
        w = torch.randn(Cout, Cin, kh, kw, generator=g) / (Cin * kh * kw) ** 0.5
        gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
        rm0, rv0 = 0.1 * torch.randn(Cout, generator=g), 0.5 + torch.rand(Cout, generator=g)
        xd = x.to(DEV)
        wu = C.gconv_pack(w.to(DEV), None, False)
        OH, OW = (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1
        K = Cin * kh * kw
        ws = torch.empty(max(ops.gconv_ws_elems(B, Cout, OH, OW, K), 1), device=DEV)
        plain = torch.full((B, Cout + 9, OH, OW), 7.0, device=DEV)
        C.gconv(False, wu, xd, 0, Cin, plain, 5, kh, kw, st, ph, pw, None, False, False, ws, None)
        out = torch.full((B, Cout + 9, OH, OW), 7.0, device=DEV)
        ns = ops.gconv_stats_nslots(B, Cout, OH, OW, K)
        part = torch.full((Cout, ns, 2), float("nan"), device=DEV)
        C.gconv_stats(wu, xd, 0, Cin, out, 5, kh, kw, st, ph, pw, ws, part)
        assert torch.equal(out, plain)                               # raw slice bit-identical, other channels untouched
        raw = out[:, 5:5 + Cout].cpu().double()
        assert rel(raw, F.conv2d(x.double(), w.double(), None, st, (ph, pw))) < 2e-5
        # (sum, sum of squared deviations from the slot's mean) per slot of spx pixels, combined by Chan's formula in fp64
        spx = ops.gconv_stats_slot_pixels(B, Cout, OH, OW, K)
        N = B * OH * OW
        nt = torch.tensor([min(spx, N - t * spx) for t in range(ns)], dtype=torch.float64)
        pc = part.cpu().double()
        s64 = pc[:, :, 0].sum(1)
        mean = s64 / N
        m2 = (pc[:, :, 1] + nt * (pc[:, :, 0] / nt - mean[:, None]) ** 2).sum(1)
        assert rel(s64, raw.sum((0, 2, 3))) < 1e-6
        assert rel(m2, (raw - raw.mean((0, 2, 3), keepdim=True)).square().sum((0, 2, 3))) < 1e-6
        for mom in (0.1, 0.37):
            y = out.clone()
            rm, rv = rm0.to(DEV), rv0.to(DEV)
            nbt = torch.tensor(3, dtype=torch.int64, device=DEV)
            stats = torch.empty(4, Cout, device=DEV)
            C.bn_train_relu_slice_from_stats(y, 5, gamma.to(DEV), beta.to(DEV), 1e-3, mom, rm, rv, nbt, part, spx, stats)
            rm_ref, rv_ref = rm0.double().clone(), rv0.double().clone()
            ref = F.relu(F.batch_norm(raw, rm_ref, rv_ref, gamma.double(), beta.double(), True, mom, 1e-3))
            assert rel(y[:, 5:5 + Cout], ref) < 2e-5
            assert rel(rm, rm_ref) < 2e-5 and rel(rv, rv_ref) < 2e-5
            assert int(nbt) == 4
            assert rel(stats[0], raw.mean((0, 2, 3))) < 2e-5
            assert bool((y[:, :5] == 7).all()) and bool((y[:, 5 + Cout:] == 7).all())
    finally:
        ops.gconv_set_form(was)


def test_new_operators_opcheck():
    from tgsr_amd import custom_ops as C
    from tgsr_amd import ops
    g = torch.Generator().manual_seed(3)
    B, Cin, H, W, Cout = 2, 32, 9, 9, 48
    x = torch.rand(B, Cin, H, W, generator=g).to(DEV)
    wu = C.gconv_pack(torch.randn(Cout, Cin, 3, 3, generator=g).to(DEV), None, False)
    out = torch.zeros(B, Cout + 4, H, W, device=DEV)
    ws = torch.empty(max(ops.gconv_ws_elems(B, Cout, H, W, Cin * 9), 1), device=DEV)
    part = torch.empty(Cout, ops.gconv_stats_nslots(B, Cout, H, W, Cin * 9), 2, device=DEV)
    torch.library.opcheck(C.gconv_stats, (wu, x, 0, Cin, out, 2, 3, 3, 1, 1, 1, ws, part))
    C.gconv_stats(wu, x, 0, Cin, out, 2, 3, 3, 1, 1, 1, ws, part)
    torch.library.opcheck(C.bn_train_relu_slice_from_stats,
                          (out, 2, torch.rand(Cout, device=DEV) + 0.5, torch.zeros(Cout, device=DEV), 1e-3, 0.1,
                           torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV),
                           part, ops.gconv_stats_slot_pixels(B, Cout, H, W, Cin * 9), torch.empty(4, Cout, device=DEV)))


def _encoder(seed):
    from inception_v3_arch import InceptionV3Arch
    from tgsr_amd.util import CNN_ENCODER
    enc = CNN_ENCODER(64, inception=InceptionV3Arch(seed=seed))
    for p in enc.frozen_parameters():
        p.requires_grad = False
    return enc


def _bns(enc):
    return [m for m in enc.modules() if isinstance(m, nn.BatchNorm2d)]


@pytest.fixture
def _cfg():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.TRAIN.FLAG = True
    yield cfg
    cfg_reset()


def test_train_mode_routing_and_no_torch_module_runs(_cfg, monkeypatch):
    enc = _encoder(3).train().to(DEV)
    img = torch.rand(2, 3, 128, 128, device=DEV) * 2 - 1
    assert enc._hip_trunk_ok(img)
    xg = img.clone().requires_grad_(True)
    assert not enc._hip_trunk_ok(xg)                                    # a gradient to the image: the torch modules
    with torch.no_grad():
        assert enc._hip_trunk_ok(xg)

    def boom(*a, **k):
        raise AssertionError("a torch module ran in the HIP train-mode walk")
    with monkeypatch.context() as m:
        m.setattr(nn.Conv2d, "forward", boom)
        m.setattr(nn.BatchNorm2d, "forward", boom)
        m.setattr(F, "batch_norm", boom)
        m.setattr(torch, "batch_norm", boom)
        with torch.no_grad():
            f, p = enc.run_trunk(img)
    assert tuple(f.shape) == (2, 768, 17, 17) and tuple(p.shape) == (2, 2048)
    assert all(int(bn.num_batches_tracked) == 1 for bn in _bns(enc))
    monkeypatch.setenv("TGSR_TRUNK", "torch")
    assert not enc._hip_trunk_ok(img)
    monkeypatch.delenv("TGSR_TRUNK")
    enc.Mixed_6b.branch7x7_2.bn.momentum = None
    assert not enc._hip_trunk_ok(img)


@pytest.mark.parametrize("B,H,W", [(4, 256, 256), (3, 240, 200)])
def test_whole_trunk_train_mode_against_the_modules_in_float64(_cfg, B, H, W):
    """Two consecutive training-mode batches: features, pooled code, every BatchNorm's running statistics and num_batches_tracked
    against the fp64 CPU walk of the same modules; then both in eval mode (the folded packs follow the drifted statistics).
    Batch-statistics BatchNorm over 94 layers is ill-conditioned at these batch sizes: torch's OWN fp32 walk of the same modules on
    the CPU lands ~1.7e-3 from fp64 at the outputs, so the HIP walk is held to 2e-4 or, where fp32 arithmetic itself
    cannot get there, to 1.5 x torch's fp32 margin on the same inputs."""
    enc = _encoder(2).train()
    ref = copy.deepcopy(enc).double()
    f32 = copy.deepcopy(enc)
    enc.to(DEV)
    g = torch.Generator().manual_seed(B + H)
    margins, fp32 = {}, {}

    def stat_margins(a_enc, step, into):
        into["running_mean%d" % step] = max(rel(a.running_mean, b.running_mean) for a, b in zip(_bns(a_enc), _bns(ref)))
        into["running_var%d" % step] = max(rel(a.running_var, b.running_var) for a, b in zip(_bns(a_enc), _bns(ref)))

    for step in range(2):
        img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
        with torch.no_grad():
            fr, pr = ref.run_trunk(img.double())
            fc, pc = f32.run_trunk(img)
            xd = img.to(DEV)
            assert enc._hip_trunk_ok(xd)
            fd, pd = enc.run_trunk(xd)
        margins["features%d" % step], margins["pooled%d" % step] = rel(fd, fr), rel(pd, pr)
        fp32["features%d" % step], fp32["pooled%d" % step] = rel(fc, fr), rel(pc, pr)
        stat_margins(enc, step, margins)
        stat_margins(f32, step, fp32)
        assert all(int(a.num_batches_tracked) == int(b.num_batches_tracked) == step + 1 for a, b in zip(_bns(enc), _bns(ref)))
    for m in (enc, ref, f32):
        m.eval()
    img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    with torch.no_grad():
        fr, pr = ref.run_trunk(img.double())
        fc, pc = f32.run_trunk(img)
        fd, pd = enc.run_trunk(img.to(DEV))
    margins["eval_features"], margins["eval_pooled"] = rel(fd, fr), rel(pd, pr)
    fp32["eval_features"], fp32["eval_pooled"] = rel(fc, fr), rel(pc, pr)
    fmt = lambda d: {k: "%.2e" % v for k, v in d.items()}                         # noqa: E731
    print("\ntrain-mode trunk margins against fp64 (B=%d, %dx%d)\n  hip:        %s\n  torch fp32: %s" % (B, H, W, fmt(margins),
                                                                                                 fmt(fp32)))
    bad = {k: (v, fp32[k]) for k, v in margins.items() if not (v < 2e-4 or v < 1.5 * fp32[k])}
    assert not bad, bad


def test_train_mode_walk_is_deterministic_across_streams_and_runs(_cfg):
    from tgsr_amd.inception import InceptionTrunk
    enc = _encoder(4).train().to(DEV)
    enc._hip_trunk = InceptionTrunk(enc)
    state = copy.deepcopy(enc.state_dict())
    img = torch.rand(4, 3, 192, 192, device=DEV) * 2 - 1

    def walk(nstreams):
        enc.load_state_dict(state)
        enc._hip_trunk.nstreams = nstreams
        with torch.no_grad():
            f, p = enc.run_trunk(img)
        assert len(enc._hip_trunk._streams) == nstreams
        return [f.clone(), p.clone()] + [t.clone() for bn in _bns(enc) for t in (bn.running_mean, bn.running_var)]

    one = walk(1)
    for _ in range(2):
        for a, b in zip(one, walk(4)):
            assert torch.equal(a, b)


def test_damsm_trainer_from_images_against_the_torch_trunk(_cfg, tmp_path, monkeypatch):
    from inception_v3_arch import InceptionV3Arch
    from tgsr_amd.train import DAMSMTrainer
    _cfg.TEXT.WORDS_NUM = 10
    B, lens = 8, [10, 9, 8, 7, 5, 4, 2, 1]
    g = torch.Generator().manual_seed(21)
    batches = []
    for _ in range(3):
        cap = torch.zeros(B, 10, dtype=torch.int64)
        for b, n in enumerate(lens):
            cap[b, :n] = torch.randint(1, 40, (n,), generator=g)
        batches.append(((torch.rand(B, 3, 256, 256, generator=g) * 2 - 1).to(DEV), cap.to(DEV), lens, None))

    def run(trunk_env):
        if trunk_env:
            monkeypatch.setenv("TGSR_TRUNK", trunk_env)
        else:
            monkeypatch.delenv("TGSR_TRUNK", raising=False)
        torch.manual_seed(0)
        tr = DAMSMTrainer(40, device=DEV, lr=2e-3, inception=InceptionV3Arch(seed=6))
        losses = []
        for i, bt in enumerate(batches):
            torch.manual_seed(100 + i)
            losses.append(float(tr.step(*bt)))
        return tr, losses

    tr_t, loss_t = run("torch")
    assert tr_t.image_encoder._hip_trunk is None
    tr_h, loss_h = run(None)
    assert tr_h.image_encoder._hip_trunk is not None
    # the same trainer with the torch modules walked in float64 on the CPU as its trunk (MIOpen's fp32 convolutions, which
    # TGSR_TRUNK=torch runs, are themselves ~1e-1 from fp64 at the trunk's outputs in training mode: DESIGN 3.6)
    monkeypatch.delenv("TGSR_TRUNK", raising=False)
    torch.manual_seed(0)
    tr_r = DAMSMTrainer(40, device=DEV, lr=2e-3, inception=InceptionV3Arch(seed=6))
    ref_enc = copy.deepcopy(tr_r.image_encoder).cpu().double().train()
    tr_r.image_encoder.run_trunk = lambda x: tuple(t.float().to(DEV) for t in ref_enc.run_trunk(x.detach().cpu().double()))
    loss_r = []
    for i, bt in enumerate(batches):
        torch.manual_seed(100 + i)
        loss_r.append(float(tr_r.step(*bt)))
    print("\nDAMSMTrainer losses from images: hip %s, fp64 trunk %s, TGSR_TRUNK=torch %s" % (loss_h, loss_r, loss_t))
    for a, b, c in zip(loss_h, loss_r, loss_t):
        assert abs(a - b) <= 2e-4 * abs(b), (loss_h, loss_r)
        assert abs(a - c) <= 5e-3 * abs(c), (loss_h, loss_t)
    for a, b in zip(_bns(tr_h.image_encoder), _bns(ref_enc)):
        assert rel(a.running_mean, b.running_mean) < 5e-4 and rel(a.running_var, b.running_var) < 5e-4
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 3
    for a, b in zip(_bns(tr_h.image_encoder), _bns(tr_t.image_encoder)):
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 3
    # snapshot / resume restores the drifted statistics
    _pi, pt = tr_h.snapshot(str(tmp_path), 1)
    tr2 = DAMSMTrainer(40, device=DEV, lr=2e-3, inception=InceptionV3Arch(seed=7))
    assert tr2.resume(pt) == 2
    for a, b in zip(_bns(tr2.image_encoder), _bns(tr_h.image_encoder)):
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
    # evaluate: the eval-mode HIP walk with the updated statistics, no torch module
    real_conv = nn.Conv2d.forward
    ran = []
    monkeypatch.setattr(nn.Conv2d, "forward", lambda self, x: (ran.append(1), real_conv(self, x))[1])
    s_h, w_h = tr_h.evaluate([(bt[0], bt[1], bt[2], bt[3]) for bt in batches[:2]])
    assert not ran and not tr_h.image_encoder.training
    ref_enc.eval()
    s_r, w_r = tr_r.evaluate([(bt[0], bt[1], bt[2], bt[3]) for bt in batches[:2]])
    assert abs(s_h - s_r) <= 2e-4 * abs(s_r) and abs(w_h - w_r) <= 2e-4 * abs(w_r), ((s_h, w_h), (s_r, w_r))
