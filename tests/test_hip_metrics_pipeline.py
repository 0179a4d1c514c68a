"""GPU: the callers of the image-quality kernels - SRPipeline.score / from_modules and SRTrainer.evaluate / snapshot / resume.
Scores are held to the numpy model applied to the images the pipeline itself returned (SSE exact, SSIM within 1e-9: see
tests/test_hip_metrics.py); what a trainer looks like after an evaluation is held to a twin that never evaluated, bit for bit."""
import numpy as np
import pytest
import torch

from conftest import load_npz, split_sd
from oracle import tgsr_oracle as O

import metrics_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("psnr", "rmse", "psnr_y", "rmse_y", "ssim_y")


@pytest.fixture
def cfg_face():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 256
    cfg.TREE.BRANCH_NUM = 4
    yield cfg
    cfg_reset()


def _check_scores(sc, img, hr, shave):
    """`sc` (image_scores' dict) against the model on the returned image `img` and ground truth `hr` (host arrays)."""
    from tgsr_amd.metrics import psnr_from_sse
    s_rgb, s_y, ss, (pixels, windows) = M.rows(img, hr, shave)
    for i in range(len(s_rgb)):
        p, r = psnr_from_sse(s_rgb[i], 3 * pixels)
        py, ry = psnr_from_sse(s_y[i], pixels)
        assert sc["rmse"][i] == r and sc["psnr"][i] == p, (i, sc["rmse"][i], r)              # exact SSE <=> these bits
        assert sc["rmse_y"][i] == ry and sc["psnr_y"][i] == py, (i, sc["rmse_y"][i], ry)
        assert abs(sc["ssim_y"][i] - ss[i] / windows) <= 1e-9, (i, sc["ssim_y"][i], ss[i] / windows)
    for k in KEYS:
        assert sc[k].dtype == np.float64 and sc[k].shape == (len(s_rgb),)


def _check_pipeline_score(pipe, args, hr_pyramid, shave):
    out = pipe(*args)
    res = pipe.score(out, hr_pyramid, shave)
    assert sorted(res) == ["fake", "fine"]
    for name in ("fine", "fake"):
        assert len(res[name]) == len(hr_pyramid)
        for k, hr in enumerate(hr_pyramid):
            assert out[name][k].dtype == torch.float32
            _check_scores(res[name][k], out[name][k].cpu().numpy(), hr.cpu().numpy(), shave)
    return res


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_on_the_face_checkpoint(dtype, face_c1, face_weights, cfg_face):
    from tgsr_amd.trainer import SRPipeline
    g, io = face_c1, load_npz("io_pyramid.npz")
    pipe = SRPipeline(41, device=DEV, low="lr", dtype=dtype)
    pipe.load_state_dicts(split_sd(face_weights, "E."), split_sd(face_weights, "GL."), split_sd(face_weights, "GH."))
    args = (torch.from_numpy(g["captions"]).to(DEV), g["cap_lens"].tolist(), torch.from_numpy(g["LR"]).to(DEV),
            torch.from_numpy(g["LRb"]).to(DEV))
    assert g["LR"].shape[0] == 2
    hr_u8 = [torch.from_numpy(np.stack([io["ret%d_u8" % k], io["bic%d_u8" % k]])).to(DEV) for k in (1, 2, 3)]
    hr_f = [torch.from_numpy(M.loader_normalise(h.cpu().numpy())).to(DEV) for h in hr_u8]
    a = _check_pipeline_score(pipe, args, hr_u8, 0)
    b = _check_pipeline_score(pipe, args, hr_f, 0)              # a float pyramid scores exactly as its source bytes
    for name in ("fine", "fake"):
        for k in range(3):
            for key in KEYS:
                assert np.array_equal(a[name][k][key], b[name][k][key])
    _check_pipeline_score(pipe, args, hr_f, 4)
    with pytest.raises(ValueError):
        pipe.score(pipe(*args), hr_f[:2])


def test_score_on_a_x16_pipeline_with_random_weights(cfg_face):
    from tgsr_amd import models16
    from tgsr_amd.synthetic import random_init_
    from tgsr_amd.trainer import SRPipeline
    sdE, _, _ = O.random_state(seed=2)
    pipe = SRPipeline(41, device=DEV, branch_num=5)
    assert isinstance(pipe.netGL, models16.G_SR_NET_low)
    random_init_(pipe.netGL, 5), random_init_(pipe.netGH, 6)
    pipe.text_encoder.load_state_dict(sdE)
    pipe.invalidate_caches()
    cap, lens, LR, LRb = O.synthetic_batch(2, lr=16, seed=9)
    g = torch.Generator().manual_seed(3)
    hr = [(torch.rand(2, 3, 16 * s, 16 * s, generator=g) * 2 - 1).to(DEV) for s in (2, 4, 8, 16)]
    _check_pipeline_score(pipe, (cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV)), hr, 0)
    # from_modules over the same modules: the x16 generators are recognised, the same images, the same scores
    again = SRPipeline.from_modules(pipe.text_encoder, pipe.netGL, pipe.netGH)
    assert again.branch_num != 4 and again.netGL is pipe.netGL and again.device == next(pipe.netGL.parameters()).device
    o1 = pipe(cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV))
    o2 = again(cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV))
    for x, y in zip(o1["fine"], o2["fine"]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(gan, graphs, seed=5):
    from tgsr_amd import train
    from tgsr_amd.miscc.config import cfg
    cfg.GAN.DF_DIM = 8
    torch.manual_seed(seed)
    tr = train.SRTrainer(41, device=DEV, discriminators=gan)
    assert tr._graph_capable and tr._packs is not None
    tr._graph_g = graphs
    if not graphs:
        tr._dsteps = -10 ** 9                                # the discriminator updates stay eager too
    return tr


def _train_batch(step, B=4):
    cap, lens, _LR, LRb = O.synthetic_batch(B, seed=40 + step % 2)
    g = torch.Generator().manual_seed(step)
    LR = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).to(DEV) for s in (64, 128, 256)]
    return cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), hr


def _val_batches(n=2, B=2):
    for k in range(n):
        cap, lens, LR, LRb = O.synthetic_batch(B, seed=70 + k)
        g = torch.Generator().manual_seed(80 + k)
        hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).to(DEV) for s in (64, 128, 256)]
        yield cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), hr


def _state(tr):
    nets = [tr.netGL, tr.netGH] + list(tr.netsD)
    return [(k, v) for m in nets for k, v in m.state_dict().items()]


def _assert_twins(a, b):
    for (ka, va), (_kb, vb) in zip(_state(a), _state(b)):
        assert torch.equal(va, vb), ka
    for x, y in zip(a.avg_param_G, b.avg_param_G):
        assert torch.equal(x, y)
    for x, y in zip(a.params, b.params):
        assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize("gan", [False, True], ids=["g", "gd"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
def test_evaluate_leaves_the_trainer_as_it_was(graphs, gan, cfg_face):
    """Twins from one initialisation take the same steps; one evaluates (EMA weights, then the current ones) before the last
    step.  Eager: three steps, the evaluation between steps 2 and 3.  Replayed: the warm-up steps in front, so that the last
    steps - and the one behind the evaluation - are replays of the captured update."""
    from tgsr_amd import train
    nsteps = 3 + (train.GRAPH_G_WARMUP if graphs else 0)
    twins = [_trainer(gan, graphs), _trainer(gan, graphs)]
    losses = [[], []]
    for step in range(nsteps):
        batch = _train_batch(step)
        for k, tr in enumerate(twins):
            if k == 0 and step == nsteps - 1:
                ptrs = [p.data_ptr() for p in tr.params]
                before = [v.clone() for _k, v in _state(tr)] + [a.clone() for a in tr.avg_param_G]
                modes = (tr.netGL.training, tr.netGH.training)
                res = tr.evaluate(_val_batches(), ema=True, shave=4)
                res_cur = tr.evaluate(_val_batches(), ema=False, max_batches=1)
                assert [p.data_ptr() for p in tr.params] == ptrs
                assert (tr.netGL.training, tr.netGH.training) == modes == (True, True)
                after = [v for _k, v in _state(tr)] + list(tr.avg_param_G)
                assert all(torch.equal(x, y) for x, y in zip(before, after))
                assert res["fine"][2]["n"] == 4 and res_cur["fine"][2]["n"] == 2 and len(res["fake"]) == 3
                assert np.all(np.isfinite(res["fine"][2]["psnr"]))
                assert not np.array_equal(res["fine"][2]["psnr"][:2], res_cur["fine"][2]["psnr"])   # EMA != current weights
            torch.manual_seed(100 + step)
            losses[k].append(float(tr.step(*batch)))
    torch.cuda.synchronize()
    assert losses[0] == losses[1], losses
    _assert_twins(twins[0], twins[1])
    if graphs:
        for tr in twins:
            caps = list(tr._ggraphs.values())
            assert caps and all(isinstance(c, dict) for c in caps), "the update was not captured: %r" % (caps,)
    else:
        assert not twins[0]._ggraphs


@pytest.mark.parametrize("ema", [True, False], ids=["ema", "current"])
def test_evaluate_equals_a_fresh_pipeline_on_the_snapshot(ema, tmp_path, cfg_face):
    from tgsr_amd.metrics import ScoreBook  # noqa: F401
    from tgsr_amd.trainer import SRPipeline
    tr = _trainer(False, False)
    for step in range(2):
        torch.manual_seed(100 + step)
        tr.step(*_train_batch(step))
    res = tr.evaluate(_val_batches(), ema=ema, shave=0)
    pl, ph = tr.snapshot(str(tmp_path / "model"), 7, ema=ema)
    pipe = SRPipeline(41, device=DEV, low="lr", branch_num=4)
    pipe.load_state_dicts(tr.text_encoder.state_dict(), torch.load(pl, map_location=DEV), torch.load(ph, map_location=DEV))
    at = 0
    for cap, lens, LR, LRb, hr in _val_batches():
        sc = pipe.score(pipe(cap, lens, LR, LRb), hr, 0)
        B = LR.shape[0]
        for name in ("fine", "fake"):
            for k in range(3):
                for key in KEYS:
                    got = res[name][k][key][at:at + B]
                    assert got.tobytes() == sc[name][k][key].tobytes(), (name, k, key, got, sc[name][k][key])
        at += B
    assert res["fine"][0]["n"] == at
    for name in ("fine", "fake"):
        for k in range(3):
            for key in KEYS:
                assert res[name][k]["mean"][key] == float(np.mean(res[name][k][key]))


def _same_entry(a, b, path):
    """Arrays and tensors element for element (NaNs in the same places), everything else ==."""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            _same_entry(a[k], b[k], path + (k,))
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_entry(x, y, path + (i,))
    elif torch.is_tensor(a):
        assert torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), path
    else:
        assert a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), (path, a, b)


def test_evaluate_with_every_score_is_one_call_per_score(cfg_face):
    """One call with r_precision, fid, kid and niqe returns, entry by entry, what the plain call and the four calls with one of
    them each return, and leaves the trainer as it was.  LR 32 gives 64 / 128 / 256: the finest scale has NIQE's 96 pixels.  An
    untrained output may have no finite NIQE block (its rows are then NaN in both calls); the ground truth's rows are finite."""
    from test_hip_featdist import _Encoder
    from tgsr_amd import retrieval, train
    cfg_face.TREE.BASE_SIZE = 32
    NB, B, K, SEED = 2, 4, 3, 1
    kid = {"subsets": 4, "subset_size": 6}
    torch.manual_seed(3)
    enc = _Encoder().to(DEV).eval()
    for p in enc.parameters():
        p.requires_grad = False
    ids = [[B * k + i for i in range(B)] for k in range(NB)]

    def batches(with_ids=False):
        for k, b in enumerate(_val_batches(NB, B)):
            yield b + (ids[k],) if with_ids else b
    torch.manual_seed(7)
    tr = train.SRTrainer(41, device=DEV, image_encoder=enc)
    state = [p.detach().clone() for p in tr.params] + [b.detach().clone() for m in (tr.netGL, tr.netGH) for b in m.buffers()]
    every = tr.evaluate(batches(True), shave=2, r_precision=K, fid=True, kid=kid, niqe=True,
                        generator=torch.Generator().manual_seed(SEED))
    assert list(every) == ["fine", "fake", "r_precision", "fid", "kid", "niqe"] and enc.trunk_calls == 2 * NB
    after = [p.detach() for p in tr.params] + [b.detach() for m in (tr.netGL, tr.netGH) for b in m.buffers()]
    assert len(state) == len(after) and all(torch.equal(a, b) for a, b in zip(state, after))
    # `generator` is drawn from by r_precision's candidate table first, then by kid's subset tables: the call with kid alone gets
    # a generator of the same seed that has already given that candidate table, so its subset tables are the same ones
    past_candidates = torch.Generator().manual_seed(SEED)
    retrieval.sample_candidates(sum(ids, []), K, past_candidates)
    alone = {"plain": tr.evaluate(batches(), shave=2),
             "r_precision": tr.evaluate(batches(True), shave=2, r_precision=K, generator=torch.Generator().manual_seed(SEED)),
             "fid": tr.evaluate(batches(), shave=2, fid=True),
             "kid": tr.evaluate(batches(), shave=2, kid=kid, generator=past_candidates),
             "niqe": tr.evaluate(batches(), shave=2, niqe=True)}
    assert every["fine"][0]["n"] == NB * B and every["fid"]["n"] == NB * B and every["niqe"]["n"] == NB * B
    assert every["kid"]["per_subset"].shape == (4,) and np.isfinite(every["niqe"]["hr"]).all()
    for name, res in alone.items():
        assert list(res) == ["fine", "fake"] + ([] if name == "plain" else [name]), name
        for key in res:
            _same_entry(every[key], res[key], (name, key))
    after = [p.detach() for p in tr.params] + [b.detach() for m in (tr.netGL, tr.netGH) for b in m.buffers()]
    assert all(torch.equal(a, b) for a, b in zip(state, after))


def test_resume_in_place_then_replay_equals_eager(tmp_path, cfg_face):
    from tgsr_amd import train
    src = _trainer(False, False, seed=11)
    for step in range(2):
        torch.manual_seed(100 + step)
        src.step(*_train_batch(step))
    pl, ph = src.snapshot(str(tmp_path / "model"), 41, ema=True)
    want = [a.clone() for a in src.avg_param_G]
    twins = [_trainer(False, True), _trainer(False, False)]
    losses = [[], []]
    nwarm = train.GRAPH_G_WARMUP + 2
    for step in range(nwarm + 2):
        batch = _train_batch(step)
        for k, tr in enumerate(twins):
            if step == nwarm:
                ptrs = [p.data_ptr() for p in tr.params]
                v0 = tr.params[0]._version
                assert tr.resume(pl) == 42
                assert [p.data_ptr() for p in tr.params] == ptrs and tr.params[0]._version > v0
                for p, a, w in zip(tr.params, tr.avg_param_G, want):
                    assert torch.equal(p.detach(), w) and torch.equal(a, w)
            torch.manual_seed(100 + step)
            losses[k].append(float(tr.step(*batch)))
    torch.cuda.synchronize()
    caps = list(twins[0]._ggraphs.values())
    assert caps and all(isinstance(c, dict) for c in caps) and not twins[1]._ggraphs
    assert losses[0] == losses[1], losses
    _assert_twins(twins[0], twins[1])
    assert twins[0].resume("") == 0
