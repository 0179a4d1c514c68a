"""GPU: NIQE on the device - tgsr_niqe_features through ctypes (every operand in a guarded arena) and through
torch.ops.tgsr.niqe_features, then niqe.NIQEModel, SRPipeline.niqe and SRTrainer.evaluate(niqe=) on top of it.

Every expected value comes from the numpy / scipy fp64 model of tests/niqe_model.py.  The inputs are a seeded smooth field plus +-6
grey levels of noise per pixel; on the model ALONE each case first asserts what makes a bitwise comparison of alpha meaningful: no
MSCN element with |m| < 1e-9 at either scale (a zero's sign is implementation-defined, and one flip moves a count by 1) and every
table search decided by more than 1e-9 relative.  Then
    alpha                          equal to the model's, bit for bit
    every other feature, sharpness within 1e-9 relative (the project's bound for its fp64 SSIM against its fp64 model)
    score on the same features     1e-9 relative against the model's eigh form and against np.linalg.pinv with the same cutoff
    score from the image           4 x the largest change of the model's score under +-1e-9 relative perturbations of the model's
                                   features (eight seeded draws) - measured on the model, never on the kernel
The constant-block cases hold the NaN positions to the model's; their zeros are exact on both sides (niqe_model.correlate_rows).
What the kernels promise beyond a bound is checked bit for bit: two runs, a replay from a captured graph, the operator against the
C entry."""
import ctypes

import numpy as np
import pytest
import torch

import niqe_model as M
import tgsr_amd.niqe  # noqa: F401   (registers torch.ops.tgsr.niqe_features)
from arena import Arena
from test_niqe_host import ALPHA, as_float, image, uneven

pytestmark = pytest.mark.gpu
DEV = "cuda"

# B, H, W, shave, float32 input: one block with every border replicated; the crop; the filter reads across a block edge while the
# roll wraps inside the block; shave, more than one block per side, both input types
CASES = [(2, 96, 96, 0, False), (1, 103, 191, 0, False), (1, 192, 96, 0, False), (1, 200, 300, 4, False), (1, 200, 300, 4, True)]
_CACHE = {}


def _lib():
    from tgsr_amd import _lib as L
    return L, L.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _case(B, H, W, shave, f32):
    """(images [B, 3, H, W] as numpy, the model's report per image), computed once."""
    key = (B, H, W, shave, f32)
    if key not in _CACHE:
        u8 = np.stack([image(100 * b + H + W, H, W) for b in range(B)])
        img = as_float(u8, 1) if f32 else u8
        _CACHE[key] = (img, [M.features(im, shave) for im in img])
    return _CACHE[key]


def _table():
    if "table" not in _CACHE:
        from tgsr_amd import ops
        _CACHE["table"] = tuple(torch.from_numpy(a) for a in ops.niqe_gamma_table())
    return _CACHE["table"]


def _features_abi(img, shave):
    """tgsr_niqe_features through ctypes: (feats [B, nblk, 36], sharp [B, nblk]) on the host, guards checked."""
    L_, L = _lib()
    B, _, H, W = img.shape
    nblk = ((H - 2 * shave) // 96) * ((W - 2 * shave) // 96)
    n_ws = L.tgsr_niqe_ws_elems(B, H, W, shave)
    assert n_ws == B * nblk * 64
    a = Arena(DEV)
    x = a.place_input(torch.from_numpy(img))
    gam, r_gam = (a.place_input(t) for t in _table())
    ws = a.place_ws(2 * n_ws)                                        # float words of a float64 workspace
    feats = a.place_output((B, nblk, 36), dtype=torch.float64)
    sharp = a.place_output((B, nblk), dtype=torch.float64)
    rc = L.tgsr_niqe_features(x.ptr, int(img.dtype == np.float32), B, H, W, shave, gam.ptr, r_gam.ptr, 9801, ws.ptr, feats.ptr,
                              sharp.ptr, _stream())
    assert rc == L_.OK, rc
    torch.cuda.synchronize()
    a.check()
    return feats.read().numpy(), sharp.read().numpy()


@pytest.mark.parametrize("B,H,W,shave,f32", CASES)
def test_features_against_the_model(B, H, W, shave, f32):
    img, refs = _case(B, H, W, shave, f32)
    for r in refs:                                                   # on the model alone, before any comparison
        assert r["near_zero"] == (0, 0), r["near_zero"]
        assert r["gaps"].min() > 1e-9, r["gaps"].min()
    feats, sharp = _features_abi(img, shave)
    for b, r in enumerate(refs):
        assert feats[b].shape == r["feats"].shape
        rel, rs = np.abs(feats[b] / r["feats"] - 1).max(), np.abs(sharp[b] / r["sharp"] - 1).max()
        print("%s image %d: features %.3g, sharpness %.3g relative; smallest gap %.3g" % ((B, H, W, shave, f32), b, rel, rs, r["gaps"].min()))
        assert np.array_equal(feats[b][:, ALPHA], r["feats"][:, ALPHA])
        assert rel <= 1e-9 and rs <= 1e-9


@pytest.mark.parametrize("c", [112, 96])
def test_a_constant_block_gives_nan_where_the_model_does(c):
    """192 x 192 with a black (Y = 16) top-left block - with its filter halo (c = 112: every MSCN element of the block is 0 at both
    scales) and alone (c = 96: the block's rim sees its neighbours).  NaN at exactly the model's positions, nothing else disturbed."""
    u8 = image(9, 192, 192)
    u8[:, :c, :c] = 0
    ref = M.features(u8)
    assert ref["near_zero"] == ref["exact_zero"] and ref["exact_zero"][0] >= 93 * 93     # the model's zeros are exact zeros
    assert np.isnan(ref["feats"][0]).any() and np.isfinite(ref["feats"][1:]).all()
    feats, sharp = (t.cpu().numpy()[0] for t in torch.ops.tgsr.niqe_features(torch.from_numpy(u8)[None].to(DEV), 0))
    assert np.array_equal(np.isnan(feats), np.isnan(ref["feats"]))
    ok = ~np.isnan(feats)
    assert np.array_equal(feats[:, ALPHA][ok[:, ALPHA]], ref["feats"][:, ALPHA][ok[:, ALPHA]])
    assert np.abs(feats[ok] / ref["feats"][ok] - 1).max() <= 1e-9
    assert np.abs(sharp[1:] / ref["sharp"][1:] - 1).max() <= 1e-9 and abs(sharp[0] - ref["sharp"][0]) <= 1e-9 * ref["sharp"][1:].max()


def test_two_runs_and_the_operator_give_the_same_bits():
    img, _refs = _case(1, 200, 300, 4, True)
    want = [torch.from_numpy(a) for a in _features_abi(img, 4)]
    x = torch.from_numpy(img).to(DEV)
    for _ in range(2):
        got = torch.ops.tgsr.niqe_features(x, 4)
        for a, b in zip(want, got):
            assert torch.equal(_bits(a), _bits(b.cpu()))
    two = torch.ops.tgsr.niqe_features(torch.cat([x, x.flip(0)]), 4)          # an image's rows do not depend on its neighbours
    assert torch.equal(_bits(two[0][1].cpu()), _bits(want[0][0]))


def test_the_launches_replay_from_a_captured_graph():
    img, _refs = _case(2, 96, 96, 0, False)
    x = torch.from_numpy(img).to(DEV)
    eager = [t.clone() for t in torch.ops.tgsr.niqe_features(x, 0)]   # the first call uploads the table: before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.tgsr.niqe_features(x, 0)
    for t in out:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def test_opcheck_of_the_operator():
    x = torch.from_numpy(_case(1, 103, 191, 0, False)[0]).to(DEV)
    torch.library.opcheck(torch.ops.tgsr.niqe_features.default, (x, 0), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.tgsr.niqe_features.default, (x, 3), test_utils=("test_schema", "test_faketensor"))


REFUSALS = [dict(H=95), dict(W=95), dict(H=103, shave=4), dict(shave=-1), dict(B=0), dict(B=65536), dict(n_gam=0), dict(img=False),
            dict(gam=False), dict(r_gam=False), dict(ws=False), dict(feats=False), dict(sharp=False)]


def test_bad_arguments_return_an_error_code_and_touch_nothing():
    L_, L = _lib()
    assert L.tgsr_niqe_ws_elems(1, 95, 96, 0) == 0 and L.tgsr_niqe_ws_elems(1, 103, 103, 4) == 0 and L.tgsr_niqe_ws_elems(0, 96, 96, 0) == 0
    for kw in REFUSALS:
        p = dict(B=1, H=96, W=96, shave=0, n_gam=9801, img=True, gam=True, r_gam=True, ws=True, feats=True, sharp=True)
        p.update(kw)
        a = Arena(DEV)
        x = a.place_input(torch.zeros(1, 3, 96, 96))
        gam, r_gam = (a.place_input(t) for t in _table())
        ws = a.place_output((128,), written=False)
        feats = a.place_output((1, 1, 36), written=False, dtype=torch.float64)
        sharp = a.place_output((1, 1), written=False, dtype=torch.float64)
        ptr = lambda r, name: r.ptr if p[name] else None
        rc = L.tgsr_niqe_features(ptr(x, "img"), 1, p["B"], p["H"], p["W"], p["shave"], ptr(gam, "gam"), ptr(r_gam, "r_gam"), p["n_gam"],
                                  ptr(ws, "ws"), ptr(feats, "feats"), ptr(sharp, "sharp"), _stream())
        assert rc == L_.EINVAL, kw
        torch.cuda.synchronize()
        a.check()
    from tgsr_amd import niqe
    with pytest.raises(ValueError):
        niqe.niqe_features(torch.zeros(1, 3, 95, 96, device=DEV))
    with pytest.raises(ValueError):
        torch.ops.tgsr.niqe_features(torch.zeros(1, 3, 103, 103, device=DEV), 4)


def _pristine():
    """(NIQEModel fitted on the device from 6 x 36 = 216 blocks with every block kept, the images): 216 > 36 rows, so the summed
    covariance of a score has full rank."""
    if "pristine" not in _CACHE:
        from tgsr_amd import niqe
        imgs = np.stack([image(40 + i, 576, 576, sigma=4.0 + 2 * i) for i in range(6)])
        model = niqe.NIQEModel.fit([torch.from_numpy(imgs[:3]).to(DEV), torch.from_numpy(imgs[3:]).to(DEV)], sharpness=0.0)
        _CACHE["pristine"] = (model, imgs)
    return _CACHE["pristine"]


def test_the_fit_on_the_device_against_the_model():
    from tgsr_amd import niqe
    model, imgs = _pristine()
    assert float(model.n) == 216.0
    rough = np.stack([uneven(90 + i, 480, 384) for i in range(3)])                    # 3 x 20 blocks of differing sharpness
    picky = niqe.NIQEModel.fit([torch.from_numpy(rough[:2]).to(DEV), torch.from_numpy(rough[2:]).to(DEV)])   # the default: 0.75
    mu, cov, n = M.fit(list(rough))
    assert 2 <= n < 60 and float(picky.n) == n                       # the threshold dropped blocks, the same ones
    assert np.allclose(picky.mu.cpu().numpy(), mu, rtol=1e-9, atol=0)
    assert np.allclose(picky.cov.cpu().numpy(), cov, rtol=0, atol=1e-9 * np.abs(cov).max())


def test_scores_against_the_model():
    model, _imgs = _pristine()
    mu_p, cov_p = model.mu.cpu().numpy(), model.cov.cpu().numpy()
    img, refs = _case(1, 200, 300, 4, False)
    u8 = np.stack([img[0], image(77, 200, 300, sigma=3.0), image(78, 200, 300, sigma=14.0, noise=9)])
    refs = [refs[0]] + [M.features(im, 4) for im in u8[1:]]
    x = torch.from_numpy(u8).to(DEV)
    feats = torch.ops.tgsr.niqe_features(x, 4)[0]
    got = model.score(x, 4)
    assert got.dtype == torch.float64 and got.device == x.device
    got = got.cpu().numpy()
    assert np.array_equal(got, model.score_features(feats).cpu().numpy())
    for k, r in enumerate(refs):
        f = feats[k].cpu().numpy()
        same = M.score(f, mu_p, cov_p)                                # the same features through the model's eigh form ...
        d, S = mu_p - f.mean(0), (cov_p + np.cov(f, rowvar=False)) / 2
        alt = float(np.sqrt(d @ np.linalg.pinv(S, rcond=36 * 2.0 ** -52, hermitian=True) @ d))     # ... and through numpy's pinv
        assert abs(got[k] - same) <= 1e-9 * same and abs(alt - same) <= 1e-9 * same
        want = M.score(r["feats"], mu_p, cov_p)                       # end to end: the model's own features
        rng = np.random.default_rng(500 + k)
        moved = max(abs(M.score(r["feats"] * (1 + 1e-9 * rng.choice([-1.0, 1.0], r["feats"].shape)), mu_p, cov_p) - want) for _ in range(8))
        print("image %d: score %.17g model %.17g, |difference| %.3g, allowed 4 x %.3g" % (k, got[k], want, abs(got[k] - want), moved))
        assert moved > 0 and abs(got[k] - want) <= 4 * moved
    one = feats[:1].clone()
    one[0, 1:] = float("nan")
    assert bool(torch.isnan(model.score_features(one)).all())


def test_sr_trainer_evaluate_niqe(tmp_path):
    from tgsr_amd import niqe
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.synthetic import synthetic_batch
    from tgsr_amd.train import SRTrainer
    from tgsr_amd.trainer import SRPipeline
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 256
    cfg.TREE.BRANCH_NUM = 4
    cfg.TREE.BASE_SIZE = 32
    NB, B = 3, 4
    try:
        def batches():
            for k in range(NB):
                cap, lens, LR, LRb = synthetic_batch(B, seed=70 + k)
                g = torch.Generator().manual_seed(80 + k)
                hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).to(DEV) for s in (64, 128, 256)]
                yield cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), hr
        torch.manual_seed(7)
        tr = SRTrainer(41, device=DEV)
        state = [p.detach().clone() for p in tr.params] + [b.detach().clone() for m in (tr.netGL, tr.netGH) for b in m.buffers()]
        plain = tr.evaluate(batches(), ema=False)
        assert sorted(plain) == ["fake", "fine"] and sorted(tr.evaluate(batches(), ema=False, niqe=None)) == ["fake", "fine"]
        fitted = tr.evaluate(batches(), ema=False, niqe=True, shave=2)
        assert sorted(fitted) == ["fake", "fine", "niqe"]
        same = tr.evaluate(batches(), ema=False, niqe=True)
        for name in ("fine", "fake"):                                # the PSNR / SSIM rows: bit for bit those of the plain call
            for a, b in zip(plain[name], same[name]):
                for key in a:
                    assert a[key] == b[key] if key in ("mean", "n") else np.array_equal(a[key], b[key]), (name, key)
        after = [p.detach() for p in tr.params] + [b.detach() for m in (tr.netGL, tr.netGH) for b in m.buffers()]
        assert len(state) == len(after) and all(torch.equal(a, b) for a, b in zip(state, after))

        # the same rows by hand: the ground truth's fit, then SRPipeline.niqe of the pipeline's outputs
        pipe = SRPipeline.from_modules(tr.text_encoder, tr.netGL, tr.netGH, device=DEV)
        hrs = [b[4][-1] for b in batches()]
        own = niqe.NIQEModel.fit(hrs, shave=2)
        given = niqe.NIQEModel.fit(hrs[:1])
        path = given.save(str(tmp_path / "pristine.npz"))
        for res, model, shave in ((fitted, own, 2), (tr.evaluate(batches(), ema=False, niqe=given), given, 0),
                                  (tr.evaluate(batches(), ema=False, niqe=path), given, 0)):
            rows = {"fine": [], "hr": []}
            with torch.no_grad(), tr._eval_weights(False):
                for cap, lens, LR, LRb, hr in batches():
                    rows["fine"].append(pipe.niqe(pipe(cap, lens, LR, LRb), model, shave))
                    rows["hr"].append(model.score(hr[-1], shave))
            assert res["niqe"]["n"] == NB * B and sorted(res["niqe"]) == ["fine", "hr", "mean", "n"]
            for key in rows:
                want = torch.cat(rows[key]).cpu().numpy()
                assert res["niqe"][key].dtype == np.float64 and np.array_equal(res["niqe"][key], want, equal_nan=True), key
                assert np.isfinite(want).all() or key == "fine"      # noise images have finite blocks; an untrained output may not
                m = res["niqe"]["mean"][key]
                assert m == float(np.mean(want)) or (np.isnan(m) and np.isnan(want).any())
        plus = tr.evaluate(batches(), ema=False, niqe=given, ensemble=8, max_batches=1)
        assert plus["niqe"]["n"] == B and plus["niqe"]["fine"].shape == (B,)
        cap, lens, LR, LRb, _hr = next(batches())
        up = pipe.upscale(LR[0], cap[0], lens[0], lr_blur=LRb[0])
        assert tuple(pipe.niqe(up, given).shape) == (1,)
        with pytest.raises(ValueError, match="niqe"):
            tr.evaluate(batches(), ema=False, niqe=3)
        with pytest.raises(ValueError, match="96"):
            tr.evaluate(batches(), ema=False, niqe=given, shave=81)
    finally:
        cfg_reset()
