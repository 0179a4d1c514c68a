"""CPU: NIQE on the host - the constants of the definition, the torch fp64 path of tgsr_amd/niqe.py against the numpy / scipy model of
tests/niqe_model.py, the streaming fit, the parameter files and the refusals (no kernel runs)."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch
from scipy import ndimage

import niqe_model as M

ALPHA = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]          # the columns of the 36 that hold a table entry


def image(seed, H, W, sigma=8.0, noise=6):
    """uint8 [3, H, W]: a seeded smooth field plus +-`noise` grey levels per pixel (no MSCN element is then near zero)."""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((3, H, W)), (0, sigma, sigma))
    f = f / np.abs(f).max()
    return np.clip(128 + 100 * f + rng.integers(-noise, noise + 1, (3, H, W)), 0, 255).astype(np.uint8)


def uneven(seed, H, W):
    """The same with +-2 grey levels of noise in the upper half and +-8 in the lower: the sharpness of the blocks differs, a fit
    with the default threshold keeps only some of them."""
    rng = np.random.default_rng(seed + 1000)
    u8 = image(seed, H, W, noise=2).astype(np.int64)
    u8[:, H // 2:] += rng.integers(-6, 7, (3, H - H // 2, W))
    return np.clip(u8, 0, 255).astype(np.uint8)


def as_float(u8, seed):
    """float32 in [-1, 1] that quantises back to `u8`, off the grid of byte values by up to 0.4 of a level."""
    rng = np.random.default_rng(seed)
    return ((u8.astype(np.float64) + rng.uniform(-0.4, 0.4, u8.shape)) / 127.5 - 1.0).astype(np.float32)


def test_the_down_sampling_taps_are_the_cubic_kernel_at_half_rate():
    x = (np.arange(8) - 3.5) * 0.5                                  # +-0.25 ... +-1.75
    assert np.array_equal(M.cubic(x) * 0.5, M.TAPS)
    assert M.TAPS.sum() == 1.0
    from tgsr_amd import niqe
    assert np.array_equal(np.array(niqe.TAPS) / 256.0, M.TAPS)


def test_the_window_adds_up_to_one_exactly_and_the_table_increases():
    from tgsr_amd import niqe, ops
    w = M.window()
    s = 0.0
    for v in w:
        s += v
    assert s == 1.0                                                 # a constant power-of-two plane passes the filter unchanged
    assert np.array_equal(niqe.gaussian_window().numpy(), w)
    gam, r_gam = ops.niqe_gamma_table()
    assert gam.shape == (9801,) and np.array_equal(gam, M.GAM)
    assert (np.diff(r_gam) > 1e-6).all() and (np.diff(M.R_GAM) > 1e-6).all()
    assert np.abs(r_gam / M.R_GAM - 1).max() < 1e-13


def test_the_models_filter_is_ndimages_to_rounding():
    y = np.random.default_rng(0).uniform(0, 255, (40, 50))
    w = M.window()
    want = ndimage.correlate1d(ndimage.correlate1d(y, w, axis=1, mode="nearest"), w, axis=0, mode="nearest")
    got = M.correlate_rows(M.correlate_rows(y, w).T, w).T
    assert np.abs(got - want).max() <= 1e-13 * 255
    c = np.full((12, 12), 16.0)
    assert np.array_equal(M.correlate_rows(c, w), c)


CASES = [(96, 96, 0, False), (103, 191, 0, False), (192, 96, 0, False), (200, 300, 4, False), (200, 300, 4, True)]


@pytest.mark.parametrize("H,W,shave,f32", CASES)
def test_the_host_path_against_the_model(H, W, shave, f32):
    from tgsr_amd import niqe
    u8 = image(H + W, H, W)
    img = as_float(u8, 1) if f32 else u8
    ref = M.features(img, shave)
    assert ref["near_zero"] == (0, 0) and ref["gaps"].min() > 1e-9
    feats, sharp = niqe.niqe_features(torch.from_numpy(img)[None], shave)
    feats, sharp = feats[0].numpy(), sharp[0].numpy()
    assert feats.shape == ref["feats"].shape and np.isfinite(feats).all()
    assert np.array_equal(feats[:, ALPHA], ref["feats"][:, ALPHA])
    assert np.abs(feats / ref["feats"] - 1).max() <= 1e-9 and np.abs(sharp / ref["sharp"] - 1).max() <= 1e-9
    if f32:
        assert np.array_equal(M.to_uint8(img), u8)


def test_a_constant_block_gives_nan_where_the_model_does():
    from tgsr_amd import niqe
    for c in (112, 96):                                             # the block with its filter halo, the block alone
        u8 = image(9, 192, 192)
        u8[:, :c, :c] = 0                                           # black: Y = 16
        ref = M.features(u8)
        assert ref["near_zero"] == ref["exact_zero"] and ref["exact_zero"][0] >= 93 * 93
        feats = niqe.niqe_features(torch.from_numpy(u8)[None])[0][0].numpy()
        assert np.isnan(ref["feats"][0]).any() and np.isfinite(ref["feats"][1:]).all()
        assert np.array_equal(np.isnan(feats), np.isnan(ref["feats"]))
        ok = ~np.isnan(feats)
        assert np.abs(feats[ok] / ref["feats"][ok] - 1).max() <= 1e-9


def _batches():
    return [torch.from_numpy(np.stack([uneven(10 * k + i, 384, 288) for i in range(2)])) for k in range(3)]


def test_fit_on_a_stream_is_fit_on_the_concatenation_and_the_models():
    from tgsr_amd import niqe
    bs = _batches()
    a = niqe.NIQEModel.fit(bs, device="cpu")
    b = niqe.NIQEModel.fit([torch.cat(bs)], device="cpu")
    assert 2 <= float(a.n) == float(b.n) < 72                       # 6 images of 12 blocks, the threshold drops some
    assert np.allclose(a.mu.numpy(), b.mu.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(a.cov.numpy(), b.cov.numpy(), rtol=0, atol=1e-12 * float(a.cov.abs().max()))
    halves = [niqe.NIQEModel.fit(bs[:1], device="cpu"), niqe.NIQEModel.fit(bs[1:], device="cpu")]
    m = niqe.NIQEModel(device="cpu").merge(halves)
    assert float(m.n) == float(a.n) and np.allclose(m.mu.numpy(), a.mu.numpy(), rtol=1e-12, atol=0)
    mu, cov, n = M.fit([im.numpy() for bt in bs for im in bt])
    assert n == float(a.n)
    assert np.allclose(a.mu.numpy(), mu, rtol=1e-9, atol=0)
    assert np.allclose(a.cov.numpy(), cov, rtol=0, atol=1e-9 * np.abs(cov).max())


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from tgsr_amd import niqe, parallel
    parallel.init_distributed("gloo")
    model = niqe.NIQEModel.fit(_batches()[:1] if rank == 0 else _batches()[1:], device="cpu")      # uneven shards
    model.all_reduce()
    q.put((rank, float(model.n), model.mu.numpy(), model.cov.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_leaves_the_fit_of_the_union_on_both_ranks():
    from tgsr_amd import niqe
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=120) for _ in ps), key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    whole = niqe.NIQEModel.fit(_batches(), device="cpu")
    for _rank, n, mu, cov in res:
        assert n == float(whole.n)
        assert np.allclose(mu, whole.mu.numpy(), rtol=1e-12, atol=0)
        assert np.allclose(cov, whole.cov.numpy(), rtol=0, atol=1e-12 * float(whole.cov.abs().max()))
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


def test_scores_against_the_model_and_numpys_pinv():
    from tgsr_amd import niqe
    pristine = niqe.NIQEModel.fit([torch.from_numpy(np.stack([image(40 + i, 576, 576) for i in range(3)]))], sharpness=0.0, device="cpu")
    assert float(pristine.n) == 108                                 # > 36: the summed covariance has full rank
    imgs = torch.from_numpy(np.stack([image(60 + i, 200, 300, sigma=3.0 + 4 * i) for i in range(3)]))
    feats, _ = niqe.niqe_features(imgs, 4)
    got = pristine.score_features(feats).numpy()
    assert np.array_equal(got, pristine.score(imgs, 4).numpy())
    mu_p, cov_p = pristine.mu.numpy(), pristine.cov.numpy()
    for k in range(3):
        f = feats[k].numpy()
        want = M.score(f, mu_p, cov_p)
        d = mu_p - f.mean(0)
        S = (cov_p + np.cov(f, rowvar=False)) / 2
        alt = np.sqrt(d @ np.linalg.pinv(S, rcond=36 * 2.0 ** -52, hermitian=True) @ d)
        assert abs(got[k] - want) <= 1e-9 * want and abs(alt - want) <= 1e-9 * want
    one = feats[:1].clone()
    one[0, 1:] = float("nan")                                       # a single finite row: no covariance
    assert np.isnan(pristine.score_features(one).numpy()).all() and np.isnan(M.score(one[0].numpy(), mu_p, cov_p))


def test_save_load_and_the_foreign_parameter_files(tmp_path):
    from scipy import io as sio
    from tgsr_amd import niqe
    fitted = niqe.NIQEModel.fit(_batches()[:1], device="cpu")
    again = niqe.NIQEModel.load(fitted.save(str(tmp_path / "fit.npz")), "cpu")
    assert torch.equal(again.mu, fitted.mu) and torch.equal(again.cov, fitted.cov) and float(again.n) == float(fitted.n)
    again.add(*niqe.niqe_features(_batches()[1]))                   # a loaded fit goes on streaming
    given = niqe.NIQEModel(fitted.mu, fitted.cov, "cpu")
    back = niqe.NIQEModel.load(given.save(str(tmp_path / "given.npz")), "cpu")
    assert torch.equal(back.mu, fitted.mu) and torch.equal(back.cov, fitted.cov)
    with pytest.raises(ValueError):
        back.add(*niqe.niqe_features(_batches()[1]))
    mu, cov = fitted.mu.numpy(), fitted.cov.numpy()
    np.savez(str(tmp_path / "basicsr.npz"), mu_pris_param=mu[None], cov_pris_param=cov, gaussian_window=np.zeros((7, 7)))
    sio.savemat(str(tmp_path / "matlab.mat"), {"mu_prisparam": mu[None], "cov_prisparam": cov, "blocksizerow": 96})
    for name in ("basicsr.npz", "matlab.mat"):
        m = niqe.NIQEModel.load(tmp_path / name, "cpu")
        assert np.array_equal(m.mu.numpy(), mu) and np.array_equal(m.cov.numpy(), cov)
    np.savez(str(tmp_path / "other.npz"), mean=mu, cov=cov)
    with pytest.raises(ValueError, match="mu_pris_param"):
        niqe.NIQEModel.load(str(tmp_path / "other.npz"), "cpu")
    with pytest.raises(ValueError):
        niqe.NIQEModel(mu[:35], cov, "cpu")


def test_small_images_and_cpu_operands_are_refused():
    from tgsr_amd import niqe, ops
    from tgsr_amd._lib import TgsrError
    for shape, shave in (((1, 3, 95, 200), 0), ((1, 3, 200, 95), 0), ((1, 3, 103, 103), 4)):
        with pytest.raises(ValueError, match="96"):
            niqe.niqe_features(torch.zeros(shape, dtype=torch.uint8), shave)
    with pytest.raises(ValueError):
        niqe.niqe_features(torch.zeros(1, 3, 96, 96, dtype=torch.float64))
    with pytest.raises(ValueError):
        niqe.niqe_features(torch.zeros(1, 1, 96, 96))
    with pytest.raises(TgsrError):
        ops.niqe_features(torch.zeros(1, 3, 96, 96))
    with pytest.raises(TgsrError):
        torch.ops.tgsr.niqe_features(torch.zeros(1, 3, 96, 96), 0)


def test_evaluate_refuses_a_bad_niqe_argument(tmp_path):
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import SRTrainer
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    try:
        torch.manual_seed(2)
        tr = SRTrainer(41, device="cpu")
        for bad in (3, 0.5, {"mu": 1}, [True]):
            with pytest.raises(ValueError, match="niqe"):
                tr.evaluate(iter(()), niqe=bad)
        with pytest.raises(FileNotFoundError):
            tr.evaluate(iter(()), niqe=str(tmp_path / "absent.npz"))
    finally:
        cfg_reset()
