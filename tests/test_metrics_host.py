"""CPU: the image-quality metrics' host side - the numpy model of the definitions against the reference's recorded results
(tests/golden/sr_metrics.npz, written by tests/golden/make_metrics_golden.py from the reference's own rgb2y / psnr), the host
formulas of tgsr_amd.metrics, the score book, the operators' registration and the SR trainer's snapshot naming."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz

import metrics_model as M


@pytest.fixture(scope="module")
def golden():
    return load_npz("sr_metrics.npz")


@pytest.fixture(scope="module")
def pyramid():
    return load_npz("io_pyramid.npz")


def test_model_y_equals_the_reference_on_the_fixture_images(golden, pyramid):
    for k in (1, 2, 3):
        for name in ("ret", "bic"):
            y = M.rgb2y(pyramid["%s%d_u8" % (name, k)])
            assert y.dtype == np.uint8 and np.array_equal(y, golden["%s%d_y" % (name, k)]), (name, k)


def test_model_y_equals_the_reference_on_every_rgb_triple(golden):
    y = M.rgb2y(M.all_triples())
    assert y.shape == (4096, 4096)
    assert [int(y.min()), int(y.max())] == list(golden["triples_y_range"]) == [16, 235]
    assert M.sha256(y) == str(golden["triples_y_sha256"])


def test_psnr_from_sse_is_bit_equal_to_the_reference(golden, pyramid):
    from tgsr_amd.metrics import psnr_from_sse
    shown = {1: (27.7195, 29.9269), 2: (25.3672, 27.4544), 3: (23.5996, 25.5677)}
    for k in (1, 2, 3):
        a, b = pyramid["ret%d_u8" % k], pyramid["bic%d_u8" % k]
        got = psnr_from_sse(M.sse(a, b), a.size)
        got_y = psnr_from_sse(M.sse(M.rgb2y(a), M.rgb2y(b)), a.size // 3)
        for g, want in ((got, golden["pair%d_rgb" % k]), (got_y, golden["pair%d_y" % k])):
            assert np.float64(g[0]).tobytes() == want[0].tobytes() and np.float64(g[1]).tobytes() == want[1].tobytes(), (k, g, want)
        assert abs(got[0] - shown[k][0]) < 5e-5 and abs(got_y[0] - shown[k][1]) < 5e-5


def test_psnr_of_identical_images_is_inf_without_a_warning():
    import warnings
    from tgsr_amd.metrics import psnr_from_sse, scores_from_rows
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        p, r = psnr_from_sse(np.array([0.0, 3.0]), 3)
        sc = scores_from_rows(np.array([[0.0, 0.0, 36.0]]), 16, 16)
    assert p[0] == np.inf and r[0] == 0.0 and p.dtype == np.float64 and r[1] == 1.0
    assert sc["psnr"][0] == np.inf and sc["psnr_y"][0] == np.inf and sc["ssim_y"][0] == 1.0


def test_model_ssim_on_the_fixture_pairs(pyramid):
    """The build's own definition (the reference has none): the values DESIGN.md records for the three pairs."""
    shown = {1: 0.88595, 2: 0.77284, 3: 0.70437}
    for k in (1, 2, 3):
        _rgb, _y, ss, (_pixels, windows) = M.rows(pyramid["ret%d_u8" % k][None], pyramid["bic%d_u8" % k][None])
        assert windows == (pyramid["ret%d_u8" % k].shape[1] - 10) ** 2
        assert abs(ss[0] / windows - shown[k]) < 5e-6
    a = pyramid["ret1_u8"][None]
    assert M.rows(a, a)[2][0] / 54 ** 2 == 1.0


def test_uint8_round_trip_through_the_loader_normalisation_is_the_identity():
    u = np.arange(256, dtype=np.uint8)
    f = M.loader_normalise(u)
    assert f.dtype == np.float32 and f.min() == -1.0 and f.max() == 1.0
    assert np.array_equal(M.quantise(f), u)
    t = torch.from_numpy(u.copy())                                  # the same arithmetic in torch (what the loader's kernel restates)
    ft = (t.float() / 255 - 0.5) / 0.5
    assert np.array_equal(ft.numpy(), f)


def test_wrappers_and_operators_refuse_cpu_tensors():
    from tgsr_amd import custom_ops, ops  # noqa: F401
    from tgsr_amd._lib import TgsrError
    x = torch.zeros(1, 3, 16, 16)
    u = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(TgsrError):
        ops.sr_metrics(x, x)
    with pytest.raises(TgsrError):
        ops.rgb_to_y(u)
    with pytest.raises(TgsrError):
        torch.ops.tgsr.sr_metrics(x, u, 0)
    with pytest.raises(TgsrError):
        torch.ops.tgsr.rgb_to_y(u)


def test_pyramid_wrappers_check_their_arguments_and_refuse_cpu_tensors():
    """ops.resize_bilinear_u8 / gaussian_blur_u8 / u8_normalize: a tensor that is not uint8 (its bytes would be read as pixels), has
    too few dimensions or is empty, and a size or a pass count below 1, are named as such - with no device at all - and a good
    uint8 tensor on the CPU is refused for where it lives."""
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    u = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    blur = (1, 4473924, 1677722)
    for bad, what in ((u.float(), "uint8"), (u.to(torch.int8), "uint8"), (u[0, 0, 0], "dimension"), (u[:0], "empty"), (u, "HIP tensors")):
        with pytest.raises(TgsrError, match=what):
            ops.resize_bilinear_u8(bad, 4, 4, None, None)
        with pytest.raises(TgsrError, match=what):
            ops.gaussian_blur_u8(bad, *blur, 3)
    for bad, what in ((u.float(), "uint8"), (u.double(), "uint8"), (torch.tensor(3, dtype=torch.uint8), "dimension"), (u[:, :0], "empty"),
                      (u[0, 0, 0], "HIP tensors")):
        with pytest.raises(TgsrError, match=what):
            ops.u8_normalize(bad)
    for oh, ow in ((0, 4), (4, 0), (-2, 4)):
        with pytest.raises(TgsrError, match="at least 1 x 1"):
            ops.resize_bilinear_u8(u, oh, ow, None, None)
    for passes in (0, -1):
        with pytest.raises(TgsrError, match="passes"):
            ops.gaussian_blur_u8(u, *blur, passes)


def test_both_schemas_are_registered():
    from tgsr_amd import custom_ops  # noqa: F401
    have = {str(s) for s in torch._C._jit_get_all_schemas() if s.name.startswith("tgsr::")}
    assert "tgsr::sr_metrics(Tensor sr, Tensor hr, int shave=0) -> Tensor" in have
    assert "tgsr::rgb_to_y(Tensor rgb) -> Tensor" in have
    # the fake kernels: shapes and dtypes without a device
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a = torch.empty(5, 3, 40, 24)
        r = torch.ops.tgsr.sr_metrics(a, a.to(torch.uint8), 2)
        y = torch.ops.tgsr.rgb_to_y(a.to(torch.uint8))
    assert tuple(r.shape) == (5, 3) and r.dtype == torch.float64
    assert tuple(y.shape) == (5, 40, 24) and y.dtype == torch.uint8


def test_crop_rule():
    from tgsr_amd.metrics import crop_counts
    assert crop_counts(11, 11) == (121, 1)
    assert crop_counts(37, 53, 4) == (29 * 45, 19 * 35)
    for H, W, s in ((10, 64, 0), (64, 26, 8), (18, 18, 4), (64, 64, -1)):
        with pytest.raises(ValueError):
            crop_counts(H, W, s)


def test_score_book_merge_and_means():
    from tgsr_amd.metrics import KEYS, ScoreBook, scores_from_rows
    rng = np.random.default_rng(3)

    def rows(n):
        return np.stack([rng.integers(1, 10 ** 7, n), rng.integers(1, 10 ** 6, n), rng.uniform(100, 2000, n)], 1).astype(np.float64)
    sizes = {("fine", 0): (64, 64), ("fine", 1): (128, 96)}
    per_rank = [{s: rows(n) for s in sizes} for n in (3, 2, 4)]
    books = [ScoreBook.from_rows(r, sizes, shave=4) for r in per_rank]
    res = ScoreBook.merge(books).result()
    for s, (H, W) in sizes.items():
        allrows = np.concatenate([r[s] for r in per_rank], 0)                  # rank order
        want = scores_from_rows(allrows, H, W, 4)
        assert res[s]["n"] == 9
        for k in KEYS:
            assert np.array_equal(res[s][k], want[k]) and res[s][k].dtype == np.float64
            assert res[s]["mean"][k] == float(np.mean(want[k]))
        pixels = (H - 8) * (W - 8)
        assert np.array_equal(want["rmse"], np.sqrt(allrows[:, 0] / (3 * pixels)))
        assert np.array_equal(want["ssim_y"], allrows[:, 2] / ((H - 18) * (W - 18)))
    with pytest.raises(ValueError):
        ScoreBook.merge([books[0], ScoreBook.from_rows(per_rank[0], sizes, shave=0)])
    with pytest.raises(ValueError):
        ScoreBook.merge([])


def test_snapshot_names_resume_epoch_and_snapshot_due():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import SRTrainer
    pl, ph = SRTrainer.snapshot_paths("/some/netG_dir", 7)
    assert os.path.basename(pl) == "netG_epoch_7.pth" and os.path.basename(ph) == "netGH_epoch_7.pth"
    assert os.path.dirname(pl) == os.path.dirname(ph) == "/some/netG_dir"
    assert os.path.basename(ph) == os.path.basename(pl).replace("netG", "netGH")       # trainer_objective.py:91-93
    assert SRTrainer.resume_epoch("") == 0
    assert SRTrainer.resume_epoch(pl) == 8
    assert SRTrainer.resume_epoch("../models/netG_epoch_600.pth") == 601
    cfg_reset()
    try:
        cfg.TRAIN.SNAPSHOT_INTERVAL, cfg.TRAIN.MAX_EPOCH = 5, 12
        due = [e for e in range(1, 13) if SRTrainer.snapshot_due(None, e)]
        assert due == [5, 10, 12]
        assert [e for e in range(1, 9) if SRTrainer.snapshot_due(None, e, max_epoch=8)] == [5, 8]
    finally:
        cfg_reset()


def test_snapshot_files_hold_the_shipped_checkpoints_keys(tmp_path):
    """A trainer built on the host (no step is run there): snapshot() writes the two state_dicts under the reference's names with
    the keys and shapes of ckpt_manifest.json; ema=True stores the EMA parameters, ema=False the current ones; the generator
    classes load both strictly."""
    from tgsr_amd import model
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import SRTrainer
    man = json.load(open(os.path.join(GOLDEN, "ckpt_manifest.json")))
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    try:
        torch.manual_seed(2)
        tr = SRTrainer(41, device="cpu")
        with torch.no_grad():
            for a in tr.avg_param_G:
                a.add_(1.0)                                                     # EMA != current, recognisably
        for ema in (True, False):
            pl, ph = tr.snapshot(str(tmp_path / "m"), 3, ema=ema)
            assert (os.path.basename(pl), os.path.basename(ph)) == ("netG_epoch_3.pth", "netGH_epoch_3.pth")
            sd_l, sd_h = torch.load(pl), torch.load(ph)
            assert {k: list(v.shape) for k, v in sd_l.items()} == {k: v[0] for k, v in man["netG_epoch_7"].items()}
            assert {k: list(v.shape) for k, v in sd_h.items()} == {k: v[0] for k, v in man["netGH_epoch_7"].items()}
            model.G_SR_NET_low().load_state_dict(sd_l, strict=True)
            model.NetG_highweight(weightmap=False, low="lr").load_state_dict(sd_h, strict=True)
            k = 0
            for net, sd in ((tr.netGL, sd_l), (tr.netGH, sd_h)):
                for name, p in net.named_parameters():
                    want = tr.avg_param_G[k] if ema else p.detach()
                    assert torch.equal(sd[name], want), (ema, name)
                    k += 1
                for name, b in net.named_buffers():
                    if name in sd:
                        assert torch.equal(sd[name], b), name
            assert k == len(tr.avg_param_G)
    finally:
        cfg_reset()
