"""GPU: the image-quality kernels (tgsr_metrics.hip) through torch.ops.tgsr - Y byte for byte against the numpy model on every
RGB triple, the sums of squared differences exact, PSNR / RMSE bit-equal to the reference's recorded values, SSIM within 1e-9 of
the fp64 model (tests/metrics_model.py: a window statistic is a sum of 121 terms <= 65 025 in fp64, absolute error <~ 1e-9 against
denominators >= C2 = 58.5; both sides are fp64 and differ in summation order only)."""
import numpy as np
import pytest
import torch

from conftest import load_npz

import metrics_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
SSIM_TOL = 1e-9


def _ops():
    from tgsr_amd import custom_ops  # noqa: F401
    return torch.ops.tgsr


def test_rgb_to_y_on_every_rgb_triple():
    rgb = M.all_triples()
    want = M.rgb2y(rgb)
    golden = load_npz("sr_metrics.npz")
    assert M.sha256(want) == str(golden["triples_y_sha256"])
    got = _ops().rgb_to_y(torch.from_numpy(rgb)[None].to(DEV)).cpu().numpy()
    assert got.shape == (1, 4096, 4096) and got.dtype == np.uint8
    bad = np.flatnonzero(got[0].ravel() != want.ravel())
    assert bad.size == 0, "%d of 2^24 triples differ, first at index %d" % (bad.size, bad[0])
    assert M.sha256(got[0]) == str(golden["triples_y_sha256"])
    # batched: the plane arithmetic of B > 1
    small = torch.from_numpy(np.ascontiguousarray(rgb[:, :64, :96].reshape(3, 3, 32, 64).transpose(1, 0, 2, 3))).to(DEV)
    assert np.array_equal(_ops().rgb_to_y(small).cpu().numpy(), M.rgb2y(small.cpu().numpy()))


def test_fixture_pairs_sse_exact_psnr_bit_equal_ssim_close():
    from tgsr_amd import metrics
    golden, io = load_npz("sr_metrics.npz"), load_npz("io_pyramid.npz")
    for k in (1, 2, 3):
        a, b = io["ret%d_u8" % k][None], io["bic%d_u8" % k][None]
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        got = _ops().sr_metrics(ta, tb, 0).cpu().numpy()
        dev = M.check_rows(got, a, b, 0, SSIM_TOL)
        print("pair %d: rows %s, |ssim - model| = %.3g" % (k, got[0].tolist(), dev))
        sc = metrics.image_scores(ta, tb)
        for key, want in (("psnr", golden["pair%d_rgb" % k][0]), ("rmse", golden["pair%d_rgb" % k][1]),
                          ("psnr_y", golden["pair%d_y" % k][0]), ("rmse_y", golden["pair%d_y" % k][1])):
            assert sc[key].dtype == np.float64 and sc[key].shape == (1,)
            assert sc[key][0].tobytes() == want.tobytes(), (k, key, sc[key][0], want)
        # the same bytes as float images through the loader's normalisation
        fa, fb = torch.from_numpy(M.loader_normalise(a)).to(DEV), torch.from_numpy(M.loader_normalise(b)).to(DEV)
        assert np.array_equal(_ops().sr_metrics(fa, fb, 0).cpu().numpy(), got)


def _case(B, H, W, seed):
    """Float images with values outside [-1, 1] and inputs sitting exactly on rounding ties, and the bytes they quantise to."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((2, B, 3, H, W)) * 0.8).astype(np.float32)
    x[1] = x[0] + (rng.standard_normal((B, 3, H, W)) * 0.15).astype(np.float32)      # an "SR" near its ground truth
    k = np.arange(255, dtype=np.float32)
    ties = ((k + np.float32(0.5)) / np.float32(127.5) - np.float32(1)).astype(np.float32)
    exact = ties[(ties + np.float32(1)) * np.float32(127.5) == k + np.float32(0.5)]
    assert exact.size >= 8                                                           # inputs whose product is k + 0.5 exactly
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=max(16, flat.size // 7), replace=False)
    flat[idx] = rng.choice(exact, size=idx.size)
    flat[rng.choice(flat.size, size=max(4, flat.size // 50), replace=False)] = rng.choice(
        np.array([-3.0, 2.5, -1.0, 1.0, 1.0000001, -1.0000001, 100.0], dtype=np.float32), size=max(4, flat.size // 50))
    return x[1], x[0], M.quantise(x[1]), M.quantise(x[0])


SIZES = [(11, 11), (37, 53), (64, 64), (200, 240), (256, 256)]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("B", [1, 3, 16])
def test_sweep_against_the_model(B, H, W):
    from tgsr_amd._lib import TgsrError  # noqa: F401
    sr_f, hr_f, sr_u, hr_u = _case(B, H, W, seed=B * 1000 + H + W)
    t = {("f", 0): torch.from_numpy(sr_f).to(DEV), ("f", 1): torch.from_numpy(hr_f).to(DEV),
         ("u", 0): torch.from_numpy(sr_u).to(DEV), ("u", 1): torch.from_numpy(hr_u).to(DEV)}
    worst = 0.0
    for shave in (0, 4, 8):
        if H - 2 * shave < 11 or W - 2 * shave < 11:
            for da in "fu":
                for db in "fu":
                    with pytest.raises(ValueError):
                        _ops().sr_metrics(t[(da, 0)], t[(db, 1)], shave)
            continue
        first = None
        for da in "fu":
            for db in "fu":
                got = _ops().sr_metrics(t[(da, 0)], t[(db, 1)], shave).cpu().numpy()
                if first is None:
                    first = got
                    worst = max(worst, M.check_rows(got, sr_u, hr_u, shave, SSIM_TOL))
                else:                                   # the float inputs quantise to the uint8 inputs: the same bits whatever the dtypes
                    assert np.array_equal(got, first), (shave, da, db)
    print("B=%d %dx%d: worst |mean ssim - model| = %.3g" % (B, H, W, worst))


def test_identical_images_give_zero_inf_and_exactly_one():
    from tgsr_amd import metrics
    sr_f, _hr_f, sr_u, _hr_u = _case(3, 75, 131, seed=9)
    for a, b in ((sr_f, sr_f), (sr_u, sr_u), (sr_f, sr_u)):
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        for shave in (0, 4):
            rows = _ops().sr_metrics(ta, tb, shave).cpu().numpy()
            assert np.all(rows[:, :2] == 0)
            sc = metrics.image_scores(ta, tb, shave)
            assert np.all(sc["psnr"] == np.inf) and np.all(sc["psnr_y"] == np.inf)
            assert np.all(sc["rmse"] == 0) and np.all(sc["rmse_y"] == 0)
            assert np.all(sc["ssim_y"] == 1.0), sc["ssim_y"]


def test_runs_are_bit_equal_on_any_stream_and_in_a_captured_graph():
    sr_f, hr_f, _sr_u, hr_u = _case(16, 128, 128, seed=4)
    a, b, bu = torch.from_numpy(sr_f).to(DEV), torch.from_numpy(hr_f).to(DEV), torch.from_numpy(hr_u).to(DEV)
    T = _ops()
    first = T.sr_metrics(a, b, 4)
    y_first = T.rgb_to_y(bu)
    torch.cuda.synchronize()
    again = T.sr_metrics(a, b, 4)
    assert torch.equal(first, again)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = T.sr_metrics(a, b, 4)
        y_side = T.rgb_to_y(bu)
    side.synchronize()
    assert torch.equal(first, on_side) and torch.equal(y_first, y_side)
    # captured: static inputs, the workspace and the result from the graph's pool; replayed on new contents
    sa, sb = torch.zeros_like(a), torch.zeros_like(b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = T.sr_metrics(sa, sb, 4)
        yout = T.rgb_to_y(bu)
    sa.copy_(a)
    sb.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first) and torch.equal(yout, y_first)
    sa.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.all(out[:, :2] == 0)
    M.check_rows(first.cpu().numpy(), sr_f, hr_f, 4, SSIM_TOL)


def test_wrappers_validate_their_inputs():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    x = torch.zeros(2, 3, 32, 32, device=DEV)
    u = torch.zeros(2, 3, 32, 32, dtype=torch.uint8, device=DEV)
    T = _ops()
    for shave in (11, 12, 16, -1):
        with pytest.raises(ValueError):
            T.sr_metrics(x, x, shave)                                       # a crop under 11 x 11
    with pytest.raises(ValueError):
        T.sr_metrics(x[:, :, :10].contiguous(), x[:, :, :10].contiguous(), 0)
    assert T.sr_metrics(x, u, 10).shape == (2, 3)                           # 12 x 12 left: fine
    with pytest.raises(TgsrError):
        T.sr_metrics(x, x[:1], 0)                                           # unequal shapes
    with pytest.raises(TgsrError):
        T.sr_metrics(x, torch.zeros(2, 3, 32, 31, device=DEV), 0)
    c4 = torch.zeros(2, 4, 32, 32, device=DEV)
    with pytest.raises(TgsrError):
        T.sr_metrics(c4, c4, 0)                                             # C != 3
    with pytest.raises(TgsrError):
        T.rgb_to_y(c4.to(torch.uint8))
    with pytest.raises(TgsrError):
        T.sr_metrics(x.transpose(2, 3), x, 0)                               # not contiguous
    with pytest.raises(TgsrError):
        T.sr_metrics(x, torch.zeros(2, 3, 32, 64, device=DEV)[:, :, :, ::2], 0)
    with pytest.raises(TgsrError):
        T.rgb_to_y(u[:, :, :, ::2])
    with pytest.raises(TgsrError):
        T.sr_metrics(x.half(), x, 0)                                        # fp32 or uint8 only
    with pytest.raises(TgsrError):
        T.sr_metrics(x, x.double(), 0)
    with pytest.raises(TgsrError):
        T.rgb_to_y(x)
    with pytest.raises(TgsrError):
        ops.sr_metrics(x.cpu(), x, 0)


def test_opcheck_of_both_operators():
    T = _ops()
    basic = ("test_schema", "test_faketensor")
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 3, 24, 40, generator=g) * 2 - 1).to(DEV)
    u = torch.randint(0, 256, (2, 3, 24, 40), generator=g, dtype=torch.uint8).to(DEV)
    torch.library.opcheck(T.sr_metrics.default, (x, u, 2), test_utils=basic)
    torch.library.opcheck(T.sr_metrics.default, (u, x), test_utils=basic)
    torch.library.opcheck(T.rgb_to_y.default, (u,), test_utils=basic)
