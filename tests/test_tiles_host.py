"""CPU: the tile planner, the receptive-field count and - on the oracle - the claim `SRPipeline.upscale` rests on: with a halo of
`receptive_halo` LR pixels, cutting an image into windows, running the generators per window and stitching the owned rectangles
changes no value; one pixel less and the high-frequency network is wrong near the seams."""
import numpy as np
import pytest
import torch

import tiles_model as M
from conftest import FP32_TOL
from tgsr_amd import tiles as T

SWEEP = [(n, tile, halo)
         for tile, halo in ((64, 16), (64, 0), (128, 16), (33, 16), (8, 2), (5, 2), (3, 1), (1, 0), (96, 17))
         for n in sorted({tile, tile + 1, tile + halo, 2 * tile - halo, 2 * tile - halo + 1, 2 * tile, 3 * tile + 7, 1000, 4099})]


@pytest.mark.parametrize("n,tile,halo", SWEEP)
def test_plan_axis_properties(n, tile, halo):
    plan = T.plan_axis(n, tile, halo)
    c = 0
    for x0, own0, own1 in plan:
        assert 0 <= x0 and x0 + tile <= n                                  # the window lies inside the image
        assert own0 == c and own1 > own0                                   # the owned intervals partition [0, n) ...
        assert x0 <= own0 and own1 <= x0 + tile                            # ... and lie inside their window
        assert x0 == 0 or own0 - x0 >= halo                                # an edge is the image edge or >= halo away
        assert x0 + tile == n or x0 + tile - own1 >= halo
        c = own1
    assert c == n
    assert len(plan) <= -(-n // max(tile - 2 * halo, 1)) + 1               # no more windows than the stride needs


def test_plan_axis_refuses_what_it_cannot_plan():
    for args in ((63, 64, 16), (100, 32, 16), (100, 31, 16), (10, 4, -1)):
        with pytest.raises(ValueError, match="plan_axis"):
            T.plan_axis(*args)


def test_plan_tiles_is_the_product_of_the_axes():
    t = T.plan_tiles(64, 136, 64, 16)
    assert t.dtype == torch.int32 and t.tolist() == [[0, 0, 0, 64, 0, 48], [0, 32, 0, 64, 48, 80], [0, 64, 0, 64, 80, 112],
                                                     [0, 72, 0, 64, 112, 136]]
    t = T.plan_tiles(13, 21, 8, 2)
    ys, xs = T.plan_axis(13, 8, 2), T.plan_axis(21, 8, 2)
    assert t.tolist() == [[y[0], x[0], y[1], y[2], x[1], x[2]] for y in ys for x in xs]
    cover = np.zeros((13, 21), int)
    for y0, x0, oy0, oy1, ox0, ox1 in t.tolist():
        cover[oy0:oy1, ox0:ox1] += 1
    assert (cover == 1).all()
    # a side shorter than the tile: its window is the whole side, whatever the halo
    assert T.plan_tiles(20, 100, (20, 64), 16).tolist() == [[0, x[0], 0, 20, x[1], x[2]] for x in T.plan_axis(100, 64, 16)]


@pytest.fixture()
def cfg_face():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 256
    cfg.TREE.BRANCH_NUM = 4
    yield cfg
    cfg_reset()


def test_receptive_halo_is_counted_from_the_modules(cfg_face):
    from tgsr_amd.model import G_SR_NET_low, NetG_highweight
    from tgsr_amd.util import ResBlock
    gl, gh = G_SR_NET_low(), NetG_highweight()
    assert T.receptive_radius(gl, gh) == 15.625 and T.receptive_halo(gl, gh) == 16
    # a seventh ResBlock: two more 3x3 convolutions.  Behind the first up-block (64^2 for a 32^2 LR) each is half an LR pixel:
    # 15.625 + 1 = 16.625 -> 17 ...
    gh7 = NetG_highweight()
    gh7.residual24 = torch.nn.Sequential(gh7.residual24, ResBlock(channel_num=32))
    assert T.receptive_radius(gl, gh7) == 16.625 and T.receptive_halo(gl, gh7) == 17
    # ... and at LR resolution, in `residual` itself, a whole pixel each: 15.625 + 2 = 17.625 -> 18
    gh.residual = torch.nn.Sequential(*[ResBlock(channel_num=32) for _ in range(7)])
    assert T.receptive_radius(gl, gh) == 17.625 and T.receptive_halo(gl, gh) == 18
    gh.residual = torch.nn.Sequential(*[ResBlock(channel_num=32) for _ in range(1)])
    assert T.receptive_halo(gl, gh) == 9                                   # G_SR_NET_low's own radius takes over: 9.0
    with pytest.raises(ValueError, match="x8 generators"):
        T.receptive_halo(torch.nn.Identity(), gh)


def _worst(got, want):
    """max over values of |got - want| / (atol + rtol |want|) with atol = rtol = FP32_TOL: <= 1 is assert_allclose passing."""
    return float(np.max(np.abs(got - want) / (FP32_TOL + FP32_TOL * np.abs(want))))


def test_halo_16_is_exact_and_15_is_not():
    sds, cap, lens, LR, LRb, whole = M.face_case()
    used = {}
    for halo in (16, 15):
        table = T.plan_tiles(64, 136, 64, halo).numpy()
        tiled = M.oracle_tiled(sds, cap, lens, LR, LRb, table, 64, 64)
        for k in ("fine", "fake"):
            for i in range(3):
                assert not np.isnan(tiled[k][i]).any()
                used[halo, k, i] = _worst(tiled[k][i], whole[k][i])
    print("share of FP32_TOL used:", {k: round(v, 3) for k, v in used.items()})
    for k in ("fine", "fake"):
        for i in range(3):
            assert used[16, k, i] <= 1.0, "halo 16, %s[%d]: %.3g of the tolerance" % (k, i, used[16, k, i])
    assert max(used[15, "fine", i] for i in range(3)) > 1.0, "halo 15 is expected to break the high-frequency images"
