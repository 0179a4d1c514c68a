"""GPU: whole-image inference by tiles - the gather / stitch kernels (tgsr_tiles.hip) against their numpy model bit for bit, their
custom operators, `SRPipeline.upscale` against the CPU oracle's WHOLE-image result and against a numpy stitch of the pipeline's own
per-tile outputs, its output modes and refusals, and `datasets.example_pyramid` against the reference's own function."""
import numpy as np
import pytest
import torch

import tiles_model as M
from conftest import FP32_TOL, load_npz
from tgsr_amd import tiles as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tgsr_amd import _lib
    _lib.lib()          # raises if the HIP library is missing: no silent fallback
    assert torch.cuda.is_available()


@pytest.fixture()
def cfg_face():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 256
    cfg.TREE.BRANCH_NUM = 4
    yield cfg
    cfg_reset()


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _image(g, H, W, u8):
    return g.integers(0, 256, (3, H, W), dtype=np.uint8) if u8 else g.standard_normal((3, H, W)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ gather
# 64 x 64: one window; 64 x 136: four, the last clamped back (x0 = 72); 75 x 70: odd width and window origins 11 / 6 - the element-
# wise path; 13 x 21 at tile 8, halo 2: the generic case; 24 x 40 at tile (6, 20): a window width that is a multiple of 4 over
# origins that are not, 9 x 14 at tile (5, 7): a window width that is not
GATHER = [(64, 64, 64, 64, 16), (64, 136, 64, 64, 16), (75, 70, 64, 64, 16), (13, 21, 8, 8, 2), (24, 40, 6, 20, 2), (9, 14, 5, 7, 1)]


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("H,W,th,tw,halo", GATHER)
def test_gather_equals_the_numpy_model_bit_for_bit(H, W, th, tw, halo, u8):
    from tgsr_amd import ops
    g = np.random.default_rng(H * 1000 + W)
    a, b = _image(g, H, W, u8), _image(g, H, W, u8)
    table = T.plan_tiles(H, W, (th, tw), halo)
    want_a, want_b = M.gather(a, table.numpy(), th, tw), M.gather(b, table.numpy(), th, tw)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    lr, lrb = ops.tile_gather(ta, table, th, tw, img2=tb)
    assert lr.dtype == torch.float32 and tuple(lr.shape) == (len(table), 3, th, tw) == tuple(lrb.shape)
    assert np.array_equal(bits(lr), bits(want_a)) and np.array_equal(bits(lrb), bits(want_b))
    one, none = ops.tile_gather(tb, table, th, tw)                          # without the second image
    assert none is None and np.array_equal(bits(one), bits(want_b))
    if u8:                                                                  # the same floats u8_normalize gives
        assert torch.equal(lr, torch.stack([ops.u8_normalize(ta[:, y:y + th, x:x + tw]) for y, x in table[:, :2].tolist()]))
    # a view that starts 4 bytes (f32) / 1 byte (u8) into its storage: the aligned forms do not apply, the values do
    flat = torch.empty(a.size + 8, dtype=ta.dtype, device=DEV)
    off = flat[1:1 + a.size].view(3, H, W)
    off.copy_(ta)
    assert np.array_equal(bits(ops.tile_gather(off, table, th, tw)[0]), bits(want_a))


# ------------------------------------------------------------------------------------------------ stitch
def _stitch_case(pad=0):
    """Tile outputs at tile 8, halo 2 for a 13 x 21 image: scales 1, 2, 8 x channels 3 and 18, normal values wide enough to clip,
    with exact rounding ties ((x + 1) * 127.5 = k + 0.5) sprinkled in.  pad: the last window (and its tile) that many times more."""
    H, W, th = 13, 21, 8
    table = T.plan_tiles(H, W, th, 2)
    g = np.random.default_rng(3)
    tiles = []
    for C in (3, 18):
        for s in (1, 2, 8):
            x = (g.standard_normal((len(table), C, s * th, s * th)) * 0.9).astype(np.float32)
            ties = ((g.integers(0, 255, x.shape) + 0.5) / 127.5 - 1.0).astype(np.float32)
            x = np.where(g.random(x.shape) < 0.05, ties, x)
            tiles.append(np.concatenate([x] + [x[-1:]] * pad))
    return H, W, th, torch.cat([table] + [table[-1:]] * pad).contiguous(), tiles


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_stitch_equals_the_numpy_model(u8):
    from tgsr_amd import ops
    H, W, th, table, tiles = _stitch_case()
    dt, ndt = (torch.uint8, np.uint8) if u8 else (torch.float32, np.float32)
    pad = 64
    want, bufs, outs = [], [], []
    for x in tiles:
        C, s = x.shape[1], x.shape[2] // th
        want.append(M.stitch(x, table.numpy(), th, np.zeros((C, s * H, s * W), ndt)))
        buf = torch.full((pad + want[-1].size + pad,), 0xA5 if u8 else float("nan"), dtype=dt, device=DEV)
        bufs.append(buf)
        outs.append(buf[pad:pad + want[-1].size].view(C, s * H, s * W))     # NaN / sentinel everywhere, guards on both sides
    dev = [torch.from_numpy(x).to(DEV) for x in tiles]
    ops.tile_stitch(dev, outs, table, H, W, th, th)                         # six outputs, one launch
    for e, (o, w, buf) in enumerate(zip(outs, want, bufs)):
        got = o.cpu().numpy()
        assert not (np.isnan(got).any() if not u8 else False), "output %d keeps a NaN: a pixel without a source" % e
        assert np.array_equal(bits(got), bits(w)), "output %d" % e
        guard = buf.cpu().numpy()
        for part in (guard[:pad], guard[pad + w.size:]):
            assert np.all(part == 0xA5) if u8 else np.isnan(part).all(), "output %d: a write outside the image" % e
    if u8:                                                                   # ... and the bytes are to_uint8's
        for o, x in zip(outs, dev):
            whole = torch.full(tuple(o.shape), float("nan"), device=DEV)
            ops.tile_stitch([x], [whole], table, H, W, th, th)
            assert torch.equal(o, ops.to_uint8(whole))
    # a padded final batch (the last window twice more): the same bytes
    H, W, th, ptable, ptiles = _stitch_case(pad=2)
    pouts = [torch.full_like(o, 0x5A if u8 else float("nan")) for o in outs]
    ops.tile_stitch([torch.from_numpy(x).to(DEV) for x in ptiles], pouts, ptable, H, W, th, th)
    for o, p in zip(outs, pouts):
        assert np.array_equal(bits(o), bits(p))
    # a channel crop of a wider buffer is stitched in place (what a captured step's attention maps are)
    wide = torch.randn(len(table), 18, 2 * th, 2 * th, device=DEV)
    a, b = torch.empty(9, 2 * H, 2 * W, device=DEV), torch.empty(9, 2 * H, 2 * W, device=DEV)
    ops.tile_stitch([wide[:, :9]], [a], table, H, W, th, th)
    ops.tile_stitch([wide[:, :9].contiguous()], [b], table, H, W, th, th)
    assert torch.equal(a, b)


def test_stitch_of_an_image_with_odd_owned_columns_and_rectangular_windows():
    """75 x 70 at tile 64, halo 16 (an odd image width at s = 1 and 3, a second window that starts at column 6: element-wise; s = 2
    gives rows of 140 floats - the aligned quads of the destination against a source that is not), a 9 x 14 image at windows of
    5 x 7 and a 10 x 23 one at 10 x 9: owned columns that start and end on odd offsets, partial first and last groups of every row."""
    from tgsr_amd import ops
    g = np.random.default_rng(9)
    for H, W, th, tw, halo in ((75, 70, 64, 64, 16), (9, 14, 5, 7, 1), (10, 23, 10, 9, 3)):
        table = T.plan_tiles(H, W, (th, tw), halo)
        for s in (1, 2, 3):
            x = g.standard_normal((len(table), 3, s * th, s * tw)).astype(np.float32)
            want = M.stitch(x, table.numpy(), th, np.full((3, s * H, s * W), np.nan, np.float32))
            out = torch.full((3, s * H, s * W), float("nan"), device=DEV)
            ops.tile_stitch([torch.from_numpy(x).to(DEV)], [out], table, H, W, th, tw)
            assert np.array_equal(bits(out), bits(want)), (H, W, th, tw, s)


# ------------------------------------------------------------------------------------------------ operators
def test_opcheck_and_refusals_of_both_operators():
    import tgsr_amd.custom_ops  # noqa: F401   (registers torch.ops.tgsr.*)
    from tgsr_amd import _lib, ops
    from tgsr_amd._lib import TgsrError
    ops_ = torch.ops.tgsr
    basic = ("test_schema", "test_faketensor")
    H, W, th = 13, 21, 8
    table = T.plan_tiles(H, W, th, 2)
    tdev = table.to(DEV)
    img = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device=DEV)
    fimg = torch.randn(3, H, W, device=DEV)
    chk = torch.library.opcheck
    chk(ops_.tile_gather.default, (img, img.flip(2).contiguous(), table, tdev, th, th), test_utils=basic)
    chk(ops_.tile_gather.default, (fimg, None, table, tdev, th, th), test_utils=basic)
    lr, none = ops_.tile_gather(fimg, None, table, tdev, th, th)
    assert none.numel() == 0 and torch.equal(lr, ops.tile_gather(fimg, table, th, th)[0])
    tiles = [torch.randn(len(table), 3, 2 * th, 2 * th, device=DEV), torch.randn(len(table), 5, th, th, device=DEV)]
    outs = [torch.zeros(3, 2 * H, 2 * W, device=DEV), torch.zeros(5, H, W, dtype=torch.uint8, device=DEV)]
    chk(ops_.tile_stitch.default, (tiles, outs, table, tdev, H, W, th, th), test_utils=basic)
    # refusals, each before anything is launched
    with pytest.raises(TgsrError, match="HIP tensors"):
        ops.tile_gather(fimg.cpu(), table, th, th)
    with pytest.raises(TgsrError, match="CPU tensors"):
        ops_.tile_gather(fimg.cpu(), None, table, table, th, th)
    with pytest.raises(TgsrError, match="uint8 or float32"):
        ops.tile_gather(fimg.double(), table, th, th)
    with pytest.raises(TgsrError, match=r"\[3, H, W\]"):
        ops.tile_gather(fimg[None], table, th, th)
    with pytest.raises(TgsrError, match="img2 is"):
        ops.tile_gather(fimg, table, th, th, img2=img)
    with pytest.raises(TgsrError, match=r"int32 \[Tb, 6\]"):
        ops.tile_gather(fimg, table[:, :5].contiguous(), th, th)
    with pytest.raises(TgsrError, match=r"int32 \[Tb, 6\]"):
        ops.tile_gather(fimg, table.long(), th, th)
    with pytest.raises(TgsrError, match="device copy"):
        ops.tile_gather(fimg, table, th, th, table_dev=tdev[:2])
    bad = table.clone()
    bad[1, 1] = W - th + 1                                                  # a window that leaves the image
    with pytest.raises(TgsrError, match="outside the image"):
        ops.tile_gather(fimg, bad, th, th)
    bad = table.clone()
    bad[0, 5] = bad[0, 1] + th + 1                                          # owned columns beyond the window
    with pytest.raises(TgsrError, match="owned columns"):
        ops.tile_stitch(tiles, outs, bad, H, W, th, th)
    with pytest.raises(TgsrError, match="integer scale"):
        ops.tile_stitch([tiles[0][:, :, :-1]], [outs[0]], table, H, W, th, th)
    with pytest.raises(TgsrError, match="float32 or uint8"):
        ops.tile_stitch([tiles[0]], [outs[0].double()], table, H, W, th, th)
    with pytest.raises(TgsrError, match="float32 or uint8"):
        ops.tile_stitch([tiles[0]], [outs[0][:, :-1]], table, H, W, th, th)
    with pytest.raises(TgsrError, match="HIP tensors"):
        ops.tile_stitch([tiles[0]], [outs[0].cpu()], table, H, W, th, th)
    with pytest.raises(TgsrError, match="per launch"):
        ops.tile_stitch([tiles[0]] * 13, [outs[0]] * 13, table, H, W, th, th)
    # the C entry repeats the table checks on its host copy
    L = _lib.lib()
    bad = table.clone()
    bad[2, 0] = -1
    out = torch.empty(len(table), 3, th, th, device=DEV)
    rc = L.tgsr_tile_gather(ops._p(fimg), None, 0, H, W, ops._p(bad), ops._p(tdev), len(table), th, th, ops._p(out), None, ops._stream())
    assert rc == _lib.EINVAL
    rc = L.tgsr_tile_gather(ops._p(fimg), None, 0, H, W, ops._p(table), ops._p(tdev), len(table), H + 1, th, ops._p(out), None,
                            ops._stream())
    assert rc == _lib.EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ SRPipeline.upscale
def _pipe(weights, dtype="fp32", **kw):
    from conftest import split_sd
    from tgsr_amd.trainer import SRPipeline
    p = SRPipeline(41, device=DEV, low=kw.pop("low", "lr"), dtype=dtype, **kw)
    return p.load_state_dicts(split_sd(weights, "E."), split_sd(weights, "GL."), split_sd(weights, "GH."))


def _close(got, want, tol, what):
    got = got.detach().cpu().numpy()
    err = float(np.max(np.abs(got - want) / (tol + tol * np.abs(want))))
    print("%s: %.3f of the tolerance %g" % (what, err, tol))
    np.testing.assert_allclose(got, want, atol=tol, rtol=tol, err_msg=what)


@pytest.mark.parametrize("tile_batch", [2, 3])
def test_upscale_equals_the_oracle_on_the_whole_image(tile_batch, face_weights, cfg_face):
    """LR 64 x 136 -> four 64 x 64 windows in batches of 2, and of 3 (which pads with two repeats of the last window), against ONE
    run of the CPU oracle over the whole 64 x 136 image."""
    _sds, cap, lens, LR, LRb, whole = M.face_case()
    p = _pipe(face_weights)
    r = p.upscale(LR[0].to(DEV), cap[0].to(DEV), int(lens[0]), lr_blur=LRb[0].to(DEV), tile=64, halo=16, tile_batch=tile_batch,
                  with_att=True)
    torch.cuda.synchronize()
    for i, s in enumerate((2, 4, 8)):
        assert tuple(r["fine"][i].shape) == (3, s * 64, s * 136) == tuple(r["fake"][i].shape)
        _close(r["fake"][i], whole["fake"][i], FP32_TOL, "fake[%d]" % i)
        _close(r["fine"][i], whole["fine"][i], FP32_TOL, "fine[%d]" % i)
    for i, s in enumerate((1, 2, 4)):
        assert tuple(r["att"][i].shape) == (9, s * 64, s * 136)
        _close(r["att"][i], whole["att"][i], 2e-5, "att[%d]" % i)


def test_upscale_of_an_image_with_a_side_shorter_than_the_tile(face_weights, cfg_face):
    """40 x 100 at tile 64: windows of 40 x 64 (the whole height), two across; against the oracle on the whole image."""
    from conftest import split_sd
    from oracle import tgsr_oracle as O
    cap, lens, _, _ = O.synthetic_batch(1, fixed_len=7)
    g = torch.Generator().manual_seed(8)
    LR = torch.rand(1, 3, 40, 100, generator=g) * 2 - 1
    with torch.no_grad():
        ref = O.sr_forward(split_sd(face_weights, "E."), split_sd(face_weights, "GL."), split_sd(face_weights, "GH."), cap,
                           lens.tolist(), LR, LR)
    r = _pipe(face_weights).upscale(LR[0].to(DEV), cap.to(DEV), 7, tile=64, tile_batch=2)
    torch.cuda.synchronize()
    for i in range(3):
        _close(r["fake"][i], ref["fake"][i][0].numpy(), FP32_TOL, "fake[%d]" % i)
        _close(r["fine"][i], ref["fine"][i][0].numpy(), FP32_TOL, "fine[%d]" % i)


def _plumbing(p, LR, LRb, cap, n, tile_batch, tol_bits=True):
    """upscale's float result == a numpy stitch of the pipeline's own per-batch __call__ outputs at the same batch composition."""
    H, W = LR.shape[1:]
    table = T.plan_tiles(H, W, 64, 16)
    pad = (-len(table)) % tile_batch
    table = torch.cat([table, table[-1:].expand(pad, -1)]).contiguous()
    caps = cap.reshape(1, -1).expand(tile_batch, -1).contiguous().to(DEV)
    lr_t, lrb_t = M.gather(LR.numpy(), table.numpy(), 64, 64), M.gather(LRb.numpy(), table.numpy(), 64, 64)
    want = {k: [np.full((3, s * H, s * W), np.nan, np.float32) for s in (2, 4, 8)] for k in ("fine", "fake")}
    for b in range(0, len(table), tile_batch):
        o = p(caps, [n] * tile_batch, torch.from_numpy(lr_t[b:b + tile_batch]).to(DEV), torch.from_numpy(lrb_t[b:b + tile_batch]).to(DEV))
        for k in want:
            for i in range(3):
                M.stitch(o[k][i].cpu().numpy(), table[b:b + tile_batch].numpy(), 64, want[k][i])
    r = p.upscale(LR.to(DEV), cap.to(DEV), n, lr_blur=LRb.to(DEV), tile=64, halo=16, tile_batch=tile_batch)
    torch.cuda.synchronize()
    for k in want:
        for i in range(3):
            assert np.array_equal(bits(r[k][i]), bits(want[k][i])), "%s[%d]" % (k, i)
    return r


def test_upscale_is_a_stitch_of_the_pipelines_own_tile_outputs_fp32(face_weights, cfg_face):
    _sds, cap, lens, LR, LRb, _ = M.face_case()
    _plumbing(_pipe(face_weights), LR[0], LRb[0], cap[0], int(lens[0]), 3)


def test_upscale_is_a_stitch_of_the_pipelines_own_tile_outputs_bf16(face_weights, cfg_face):
    _sds, cap, lens, LR, LRb, whole = M.face_case()
    from oracle import tgsr_oracle_lp as OL
    r = _plumbing(_pipe(face_weights, "bf16"), LR[0], LRb[0], cap[0], int(lens[0]), 2)
    # ... and those outputs are the image: the bf16 path's usual distance from the fp32 oracle (>= 50 dB end to end
    # against its own CPU model; 45 dB against the fp32 oracle leaves room for the rounding itself)
    psnr = OL.psnr(r["fine"][2].cpu(), torch.from_numpy(whole["fine"][2]))
    print("bf16 upscale: %.1f dB against the fp32 whole-image oracle" % psnr)
    assert psnr > 45.0


def test_upscale_output_modes(face_weights, cfg_face):
    """out="u8" is to_uint8 of the float result byte for byte; graph=True is eager bit for bit (also on its second use, when the
    captured step is only replayed); low="lr-lrblur" computes the blurred LR itself from a uint8 image."""
    from tgsr_amd import ops
    _sds, cap, lens, LR, LRb, _ = M.face_case()
    p = _pipe(face_weights)
    args = (LR[0].to(DEV), cap[0].to(DEV), int(lens[0]))
    kw = dict(lr_blur=LRb[0].to(DEV), tile=64, halo=16, tile_batch=2)
    f = p.upscale(*args, with_att=True, **kw)
    u = p.upscale(*args, out="u8", with_att=True, **kw)
    for k in ("fine", "fake"):
        for i in range(3):
            assert u[k][i].dtype == torch.uint8 and torch.equal(u[k][i], ops.to_uint8(f[k][i])), "%s[%d]" % (k, i)
    for i in range(3):
        assert u["att"][i].dtype == torch.float32 and torch.equal(u["att"][i], f["att"][i])
    for rep in range(2):
        gr = p.upscale(*args, graph=True, with_att=True, **kw)
        torch.cuda.synchronize()
        for k in ("fine", "fake", "att"):
            for i in range(3):
                assert np.array_equal(bits(gr[k][i]), bits(f[k][i])), "graph, use %d: %s[%d]" % (rep, k, i)
    # uint8 input, NetG_highweight reading LR - blur(LR): the blur is computed on the whole image, then cut
    pb = _pipe(face_weights, low="lr-lrblur")
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (3, 64, 100), generator=g, dtype=torch.uint8).to(DEV)
    from tgsr_amd.datasets import gaussian_box_params
    blur = ops.gaussian_blur_u8(img, *gaussian_box_params(2.0, 3), 3)
    a = pb.upscale(img, cap[0].to(DEV), int(lens[0]), tile=64, tile_batch=2)
    b = pb.upscale(ops.u8_normalize(img), cap[0].to(DEV), int(lens[0]), lr_blur=ops.u8_normalize(blur), tile=64, tile_batch=2)
    for i in range(3):
        assert torch.equal(a["fine"][i], b["fine"][i])
    with pytest.raises(ValueError, match="pass lr_blur"):
        pb.upscale(ops.u8_normalize(img), cap[0].to(DEV), int(lens[0]), tile=64)


def test_upscale_graph_follows_the_weights(face_weights, cfg_face):
    """The captured tile-batch step holds pointers to the weight packs of its capture: after other weights are loaded (and after
    weights change in place) upscale(graph=True) must give what eager gives on the NEW weights, not replay the old step."""
    from conftest import split_sd
    _sds, cap, lens, LR, LRb, _ = M.face_case()
    p = _pipe(face_weights)
    args = (LR[0].to(DEV), cap[0].to(DEV), int(lens[0]))
    kw = dict(lr_blur=LRb[0].to(DEV), tile=64, halo=16, tile_batch=2)
    first = p.upscale(*args, graph=True, **kw)["fine"][2].clone()
    g = torch.Generator().manual_seed(11)
    sd_gh = {k: (v * (1 + 0.05 * torch.randn(v.shape, generator=g)) if "weight" in k and v.dim() == 4 else v)
             for k, v in split_sd(face_weights, "GH.").items()}
    p.load_state_dicts(sd_GH=sd_gh)
    gr = p.upscale(*args, graph=True, **kw)
    ea = p.upscale(*args, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(ea["fine"][2], first), "the second checkpoint must change the image for this test to say anything"
    for k in ("fine", "fake"):
        for i in range(3):
            assert np.array_equal(bits(gr[k][i]), bits(ea[k][i])), "after load_state_dicts: %s[%d]" % (k, i)
    with torch.no_grad():                                                    # in place, as an optimizer step on shared modules does
        p.netGH.residual[0].block[0].weight.mul_(0.5)
    gr = p.upscale(*args, graph=True, **kw)
    ea2 = p.upscale(*args, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(ea2["fine"][2], ea["fine"][2])
    for k in ("fine", "fake"):
        for i in range(3):
            assert np.array_equal(bits(gr[k][i]), bits(ea2[k][i])), "after an in-place change: %s[%d]" % (k, i)


def test_upscale_refusals(face_weights, cfg_face):
    from tgsr_amd.trainer import SRPipeline
    _sds, cap, lens, LR, _LRb, _ = M.face_case()
    args = (LR[0].to(DEV), cap[0].to(DEV), int(lens[0]))
    p = _pipe(face_weights)
    with pytest.raises(ValueError, match="receptive radius of 16"):
        p.upscale(*args, tile=64, halo=15)
    with pytest.raises(ValueError, match="tile > 2 \\* halo"):
        p.upscale(*args, tile=32)
    with pytest.raises(ValueError, match="'f32' or 'u8'"):
        p.upscale(*args, tile=64, out="f16")
    with pytest.raises(ValueError, match="device tensor"):
        p.upscale(LR[0], cap[0].to(DEV), 9, tile=64)
    with pytest.raises(ValueError, match="weightmap"):
        SRPipeline(41, device=DEV, low="lr", weightmap=True).upscale(*args, tile=64)
    cfg_face.TREE.BRANCH_NUM = 5
    with pytest.raises(ValueError, match="x16 generators"):
        SRPipeline(41, device=DEV, low="lr", branch_num=5).upscale(*args, tile=64)
    cfg_face.TREE.BRANCH_NUM = 4
    pl = _pipe(face_weights, "bf16")                                         # bf16 / f16: 64 x 64 windows, nothing else
    with pytest.raises(ValueError, match="64 x 64 windows only"):            # a 40-row image shrinks the window to 40 x 64
        pl.upscale(LR[0, :, :40].contiguous().to(DEV), cap[0].to(DEV), 9, tile=64)
    with pytest.raises(ValueError, match="64 x 64 windows only"):            # tile 96 on 64 x 136: a 64 x 96 window
        pl.upscale(*args, tile=96)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the example path
def test_example_pyramid_is_byte_identical_to_the_reference():
    from tgsr_amd.datasets import example_pyramid
    z = load_npz("example_pyramid.npz")
    hr = torch.from_numpy(z["hr_u8"]).to(DEV)
    assert tuple(hr.shape) == (3, 83, 117)
    lists = example_pyramid(hr, scale=int(z["scale"]), u8=True)
    for name, lst in zip(("ret", "bic", "retb", "bicb"), lists):
        assert len(lst) == 4
        for i, t in enumerate(lst):
            assert t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), z["%s%d_u8" % (name, i)]), "%s[%d]" % (name, i)
    ret, bic, retb, bicb = example_pyramid(hr, scale=8)
    assert np.array_equal(bits(bic[0]), bits(z["bic0_f32"])) and np.array_equal(bits(retb[3]), bits(z["retb3_f32"]))
    assert tuple(ret[3].shape) == (3, 80, 112) and tuple(bic[0].shape) == (3, 10, 14)


def test_example_pyramid_to_upscale_to_scores(face_weights, cfg_face):
    """The whole example path for an 80 x 112 HR image: pyramid -> upscale of its 10 x 14 LR image -> PSNR / SSIM against the HR."""
    from oracle import tgsr_oracle as O
    from tgsr_amd import metrics
    from tgsr_amd.datasets import example_pyramid
    z = load_npz("example_pyramid.npz")
    hr = torch.from_numpy(z["hr_u8"]).to(DEV)[:, :80, :112].contiguous()
    ret, bic, _retb, bicb = example_pyramid(hr, scale=8, u8=True)
    cap, lens, _, _ = O.synthetic_batch(1, fixed_len=9)
    out = _pipe(face_weights).upscale(bic[0], cap[0].to(DEV), 9, lr_blur=bicb[0])
    assert tuple(out["fine"][2].shape) == (3, 80, 112)
    for k in range(3):
        sc = metrics.image_scores(out["fine"][k][None].contiguous(), ret[k + 1][None].contiguous())
        for name in ("psnr", "rmse", "psnr_y", "rmse_y", "ssim_y"):
            v = np.asarray(sc[name])
            assert v.shape == (1,) and np.isfinite(v).all(), (k, name, v)
