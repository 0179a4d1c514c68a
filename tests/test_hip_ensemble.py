"""GPU: the geometric self-ensemble (x8) - the variant gather / merge kernels (tgsr_ensemble.hip) against their numpy model bit for
bit, their custom operators and refusals, `SRPipeline.upscale(ensemble=8)` against the float64 mean of eight CPU-oracle runs and
against the model's merge of the pipeline's own outputs, its output modes, `SRPipeline.self_ensemble` and
`SRTrainer.evaluate(ensemble=8)`."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_model as E
import tiles_model as M
from conftest import FP32_TOL
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


def _groups(th, tw):
    return ((0, 8),) if th == tw else ((0, 4), (4, 4))


# 40 x 56 at tile 40: square windows, two across (the second starts at column 16); 36 x 100 at 36 x 64: rectangular windows, the two
# groups of four; 33 x 35 as one 33 x 35 window: odd sizes - no row of the image or of a variant starts on 16 bytes
CASES = [(40, 56, 40, 40, 16), (36, 100, 36, 64, 16), (33, 35, 33, 35, 0)]


def _padded(table):
    """The table with its last window once more: what a padded last batch is."""
    return torch.cat([table, table[-1:]]).contiguous()


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W,th,tw,halo", CASES)
def test_gather_equals_the_numpy_model_bit_for_bit(H, W, th, tw, halo, N, u8):
    from tgsr_amd import ops
    g = np.random.default_rng(H * 1000 + W + N)
    shape = (N, 3, H, W)
    a, b = ((g.integers(0, 256, shape, dtype=np.uint8), g.integers(0, 256, shape, dtype=np.uint8)) if u8 else
            (g.standard_normal(shape).astype(np.float32), g.standard_normal(shape).astype(np.float32)))
    table = _padded(T.plan_tiles(H, W, (th, tw), halo))
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    groups = list(_groups(th, tw)) + ([(0, 4), (4, 4)] if th == tw else [])          # a square window also in two groups
    for k0, nk in groups:
        want_a, want_b = E.gather(a, table.numpy(), th, tw, k0, nk), E.gather(b, table.numpy(), th, tw, k0, nk)
        lr, lrb = ops.d8_gather(ta, table, th, tw, k0, nk, img2=tb)
        assert lr.dtype == torch.float32 and tuple(lr.shape) == want_a.shape == tuple(lrb.shape)
        for k in range(nk):
            assert np.array_equal(bits(lr[:, :, k]), bits(want_a[:, :, k])), "variant %d" % (k0 + k)
            assert np.array_equal(bits(lrb[:, :, k]), bits(want_b[:, :, k])), "variant %d of the second image" % (k0 + k)
        again, none = ops.d8_gather(tb, table, th, tw, k0, nk)                        # without the second image; a second run
        assert none is None and np.array_equal(bits(again), bits(want_b))
    # a view that starts 4 bytes (f32) / 1 byte (u8) into its storage: the aligned forms do not apply, the values do
    flat = torch.empty(a.size + 8, dtype=ta.dtype, device=DEV)
    off = flat[1:1 + a.size].view(shape)
    off.copy_(ta)
    k0, nk = groups[0]
    assert np.array_equal(bits(ops.d8_gather(off, table, th, tw, k0, nk)[0]), bits(E.gather(a, table.numpy(), th, tw, k0, nk)))


# ------------------------------------------------------------------------------------------------ merge
def _sources(g, N, Tb, nk, C, hh, ww, wide):
    """Random variant outputs [N * (Tb + 1) * nk, C, hh, ww] for a table whose last window is repeated (the repeat holds the same
    values), normal values wide enough to clip with exact rounding ties of the mean sprinkled in; `wide`: a channel crop of a
    buffer one channel wider - a row stride larger than the dense block."""
    x = (g.standard_normal((N, Tb, nk, C, hh, ww)) * 0.9).astype(np.float32)
    ties = ((g.integers(0, 255, x.shape) + 0.5) / 127.5 - 1.0).astype(np.float32)
    x = np.where(g.random(x.shape) < 0.05, ties, x)
    x = np.concatenate([x, x[:, -1:]], 1).reshape(-1, C, hh, ww)
    dev = torch.from_numpy(x).to(DEV)
    if wide:
        buf = torch.full((x.shape[0], C + 1, hh, ww), float("nan"), device=DEV)
        buf[:, :C] = dev
        dev = buf[:, :C]
    return x, dev


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W,th,tw,halo", CASES)
def test_merge_equals_the_numpy_model_bit_for_bit(H, W, th, tw, halo, N, u8):
    """Scales 1, 2 and 8 with 3 and 7 channels (one image: the six pairs; three images: one pair per scale, so that the x8 sources
    stay small), in ONE launch; the last window of the table is there twice; every second source is a channel crop of a wider
    buffer.  NaN / sentinel bytes around and under the outputs: every pixel written, none outside."""
    from tgsr_amd import ops
    g = np.random.default_rng(H + W + 7 * N + u8)
    plain = T.plan_tiles(H, W, (th, tw), halo)
    table = _padded(plain)
    pairs = [(C, s) for C in (3, 7) for s in (1, 2, 8)] if N == 1 else [(3, 1), (7, 2), (3, 8)]
    dt, ndt = (torch.uint8, np.uint8) if u8 else (torch.float32, np.float32)
    sq = th == tw
    host_a, host_b, dev_a, dev_b, want, bufs, outs = [], [], [], [], [], [], []
    pad = 64
    for e, (C, s) in enumerate(pairs):
        xa, da = _sources(g, N, len(plain), 8 if sq else 4, C, s * th, s * tw, wide=e % 2 == 1)
        host_a.append(xa)
        dev_a.append(da)
        if not sq:
            xb, db = _sources(g, N, len(plain), 4, C, s * tw, s * th, wide=e % 2 == 1)
            host_b.append(xb)
            dev_b.append(db)
        want.append(E.merge(xa, None if sq else host_b[-1], table.numpy(), th, tw, np.zeros((N, C, s * H, s * W), ndt)))
        buf = torch.full((pad + want[-1].size + pad,), 0xA5 if u8 else float("nan"), dtype=dt, device=DEV)
        bufs.append(buf)
        outs.append(buf[pad:pad + want[-1].size].view(N, C, s * H, s * W))
    ops.d8_merge(dev_a, outs, table, H, W, th, tw, srcs_t=None if sq else dev_b)
    for e, (o, w, buf) in enumerate(zip(outs, want, bufs)):
        got = o.cpu().numpy()
        assert not (np.isnan(got).any() if not u8 else False), "output %d keeps a NaN: a pixel without a source" % e
        assert np.array_equal(bits(got), bits(w)), "output %d (C, s) = %s" % (e, pairs[e])
        guard = buf.cpu().numpy()
        for part in (guard[:pad], guard[pad + w.size:]):
            assert np.all(part == 0xA5) if u8 else np.isnan(part).all(), "output %d: a write outside the image" % e
    # two runs give equal bits
    second = [torch.full_like(o, 0x5A if u8 else float("nan")) for o in outs]
    ops.d8_merge(dev_a, second, table, H, W, th, tw, srcs_t=None if sq else dev_b)
    for o, p in zip(outs, second):
        assert np.array_equal(bits(o), bits(p))
    if u8:                                                                   # ... and the bytes are to_uint8's of the float32 mean
        mean = [torch.full(tuple(o.shape), float("nan"), device=DEV) for o in outs]
        ops.d8_merge(dev_a, mean, table, H, W, th, tw, srcs_t=None if sq else dev_b)
        for o, m in zip(outs, mean):
            assert torch.equal(o, ops.to_uint8(m))


def test_merge_of_the_gather_is_the_image():
    """The kernels end to end on an image whose values leave 3 bits of head room (multiples of 2^-10 in [-2, 2): the eight equal
    values then sum exactly): merge(gather(img)) == img bit for bit, square windows and rectangular ones."""
    from tgsr_amd import ops
    g = np.random.default_rng(4)
    for H, W, th, tw, halo in CASES:
        img = torch.from_numpy((g.integers(-2048, 2048, (2, 3, H, W)) / 1024.0).astype(np.float32)).to(DEV)
        table = T.plan_tiles(H, W, (th, tw), halo)
        parts = [ops.d8_gather(img, table, th, tw, k0, nk)[0].flatten(0, 2) for k0, nk in _groups(th, tw)]
        out = torch.full_like(img, float("nan"))
        ops.d8_merge([parts[0]], [out], table, H, W, th, tw, srcs_t=[parts[1]] if len(parts) > 1 else None)
        assert np.array_equal(bits(out), bits(img)), (H, W, th, tw)


# ------------------------------------------------------------------------------------------------ operators
def test_opcheck_of_both_operators():
    import tgsr_amd.custom_ops  # noqa: F401   (registers torch.ops.tgsr.*)
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    ops_ = torch.ops.tgsr
    basic = ("test_schema", "test_faketensor")
    chk = torch.library.opcheck
    H, W, th = 13, 21, 8
    table = T.plan_tiles(H, W, th, 2)
    tdev = table.to(DEV)
    img = torch.randint(0, 256, (2, 3, H, W), dtype=torch.uint8, device=DEV)
    fimg = torch.randn(2, 3, H, W, device=DEV)
    chk(ops_.d8_gather.default, (img, img.flip(3).contiguous(), table, tdev, th, th, 0, 8), test_utils=basic)
    chk(ops_.d8_gather.default, (fimg, None, table, tdev, th, th, 4, 4), test_utils=basic)
    lr, none = ops_.d8_gather(fimg, None, table, tdev, th, th, 0, 8)
    assert none.numel() == 0 and torch.equal(lr, ops.d8_gather(fimg, table, th, th)[0])
    rows = 2 * len(table)
    srcs = [torch.randn(rows * 8, 3, 2 * th, 2 * th, device=DEV), torch.randn(rows * 8, 5, th, th, device=DEV)]
    outs = [torch.zeros(2, 3, 2 * H, 2 * W, device=DEV), torch.zeros(2, 5, H, W, dtype=torch.uint8, device=DEV)]
    chk(ops_.d8_merge.default, (srcs, [], outs, table, tdev, H, W, th, th), test_utils=basic)
    rt = T.plan_tiles(H, W, (8, 12), 2)
    a, b = torch.randn(2 * len(rt) * 4, 3, 16, 24, device=DEV), torch.randn(2 * len(rt) * 4, 3, 24, 16, device=DEV)
    chk(ops_.d8_merge.default, ([a], [b], [outs[0]], rt, rt.to(DEV), H, W, 8, 12), test_utils=basic)
    # refusals that look at device tensors, each before anything is launched
    with pytest.raises(TgsrError, match="CPU tensors"):
        ops_.d8_gather(fimg.cpu(), None, table, table, th, th, 0, 8)
    with pytest.raises(TgsrError, match="device copy"):
        ops.d8_gather(fimg, table, th, th, table_dev=tdev[:2])
    with pytest.raises(TgsrError, match="integer scale"):
        ops.d8_merge([srcs[0][:, :, :-1]], [outs[0]], table, H, W, th, th)
    with pytest.raises(TgsrError, match="float32 or uint8"):
        ops.d8_merge([srcs[0]], [outs[0].double()], table, H, W, th, th)
    with pytest.raises(TgsrError, match="variants"):
        ops.d8_merge([srcs[0][:-1]], [outs[0]], table, H, W, th, th)
    with pytest.raises(TgsrError, match="srcs_t"):
        ops.d8_merge([a], [outs[0]], rt, H, W, 8, 12, srcs_t=[a])
    bad = table.clone()
    bad[0, 5] = bad[0, 1] + th + 1                                          # owned columns beyond the window
    with pytest.raises(TgsrError, match="owned columns"):
        ops.d8_merge(srcs, outs, bad, H, W, th, th)
    torch.cuda.synchronize()


def test_every_refusal_of_the_c_entries():
    """Each case the header names returns its code through the raw C entry, before any launch (the outputs keep their NaN)."""
    from tgsr_amd import _lib, ops
    L = _lib.lib()
    H, W, th = 13, 21, 8
    table = T.plan_tiles(H, W, th, 2)
    Tb = len(table)
    tdev = table.to(DEV)
    img = torch.randn(2, 3, H, W, device=DEV)
    out = torch.full((2, Tb, 8, 3, th, th), float("nan"), device=DEV)
    p, st = ops._p, ops._stream

    def gather(img_=img, img2=None, N=2, H_=H, W_=W, host=table, dev=tdev, Tb_=Tb, th_=th, tw_=th, k0=0, nk=8, out_=out, out2=None):
        return L.tgsr_d8_gather(p(img_), p(img2), 0, N, H_, W_, p(host), p(dev), Tb_, th_, tw_, k0, nk, p(out_), p(out2), st())

    def rows(col, val, row=1):
        bad = table.clone()
        bad[row, col] = val
        return bad

    assert gather(img_=None) == _lib.EINVAL and gather(out_=None) == _lib.EINVAL
    assert gather(img2=img) == _lib.EINVAL and gather(out2=out) == _lib.EINVAL          # the second image without its output
    assert gather(host=None) == _lib.EINVAL and gather(dev=None) == _lib.EINVAL
    assert gather(N=0) == _lib.EINVAL and gather(N=-1) == _lib.EINVAL
    for k0, nk in ((4, 8), (1, 4), (0, 2), (0, 0), (8, 4), (0, 16)):
        assert gather(k0=k0, nk=nk) == _lib.EINVAL, (k0, nk)
    rt = T.plan_tiles(H, W, (8, 12), 2)
    assert gather(host=rt, dev=rt.to(DEV), Tb_=len(rt), tw_=12) == _lib.EINVAL          # eight variants of a 8 x 12 window
    # every table rule of tgsr_tile_gather
    assert gather(Tb_=0) == _lib.EINVAL and gather(th_=H + 1) == _lib.EINVAL and gather(tw_=0) == _lib.EINVAL
    assert gather(H_=0) == _lib.EINVAL and gather(W_=(1 << 20) + 1) == _lib.EINVAL
    for bad in (rows(0, -1), rows(1, W - th + 1), rows(2, int(table[1, 0]) - 1), rows(3, int(table[1, 2])),
                rows(3, int(table[1, 0]) + th + 1), rows(4, int(table[1, 1]) - 1), rows(5, int(table[1, 4])),
                rows(5, int(table[1, 1]) + th + 1)):
        assert gather(host=bad) == _lib.EINVAL, bad[1].tolist()
    src = torch.zeros(2 * Tb * 8, 3, th, th, device=DEV)
    dst = torch.full((2, 3, H, W), float("nan"), device=DEV)

    def merge(n=1, a=src, b=None, stride=3 * th * th, dst_=dst, C=3, s=1, nk=8, N=2, host=table, dev=tdev, tw_=th, a_arr=True,
              b_arr=True, Tb_=Tb):
        vp = ctypes.c_void_p
        A = (vp * 1)(None if a is None else a.data_ptr())
        B = (vp * 1)(None if b is None else b.data_ptr())
        D = (vp * 1)(None if dst_ is None else dst_.data_ptr())
        return L.tgsr_d8_merge(n, A if a_arr else None, B if b_arr else None, (ctypes.c_int64 * 1)(stride), D, (ctypes.c_int * 1)(C),
                               (ctypes.c_int * 1)(s), (ctypes.c_int * 1)(0), nk, N, H, W, p(host), p(dev), Tb_, th, tw_, st())

    assert merge(n=0) == _lib.EINVAL and merge(n=13) == _lib.EINVAL
    assert merge(a=None) == _lib.EINVAL and merge(dst_=None) == _lib.EINVAL and merge(a_arr=False) == _lib.EINVAL
    assert merge(host=None) == _lib.EINVAL and merge(dev=None) == _lib.EINVAL
    assert merge(N=0) == _lib.EINVAL and merge(C=0) == _lib.EINVAL and merge(s=0) == _lib.EINVAL and merge(s=65) == _lib.EINVAL
    assert merge(stride=3 * th * th - 1) == _lib.EINVAL
    assert merge(nk=2) == _lib.EINVAL and merge(nk=16) == _lib.EINVAL
    assert merge(b=src) == _lib.EINVAL                                                   # srcB present with an 8-variant srcA
    assert merge(nk=4) == _lib.EINVAL and merge(nk=4, b_arr=False) == _lib.EINVAL        # ... missing with a 4-variant one
    assert merge(host=rt, dev=rt.to(DEV), Tb_=len(rt), tw_=12) == _lib.EINVAL            # eight variants, th != tw
    assert merge(host=rows(1, W - th + 1)) == _lib.EINVAL and merge(host=rows(5, int(table[1, 4]))) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dst).all())
    assert merge(b_arr=False) == 0 and gather() == 0                                     # the accepted forms of the same calls
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dst).any())


# ------------------------------------------------------------------------------------------------ SRPipeline.upscale(ensemble=8)
def _pipe(weights, dtype="fp32", **kw):
    from conftest import split_sd
    from tgsr_amd.trainer import SRPipeline
    p = SRPipeline(41, device=DEV, low=kw.pop("low", "lr"), dtype=dtype, **kw)
    return p.load_state_dicts(split_sd(weights, "E."), split_sd(weights, "GL."), split_sd(weights, "GH."))


def _close(got, want, tol, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(got - want) / (tol + tol * np.abs(want))))
    print("%s: %.3f of the tolerance %g" % (what, err, tol))
    np.testing.assert_allclose(got, want, atol=tol, rtol=tol, err_msg=what)


@pytest.mark.parametrize("H,W,tile", [(40, 56, 40), (36, 100, 64)], ids=["square", "two-groups"])
def test_upscale_ensemble_equals_the_mean_of_eight_oracle_runs(H, W, tile, face_weights, cfg_face):
    """40 x 56 at tile 40: square windows, two across, one batch of 16 rows; 36 x 100 at tile 64: windows of 36 x 64, two batches of
    8 rows (36 x 64 and 64 x 36) and one merge over both.  Expected: the float64 mean of eight runs of the CPU oracle on the
    flipped / transposed WHOLE image, each mapped back - every variant is within the tolerance, hence so is their mean."""
    cap, lens, LR, want = E.oracle_case(H, W)
    r = _pipe(face_weights).upscale(LR[0].to(DEV), cap[0].to(DEV), int(lens[0]), tile=tile, halo=16, tile_batch=2, with_att=True,
                                    ensemble=8)
    torch.cuda.synchronize()
    for i, s in enumerate((2, 4, 8)):
        assert tuple(r["fine"][i].shape) == (3, s * H, s * W) == tuple(r["fake"][i].shape)
        _close(r["fake"][i], want["fake"][i], FP32_TOL, "fake[%d]" % i)
        _close(r["fine"][i], want["fine"][i], FP32_TOL, "fine[%d]" % i)
    for i, s in enumerate((1, 2, 4)):
        assert tuple(r["att"][i].shape) == (9, s * H, s * W)
        _close(r["att"][i], want["att"][i], 2e-5, "att[%d]" % i)


def _plumbing(p, LR, LRb, cap, n, tile, tile_batch):
    """upscale(ensemble=8)'s float result == the model's merge of the pipeline's own __call__ outputs on the model's gathered
    variant batches, at the same batch composition."""
    H, W = LR.shape[1:]
    th, tw = min(tile, H), min(tile, W)
    table = T.plan_tiles(H, W, (th, tw), 16)
    pad = (-len(table)) % tile_batch
    table = torch.cat([table, table[-1:].expand(pad, -1)]).contiguous()
    groups = _groups(th, tw)
    nrows = tile_batch * groups[0][1]
    caps = cap.reshape(1, -1).expand(nrows, -1).contiguous().to(DEV)
    names = ("fine", "fake", "att")
    want = {k: [np.full((1, 9 if k == "att" else 3, s * H, s * W), np.nan, np.float32) for s in E.SCALES[k]] for k in names}
    for b in range(0, len(table), tile_batch):
        rows = table[b:b + tile_batch].numpy()
        outs = []
        for k0, nk in groups:
            x = E.gather(LR.numpy()[None], rows, th, tw, k0, nk)
            xb = E.gather(LRb.numpy()[None], rows, th, tw, k0, nk)
            o = p(caps, [n] * nrows, torch.from_numpy(x.reshape((-1,) + x.shape[3:])).to(DEV),
                  torch.from_numpy(xb.reshape((-1,) + xb.shape[3:])).to(DEV))
            outs.append({k: [t.cpu().numpy() for t in o[k]] for k in names})
        for k in names:
            for i in range(3):
                E.merge(outs[0][k][i], outs[1][k][i] if len(outs) > 1 else None, rows, th, tw, want[k][i])
    r = p.upscale(LR.to(DEV), cap.to(DEV), n, lr_blur=LRb.to(DEV), tile=tile, halo=16, tile_batch=tile_batch, with_att=True,
                  ensemble=8)
    torch.cuda.synchronize()
    for k in names:
        for i in range(3):
            assert np.array_equal(bits(r[k][i]), bits(want[k][i][0])), "%s[%d]" % (k, i)
    return r


@pytest.mark.parametrize("H,W,tile,tile_batch", [(40, 56, 40, 2), (36, 100, 64, 3)], ids=["square", "two-groups-padded"])
def test_upscale_ensemble_is_a_merge_of_the_pipelines_own_outputs_fp32(H, W, tile, tile_batch, face_weights, cfg_face):
    _sds, cap, lens, LR, LRb, _ = M.face_case()
    _plumbing(_pipe(face_weights), LR[0, :, :H, :W].contiguous(), LRb[0, :, :H, :W].contiguous(), cap[0], int(lens[0]), tile, tile_batch)


def test_upscale_ensemble_is_a_merge_of_the_pipelines_own_outputs_bf16(face_weights, cfg_face):
    """64 x 96 at tile 64: two 64 x 64 windows (the reduced-precision path's one window shape), one batch of 16 rows."""
    _sds, cap, lens, LR, LRb, _ = M.face_case()
    _plumbing(_pipe(face_weights, "bf16"), LR[0, :, :, :96].contiguous(), LRb[0, :, :, :96].contiguous(), cap[0], int(lens[0]), 64, 2)


@pytest.mark.parametrize("H,W,tile", [(40, 56, 40), (36, 100, 64)], ids=["square", "two-groups"])
def test_upscale_ensemble_output_modes(H, W, tile, face_weights, cfg_face):
    """graph=True is eager bit for bit (also on its second use, when the captured steps are only replayed); out="u8" is to_uint8 of
    the float result; ensemble=1 is the call without the keyword; other values are refused."""
    from tgsr_amd import ops
    _sds, cap, lens, LR, LRb, _ = M.face_case()
    p = _pipe(face_weights)
    args = (LR[0, :, :H, :W].contiguous().to(DEV), cap[0].to(DEV), int(lens[0]))
    kw = dict(lr_blur=LRb[0, :, :H, :W].contiguous().to(DEV), tile=tile, halo=16, tile_batch=2, with_att=True)
    f = p.upscale(*args, ensemble=8, **kw)
    u = p.upscale(*args, out="u8", ensemble=8, **kw)
    for k in ("fine", "fake"):
        for i in range(3):
            assert u[k][i].dtype == torch.uint8 and torch.equal(u[k][i], ops.to_uint8(f[k][i])), "%s[%d]" % (k, i)
    for i in range(3):
        assert u["att"][i].dtype == torch.float32 and torch.equal(u["att"][i], f["att"][i])
    for rep in range(2):
        gr = p.upscale(*args, graph=True, ensemble=8, **kw)
        torch.cuda.synchronize()
        for k in ("fine", "fake", "att"):
            for i in range(3):
                assert np.array_equal(bits(gr[k][i]), bits(f[k][i])), "graph, use %d: %s[%d]" % (rep, k, i)
    plain, one = p.upscale(*args, **kw), p.upscale(*args, ensemble=1, **kw)
    for k in ("fine", "fake", "att"):
        for i in range(3):
            assert np.array_equal(bits(plain[k][i]), bits(one[k][i]))
            assert not torch.equal(plain[k][i], f[k][i]), "the ensemble must differ from one orientation for this test to say anything"
    for bad in (3, 0, 4, "8"):
        with pytest.raises(ValueError, match="ensemble is 1 or 8"):
            p.upscale(*args, ensemble=bad, **kw)


# ------------------------------------------------------------------------------------------------ self_ensemble, evaluate
def _batch(seed, B=2):
    from oracle import tgsr_oracle as O
    cap, lens, LR, LRb = O.synthetic_batch(B, seed=seed)
    assert tuple(LR.shape) == (B, 3, 32, 32)
    return cap, lens, LR, LRb


@pytest.mark.parametrize("h,w", [(32, 32), (24, 40)], ids=["square", "rectangular"])
def test_self_ensemble_is_the_models_merge_of_the_call_on_the_variant_batch(h, w, face_weights, cfg_face):
    """[2, 3, 32, 32]: one batch of 16 rows; [2, 3, 24, 40]: two batches of 8 rows, 24 x 40 and 40 x 24, and one merge over both."""
    cap, lens, LR, LRb = _batch(70)
    if (h, w) != (32, 32):
        g = torch.Generator().manual_seed(h * 100 + w)
        LR, LRb = torch.rand(2, 3, h, w, generator=g) * 2 - 1, torch.rand(2, 3, h, w, generator=g) * 2 - 1
    p = _pipe(face_weights)
    table = np.array([[0, 0, 0, h, 0, w]], np.int32)
    groups = _groups(h, w)
    nk = groups[0][1]
    caps, rep = cap.repeat_interleave(nk, 0).to(DEV), [n for n in lens.tolist() for _ in range(nk)]
    outs = []
    for k0, _nk in groups:
        x, xb = E.gather(LR.numpy(), table, h, w, k0, nk), E.gather(LRb.numpy(), table, h, w, k0, nk)
        assert x.shape[:4] == (2, 1, nk, 3)
        o = p(caps, rep, torch.from_numpy(x.reshape((-1,) + x.shape[3:])).to(DEV), torch.from_numpy(xb.reshape((-1,) + xb.shape[3:])).to(DEV))
        outs.append({k: ([t.cpu().numpy() for t in v] if isinstance(v, (list, tuple)) else v.clone()) for k, v in o.items()})
    plain = p(cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV))
    r = p.self_ensemble(cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV))
    torch.cuda.synchronize()
    assert set(r) == set(plain)
    for k in ("fine", "fake", "att"):
        assert len(r[k]) == len(plain[k]) == 3
        for i, t in enumerate(outs[0][k]):
            s = t.shape[2] // h
            want = E.merge(t, outs[1][k][i] if len(outs) > 1 else None, table, h, w, np.full((2, t.shape[1], s * h, s * w), np.nan, np.float32))
            assert tuple(r[k][i].shape) == tuple(plain[k][i].shape) and np.array_equal(bits(r[k][i]), bits(want)), "%s[%d]" % (k, i)
    for k in ("words_emb", "sent_emb", "mask", "mu", "logvar"):
        assert tuple(r[k].shape) == tuple(plain[k].shape) and torch.equal(r[k], outs[0][k][::nk]), k


def test_evaluate_ensemble_scores_self_ensemble_and_leaves_the_trainer_as_it_was(cfg_face):
    from tgsr_amd import train
    from tgsr_amd.trainer import SRPipeline
    cfg_face.GAN.DF_DIM = 8
    torch.manual_seed(5)
    tr = train.SRTrainer(41, device=DEV, discriminators=False)

    def batches():
        for k in range(2):
            cap, lens, LR, LRb = _batch(70 + k)
            g = torch.Generator().manual_seed(80 + k)
            hr = [(torch.rand(2, 3, s, s, generator=g) * 2 - 1).to(DEV) for s in (64, 128, 256)]
            yield cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), hr

    state = lambda: ([v for m in (tr.text_encoder, tr.netGL, tr.netGH) for v in m.state_dict().values()]     # noqa: E731
                     + list(tr.avg_param_G) + [q.detach() for q in tr.params])
    before = [v.clone() for v in state()]
    ptrs = [q.data_ptr() for q in tr.params]
    modes = (tr.netGL.training, tr.netGH.training)
    res = tr.evaluate(batches(), ema=False, shave=2, ensemble=8)
    plain = tr.evaluate(batches(), ema=False, shave=2)
    assert [q.data_ptr() for q in tr.params] == ptrs and (tr.netGL.training, tr.netGH.training) == modes
    assert all(torch.equal(x, y) for x, y in zip(before, state()))
    with pytest.raises(ValueError, match="ensemble is 1 or 8"):
        tr.evaluate(batches(), ema=False, ensemble=3)
    pipe = SRPipeline(41, device=DEV, low=tr.netGH.low, branch_num=4)
    pipe.load_state_dicts(tr.text_encoder.state_dict(), tr.netGL.state_dict(), tr.netGH.state_dict())
    at = 0
    for cap, lens, LR, LRb, hr in batches():
        sc = pipe.score(pipe.self_ensemble(cap, lens, LR, LRb), hr, 2)
        for name in ("fine", "fake"):
            for k in range(3):
                for key in ("psnr", "rmse", "psnr_y", "rmse_y", "ssim_y"):
                    got = res[name][k][key][at:at + 2]
                    assert got.tobytes() == sc[name][k][key].tobytes(), (name, k, key, got, sc[name][k][key])
        at += 2
    assert res["fine"][2]["n"] == at == plain["fine"][2]["n"]
    assert not np.array_equal(res["fine"][2]["psnr"], plain["fine"][2]["psnr"])          # the "+" rows are other rows
