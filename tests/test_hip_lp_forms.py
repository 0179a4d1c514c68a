"""GPU: NetG_highweight's other three forms (model.py:212-298: weightmap x useAct) on the reduced-precision path and
through SRPipeline - the map / identity epilogues of the stand-alone head (tgsr_lp_conv_to3_map_fwd) and of the combine
(tgsr_lp_head_combine_map) against torch, the whole bf16 / f16 step against a CPU model of the same rounding points
(composed here from oracle/tgsr_oracle_lp.py's helpers), and the fp32 pipeline of every form against the fp32 oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import FP32_TOL, split_sd
from oracle import tgsr_oracle as O
from oracle import tgsr_oracle_lp as OL

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [("bf16", torch.bfloat16), ("f16", torch.float16)]
# the three forms the shipped checkpoint does not use: (weightmap, use_act)
FORMS = [(True, True), (False, False), (True, False)]
FORM_IDS = ["map-tanh", "scalar-identity", "map-identity"]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tgsr_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()


@pytest.fixture()
def cfg_face():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 256
    cfg.TREE.BRANCH_NUM = 4                  # the x8 generators (trainer_objective.py:74-87)
    yield cfg
    cfg_reset()


def _maps(sizes=(64, 128, 256), seed=11, const=None):
    """Non-constant maps a1.. (0.5 + 0.2 randn, fixed seed), or every map at `const`."""
    g = torch.Generator().manual_seed(seed)
    return {"a%d" % (k + 1): (torch.full((n, n), const) if const is not None else 0.5 + 0.2 * torch.randn(n, n, generator=g))
            for k, n in enumerate(sizes)}


def _weights(face_weights, weightmap, maps=None):
    sdE, sdL, sdH = (split_sd(face_weights, k) for k in ("E.", "GL.", "GH."))
    sdH = {k: v for k, v in sdH.items() if k != "a"}                 # never saved by the reference (model.py:246-248)
    if weightmap:
        sdH.update(_maps() if maps is None else maps)
    return sdE, sdL, sdH


def _pipe(face_weights, dtype, weightmap, use_act, maps=None, overlap=True):
    from tgsr_amd.trainer import SRPipeline
    p = SRPipeline(41, device=DEV, low="lr", overlap=overlap, dtype=dtype, weightmap=weightmap, use_act=use_act)
    return p.load_state_dicts(*_weights(face_weights, weightmap, maps))


def _args(B, seed=100):
    cap, lens, LR, LRb = O.synthetic_batch(B, seed=seed)
    return (cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV)), (cap, lens, LR, LRb)


def _model_high(sd, LR, SRb, LRb, dtype, use_act):
    """CPU model of the lp path's NetG_highweight for any x8 form: tgsr_oracle_lp.netg_highweight with the head
    act(conv5x5) + a_k * SRb_k (a_k = the map a%d in `sd`, else 0.5)."""
    out = OL._gh_trunk(sd, LR, dtype, None)                           # low = "lr"
    w5 = OL.rnd(sd["conv_output.0.weight"], dtype)

    def head(o, sr, k):
        c = F.conv2d(o, w5, None, 1, 2)
        return (torch.tanh(c) if use_act else c) + sd.get("a%d" % (k + 1), 0.5) * sr

    def nosum(x, p):
        s0, t0 = OL._fold(sd, p + "1.")
        s1, t1 = OL._fold(sd, p + "4.")
        return OL.conv_block(OL.conv_block(x, sd[p + "0.weight"], s0, t0, dtype, glu=True), sd[p + "3.weight"], s1, t1, dtype)

    ims = []
    out = OL._up_block(out, sd, "upscale2x.", dtype)
    ims.append(head(out, SRb[0], 0))
    out = OL._up_block(nosum(out, "residual24."), sd, "upscale4x.", dtype)
    ims.append(head(out, SRb[1], 1))
    out = OL._up_block(nosum(out, "residual48."), sd, "upscale8x.", dtype)
    ims.append(head(out, SRb[2], 2))
    return ims


def _references(sdE, sdL, sdH, cap, lens, LR, LRb, td, use_act):
    """(fp32 oracle, CPU model of the lp roundings): dicts with "fake" and "fine"."""
    with torch.no_grad():
        words, sent = O.rnn_encoder(sdE, cap, lens)
        mask = (cap == 0)[:, :words.shape[2]]
        imgs32, _, _, _ = O.g_sr_net_low(sdL, LR, sent, words, mask)
        fine32 = O.netg_highweight(sdH, LR, imgs32, LRb, "lr", use_act=use_act)[0]
        imgs, _, _, _ = OL.g_sr_net_low(sdL, LR, sent, words, mask, td)
        fine = _model_high(sdH, LR, imgs, LRb, td, use_act)
    return {"fake": imgs32, "fine": fine32}, {"fake": imgs, "fine": fine}


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("use_map", [True, False])
@pytest.mark.parametrize("B,H,W,cp", [(3, 16, 64, 32), (2, 8, 32, 64), (17, 64, 64, 32)])
def test_lp_conv_to3_map_against_torch(B, H, W, cp, use_map, tanh, K, name, td):
    from tgsr_amd import lp
    g = torch.Generator().manual_seed(K * 100 + H + B)
    x = OL.rnd(torch.randn(B, 32, H, W, generator=g), td)
    w = torch.randn(3, 32, K, K, generator=g) / (K * 32 ** 0.5)
    add = torch.randn(B, 3, H, W, generator=g)
    amap = 0.5 + 0.2 * torch.randn(H, W, generator=g)
    ref = F.conv2d(x, OL.rnd(w, td), None, 1, K // 2)
    ref = (torch.tanh(ref) if tanh else ref) + (amap if use_map else 0.4) * add
    xi = lp.from_nchw(x.to(DEV), name, cpitch=cp)
    got = lp.conv_to3_map(xi, lp.pack_to3_weight(w.to(DEV), name), K, tanh=tanh, addend=add.to(DEV), alpha=0.4,
                          amap=amap.to(DEV) if use_map else None)
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("name,td", DTYPES)
def test_lp_conv_to3_map_without_map_is_the_old_entry(name, td):
    """tgsr_lp_conv_to3_map_fwd with no map and act NONE / TANH_AXPY: exactly the bits of tgsr_lp_conv_to3_fwd; the
    new entry refuses a map without an addend term."""
    from tgsr_amd import _lib, lp
    from tgsr_amd.ops import _p, _stream
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 16, 64
    xi = lp.from_nchw(torch.randn(B, 32, H, W, generator=g).to(DEV), name, cpitch=32)
    add = torch.randn(B, 3, H, W, generator=g).to(DEV)
    for K in (3, 5):
        wp = lp.pack_to3_weight((torch.randn(3, 32, K, K, generator=g) / (K * 6.0)).to(DEV), name)
        for act in (False, True):
            old = lp.conv_to3(xi, wp, K, tanh_axpy=act, addend=add if act else None, alpha=0.5)
            new = torch.empty_like(old)
            rc = _lib.lib().tgsr_lp_conv_to3_map_fwd(lp.DT[xi.dtype], _p(xi), 32, B, 32, H, W, _p(wp), K,
                                                     _lib.ACT_TANH_AXPY if act else _lib.ACT_NONE, _p(add if act else None),
                                                     0.5, None, _p(new), _stream())
            assert rc == 0
            assert torch.equal(new, old), "K=%d act=%s" % (K, act)
        amap = torch.ones(H, W, device=DEV)
        assert _lib.lib().tgsr_lp_conv_to3_map_fwd(lp.DT[xi.dtype], _p(xi), 32, B, 32, H, W, _p(wp), K, _lib.ACT_NONE, None,
                                                   0.5, _p(amap), _p(new), _stream()) == _lib.EINVAL
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("high_tanh", [True, False])
@pytest.mark.parametrize("B", [2, 5])
def test_lp_head_combine_map(B, high_tanh, name, td):
    """tgsr_lp_head_combine_map: three scales with maps in ONE launch == scale by scale (bit for bit) == the stand-alone
    head on the same feature images (fp32 summation order), also with the low image as an input (partial_low = None);
    with no map and tanh it gives the bits of tgsr_lp_head_combine."""
    from tgsr_amd import lp
    g = torch.Generator().manual_seed(B * 7 + int(high_tanh))
    sizes, pl, ph, feats, p3s, p5s, maps = [], [], [], [], [], [], []
    for Hi, Wi in ((4, 32), (8, 64), (16, 128)):
        x = lp.from_nchw(torch.randn(B, 32, Hi, Wi, generator=g).to(DEV), name, cpitch=32)
        wp = lp.pack_upconv_weight((torch.randn(64, 32, 3, 3, generator=g) / 17.0).to(DEV), name)
        p3 = lp.pack_to3_weight((torch.randn(3, 32, 3, 3, generator=g) / 17.0).to(DEV), name)
        p5 = lp.pack_to3_weight((torch.randn(3, 32, 5, 5, generator=g) / 28.0).to(DEV), name)
        h, part3 = lp.upconv_glu_head(x, wp, 32, 64, None, None, p3, 3)
        pl.append(part3)
        ph.append(lp.upconv_glu_head(x, wp, 32, 64, None, None, p5, 5, write_out=False)[1])
        feats.append(h)
        p3s.append(p3)
        p5s.append(p5)
        sizes.append((2 * Hi, 2 * Wi))
        maps.append((0.5 + 0.2 * torch.randn(2 * Hi, 2 * Wi, generator=g)).to(DEV))
    mk = lambda: [torch.full((B, 3, H, W), float("nan"), device=DEV) for H, W in sizes]      # noqa: E731
    low, high, low1, high1 = mk(), mk(), mk(), mk()
    lp.head_combine(B, sizes, pl, ph, low, high, False, 0.4, amap=maps, high_tanh=high_tanh)
    for k in range(3):
        lp.head_combine(B, [sizes[k]], [pl[k]], [ph[k]], [low1[k]], [high1[k]], False, 0.4, amap=[maps[k]], high_tanh=high_tanh)
        assert torch.equal(low[k], low1[k]) and torch.equal(high[k], high1[k]), "scale %d: one launch != scale by scale" % k
        low_ref = lp.conv_to3(feats[k], p3s[k], 3)
        high_ref = lp.conv_to3_map(feats[k], p5s[k], 5, tanh=high_tanh, addend=low_ref, amap=maps[k])
        np.testing.assert_allclose(low[k].cpu().numpy(), low_ref.cpu().numpy(), atol=2e-5, rtol=1e-5)
        np.testing.assert_allclose(high[k].cpu().numpy(), high_ref.cpu().numpy(), atol=2e-5, rtol=1e-5)
        high2 = torch.empty_like(high[k])
        lp.head_combine(B, [sizes[k]], [None], [ph[k]], [low[k]], [high2], False, 0.4, amap=[maps[k]], high_tanh=high_tanh)
        assert torch.equal(high2, high[k]), "scale %d: the low image as an input differs" % k
    # the new entry without maps, tanh: the old entry's bits (a list of absent maps selects tgsr_lp_head_combine_map)
    lo_old, hi_old, lo_new, hi_new = mk(), mk(), mk(), mk()
    lp.head_combine(B, sizes, pl, ph, lo_old, hi_old, False, 0.4)
    lp.head_combine(B, sizes, pl, ph, lo_new, hi_new, False, 0.4, amap=[None, None, None], high_tanh=True)
    for k in range(3):
        assert torch.equal(lo_new[k], lo_old[k]) and torch.equal(hi_new[k], hi_old[k])


def test_opcheck_lp_form_ops():
    from tgsr_amd import custom_ops  # noqa: F401   (registers torch.ops.tgsr.*)
    from tgsr_amd import lp
    T = torch.ops.tgsr
    basic = ("test_schema", "test_faketensor")
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g).to(DEV)                  # noqa: E731
    h32 = lp.from_nchw(R(2, 32, 16, 64), "bf16", cpitch=64)
    p5 = lp.pack_to3_weight(R(3, 32, 5, 5) / 28.0, "bf16")
    torch.library.opcheck(T.lp_conv_to3_map.default, (h32, p5, 5, True, R(2, 3, 16, 64), 0.5, R(16, 64)), test_utils=basic)
    torch.library.opcheck(T.lp_conv_to3_map.default, (h32, p5, 5, False, R(2, 3, 16, 64), 0.5, None), test_utils=basic)
    xi = lp.from_nchw(R(2, 64, 8, 32), "bf16", cpitch=64)
    wu = lp.pack_upconv_weight(R(64, 64, 3, 3) / 24.0, "bf16")
    p3 = lp.pack_to3_weight(R(3, 32, 3, 3) / 17.0, "bf16")
    part3 = lp.upconv_glu_head(xi, wu, 64, 64, None, None, p3, 3, write_out=False)[1]
    part5 = lp.upconv_glu_head(xi, wu, 64, 64, None, None, p5, 5, write_out=False)[1]
    low, high = torch.empty(2, 3, 16, 64, device=DEV), torch.empty(2, 3, 16, 64, device=DEV)
    torch.library.opcheck(T.lp_head_combine_map.default, ([16], [64], [part3], [part5], [low], [high], [R(16, 64)], False, False,
                                                          0.5), test_utils=basic)
    torch.library.opcheck(T.lp_head_combine_map.default, ([16], [64], [part3], [part5], [low], [high], [], False, False, 0.5),
                          test_utils=basic)


# ------------------------------------------------------------------------------------------------ pipeline
def _check_against_model(out, ref32, model, name):
    for k in ("fake", "fine"):
        for i in range(3):
            got = out[k][i].cpu()
            p32, pm, pmodel = OL.psnr(got, ref32[k][i]), OL.psnr(got, model[k][i]), OL.psnr(model[k][i], ref32[k][i])
            assert abs(p32 - pmodel) < 1.0, "%s %s[%d]: %.2f dB vs fp32, the CPU model predicts %.2f" % (name, k, i, p32, pmodel)
            assert pm > pmodel + (3.0 if name == "f16" else 2.0), \
                "%s %s[%d]: only %.2f dB against the CPU model of the same roundings (model vs fp32 %.2f)" % (name, k, i, pm, pmodel)


@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("B", [2, 16])
def test_lp_forms_full_size(B, form, name, td, cfg_face, face_weights):
    weightmap, use_act = form
    args, (cap, lens, LR, LRb) = _args(B)
    ref32, model = _references(*_weights(face_weights, weightmap), cap, lens.tolist(), LR, LRb, td, use_act)
    out = _pipe(face_weights, name, weightmap, use_act)(*args)
    torch.cuda.synchronize()
    _check_against_model(out, ref32, model, name)
    print("%s %s B=%d: finest image %.1f dB against fp32" % (name, FORM_IDS[FORMS.index(form)], B,
                                                             OL.psnr(out["fine"][2].cpu(), ref32["fine"][2])))


@pytest.mark.parametrize("name", ["bf16", "f16"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_lp_forms_fused_heads_equal_standalone(form, name, cfg_face, face_weights, monkeypatch):
    from tgsr_amd import lp_pipeline
    args, _ = _args(3, seed=31)
    assert lp_pipeline.FUSE_HEADS
    fused = _pipe(face_weights, name, *form)(*args)
    monkeypatch.setattr(lp_pipeline, "FUSE_HEADS", False)
    plain = _pipe(face_weights, name, *form)(*args)
    torch.cuda.synchronize()
    for k in ("fake", "fine"):
        for i in range(3):
            np.testing.assert_allclose(fused[k][i].cpu().numpy(), plain[k][i].cpu().numpy(), atol=3e-5, rtol=1e-5)
    for i in range(3):
        assert torch.equal(fused["att"][i], plain["att"][i])


@pytest.mark.parametrize("name", ["bf16", "f16"])
@pytest.mark.parametrize("use_act", [True, False])
@pytest.mark.parametrize("fuse", [True, False])
def test_lp_constant_maps_reduce_to_the_scalar_form(fuse, use_act, name, cfg_face, face_weights, monkeypatch):
    from tgsr_amd import lp_pipeline
    monkeypatch.setattr(lp_pipeline, "FUSE_HEADS", fuse)
    args, _ = _args(4, seed=5)
    a = _pipe(face_weights, name, True, use_act, maps=_maps(const=0.5))(*args)
    b = _pipe(face_weights, name, False, use_act)(*args)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(a["fake"][i], b["fake"][i])
        np.testing.assert_allclose(a["fine"][i].cpu().numpy(), b["fine"][i].cpu().numpy(), atol=1e-6, rtol=0)


@pytest.mark.parametrize("name", ["bf16", "f16"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_lp_forms_hipgraph_replay_equals_eager(form, name, cfg_face, face_weights):
    B = 4
    pipe = _pipe(face_weights, name, *form)
    args, _ = _args(B)
    a = pipe(*args)
    torch.cuda.synchronize()
    pipe.capture(*args)
    r = pipe.replay()
    torch.cuda.synchronize()
    for k in ("fake", "fine", "att"):
        for i in range(3):
            assert torch.equal(r[k][i], a[k][i]), "replay differs from eager (%s[%d])" % (k, i)
    for seed in (7, 8):                                               # new batches through the captured step
        a2, _ = _args(B, seed=seed)
        g2 = pipe.replay(*a2)
        torch.cuda.synchronize()
        g2 = {k: [t.clone() for t in g2[k]] for k in ("fake", "fine")}
        e2 = pipe(*a2)
        torch.cuda.synchronize()
        for k in ("fake", "fine"):
            for i in range(3):
                assert torch.equal(g2[k][i], e2[k][i]), "replay on batch %d: %s[%d] differs from eager" % (seed, k, i)
    # two independent batches as parallel branches of one graph
    batches = [_args(B, seed=s)[0] for s in (21, 22)]
    eager = []
    for bt in batches:
        o = pipe(*bt)
        torch.cuda.synchronize()
        eager.append([t.clone() for t in o["fine"]])
    pipe.capture(*batches[0], lanes=2)
    outs = pipe.replay(*[[bt[j] for bt in batches] for j in range(4)])
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        for i in range(3):
            assert torch.equal(o["fine"][i], e[i])


@pytest.mark.parametrize("name", ["bf16", "f16"])
@pytest.mark.parametrize("use_act", [True, False])
def test_lp_in_place_map_update_reaches_the_next_call(use_act, name, cfg_face, face_weights):
    args, _ = _args(3, seed=9)
    pipe = _pipe(face_weights, name, True, use_act)
    before = pipe(*args)["fine"][1].clone()
    pipe.netGH.a2.data.mul_(0.5)
    got = pipe(*args)
    maps = {k: getattr(pipe.netGH, k).detach().cpu().clone() for k in ("a1", "a2", "a3")}
    fresh = _pipe(face_weights, name, True, use_act, maps=maps)(*args)
    torch.cuda.synchronize()
    assert not torch.equal(got["fine"][1], before)
    for i in range(3):
        assert torch.equal(got["fine"][i], fresh["fine"][i]), "fine[%d] after the in-place update" % i


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_weightmap_with_an_lr_of_the_wrong_size(name, cfg_face, face_weights):
    pipe = _pipe(face_weights, name, True, True)
    cap, lens, LR, LRb = O.synthetic_batch(2, lr=64)
    with pytest.raises(ValueError, match="a1 is"):
        pipe(cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV))
    torch.cuda.synchronize()


def test_refused_forms(cfg_face):
    from tgsr_amd.trainer import SRPipeline
    for dt in ("bf16", "f16"):
        with pytest.raises(ValueError, match="16 x 16"):
            SRPipeline(41, device=DEV, dtype=dt, branch_num=5, weightmap=True)
    for dt in ("fp32", "bf16"):
        with pytest.raises(ValueError, match="tanh-free"):
            SRPipeline(41, device=DEV, dtype=dt, branch_num=5, use_act=False)


# ------------------------------------------------------------------------------------------------ fp32 pipeline
@pytest.mark.parametrize("form", [(False, True)] + FORMS, ids=["shipped"] + FORM_IDS)
@pytest.mark.parametrize("overlap", [True, False])
def test_fp32_pipeline_every_x8_form(form, overlap, cfg_face, face_weights):
    weightmap, use_act = form
    args, (cap, lens, LR, LRb) = _args(2)
    sdE, sdL, sdH = _weights(face_weights, weightmap)
    ref = O.sr_forward(sdE, sdL, {k: v for k, v in sdH.items() if not k.startswith("a")}, cap, lens.tolist(), LR, LRb)
    with torch.no_grad():
        fine = O.netg_highweight(sdH, LR, ref["fake"], LRb, "lr", use_act=use_act)[0]
    pipe = _pipe(face_weights, "fp32", weightmap, use_act, overlap=overlap)
    out = pipe(*args)
    torch.cuda.synchronize()
    for i in range(3):
        np.testing.assert_allclose(out["fake"][i].cpu().numpy(), ref["fake"][i].numpy(), atol=FP32_TOL, rtol=FP32_TOL)
        np.testing.assert_allclose(out["fine"][i].cpu().numpy(), fine[i].numpy(), atol=FP32_TOL, rtol=FP32_TOL)
    pipe.capture(*args)
    r = pipe.replay()
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(r["fine"][i], out["fine"][i])


def _x16_heads(sdH, LR, SRb, LRb, maps):
    """models16.NetG_highweight(weightmap=True).forward restated in torch: the oracle's x16 trunk, heads
    tanh(conv5x5(out_k)) + a_k * SRb_k with the maps a1..a4 (models16.py:150, 159, 167, 175)."""
    ims = []
    w5 = sdH["conv_output.0.weight"]
    out = O.conv_bn_glu(LR, sdH, "convin.")
    r = 0
    while ("residual.%d.block.0.weight" % r) in sdH:
        out = O.res_block(out, sdH, "residual.%d." % r)
        r += 1
    out = O.up_block(out, sdH, "upscale2x.")
    ims.append(torch.tanh(F.conv2d(out, w5, None, 1, 2)) + maps[0] * SRb[0])
    out = O.up_block(O.residual_nosum(out, sdH, "residual24."), sdH, "upscale4x.")
    ims.append(torch.tanh(F.conv2d(out, w5, None, 1, 2)) + maps[1] * SRb[1])
    for k in (2, 3):
        out = O.up_block(O.residual_nosum(out, sdH, "residual48."), sdH, "upscale8x.")
        ims.append(torch.tanh(F.conv2d(out, w5, None, 1, 2)) + maps[k] * SRb[k])
    return ims


def _x16_weightmap_state(seed=5):
    """Seeded x16 generator parameters (models16 state_dicts) of the weight-map form: maps a1..a4 = 0.5 + 0.2 randn, BatchNorm
    statistics randomised so eval-mode BN does something."""
    from tgsr_amd import models16
    from tgsr_amd.synthetic import random_init_
    gl, gh = models16.G_SR_NET_low(), models16.NetG_highweight(weightmap=True, low="lr")
    random_init_(gl, seed), random_init_(gh, seed + 1)
    g = torch.Generator().manual_seed(seed)
    for m in list(gl.modules()) + list(gh.modules()):
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    maps = _maps(sizes=(32, 64, 128, 256), seed=seed + 2)
    with torch.no_grad():
        for k, v in maps.items():
            getattr(gh, k).copy_(v)
    return ({k: v.detach().clone() for k, v in gl.state_dict().items()},
            {k: v.detach().clone() for k, v in gh.state_dict().items()}, [maps["a%d" % k] for k in (1, 2, 3, 4)])


def test_fp32_pipeline_x16_weightmap_at_16x16(cfg_face):
    """The x16 weight-map form through SRPipeline (fp32), at the 16 x 16 LR its maps are sized for, against the fp32
    oracle's x16 G_SR_NET_low and the heads restated in torch; eager and replayed."""
    from tgsr_amd.trainer import SRPipeline
    sdE, _, _ = O.random_state(seed=2)
    sdL, sdH, maps = _x16_weightmap_state()
    assert "a" not in sdH and "a4" in sdH
    cap, lens, LR, LRb = O.synthetic_batch(2, lr=16)
    with torch.no_grad():
        words, sent = O.rnn_encoder(sdE, cap, lens.tolist())
        mask = (cap == 0)[:, :words.shape[2]]
        imgs, _, _, _ = O.g_sr_net_low16(sdL, LR, sent, words, mask)
        fine = _x16_heads(sdH, LR, imgs, LRb, maps)
    pipe = SRPipeline(41, device=DEV, low="lr", dtype="fp32", branch_num=5, weightmap=True)
    pipe.load_state_dicts(sdE, sdL, sdH)
    args = (cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV))
    out = pipe(*args)
    torch.cuda.synchronize()
    assert [tuple(t.shape[2:]) for t in out["fine"]] == [(32, 32), (64, 64), (128, 128), (256, 256)]
    for i in range(4):
        np.testing.assert_allclose(out["fake"][i].cpu().numpy(), imgs[i].numpy(), atol=FP32_TOL, rtol=FP32_TOL)
        np.testing.assert_allclose(out["fine"][i].cpu().numpy(), fine[i].numpy(), atol=FP32_TOL, rtol=FP32_TOL)
    eager = [f.clone() for f in out["fine"]]
    pipe.capture(*args)
    rep = pipe.replay()
    torch.cuda.synchronize()
    for a, b in zip(rep["fine"], eager):
        assert torch.equal(a, b)
