"""GPU: the attention panels (csrc/tgsr_attnviz.hip, torch.ops.tgsr.attn_panels, tgsr_amd/attnviz.py, SRPipeline.attention_panels)
against the fp64 model of tests/attnviz_model.py (scipy's zoom + gaussian_filter, Pillow's paste, numpy layout).

Map bytes: no byte more than 1 off the model's, and at most floor(1e-4 x the map's bytes) bytes off at all (a cap from the
arithmetic - two fp64 evaluations of one value disagree in the last bits, and a truncation follows - not a measurement; it is 0 for
every map under 10 000 bytes).  Before the device is asked, the numpy operator form M_h X M_w^T must give the model's bytes with NO
byte off for the case's seed.  conf within 1e-12 relative, the order equal.  The blend is compared with Pillow's paste of the kernel's
OWN map bytes over the model's image bytes: exactly, everywhere, separators and padding included.  The two smallest cases take the
model's bytes from tests/golden/attnviz.npz, so they do not depend on the scipy of the machine they run on.

The exhaustive blend case: the entry point takes maps of at most 128 x 128, so a 256 x 256 ramp is not a legal input; the same
(map byte, image byte) coverage comes from two 128 x 128 images (column ramps 0..127 and 128..255) under two words whose row ramps
interleave - every image byte meets 254 map bytes, 0 and 255 among them.
"""
import functools

import numpy as np
import pytest
import torch

import attnviz_model as AM
from conftest import split_sd
from test_attnviz_host import operator_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA = 180


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(img, att, lens, **kw):
    """attention_panels on numpy inputs with a leading batch axis; everything back as numpy."""
    from tgsr_amd.attnviz import attention_panels
    out = attention_panels(T(img), T(att), lens, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(att [T, h, w], image [3, Vh, Vw] float32, its bytes, the model's map bytes, conf, order by conf) of a listed case, computed
    once; the operator form is held to the model's bytes here, on the CPU."""
    _, Tn, n, h, w, u, seed = next(c for c in AM.CASES if c[0] == name)
    if name in AM.GOLDEN_CASES:
        g = AM.golden()
        att, maps, conf, order = g[name + "_att"], g[name + "_maps"], g[name + "_conf"], g[name + "_order"]
        assert att.tobytes() == AM.softmax_maps(Tn, h, w, seed).tobytes()
    else:
        att = AM.softmax_maps(Tn, h, w, seed)
        maps, conf = AM.map_bytes(att, n, u)
        order = AM.slot_order(conf, n, True)
    assert int((operator_bytes(att, n, u) != maps).sum()) == 0, "change the seed of case %s, not the cap" % name
    img = AM.image(u * h, u * w, seed)
    return att, img, AM.image_bytes(img), maps, conf, order


def check_maps(got, want, n, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    per_map = (d != 0).reshape(d.shape[0], -1).sum(axis=1)
    cap = int(1e-4 * want[0].size)
    print("%s: bytes off per map %s (cap %d of %d), largest difference %d" % (what, per_map.tolist(), cap, want[0].size, d.max()))
    assert d.max() <= 1, what
    assert per_map.max() <= cap, what
    assert (got[n:] == 0).all(), what


def check_panel(panel, maps, img_u8, order, n, K, what):
    want = AM.panel(maps, img_u8, order, n, K, ALPHA)
    assert panel.shape == want.shape, what
    assert np.array_equal(panel, want), "%s: %d panel bytes differ from Pillow's paste" % (what, int((panel != want).sum()))


@pytest.mark.parametrize("name", [c[0] for c in AM.CASES])
def test_listed_cases_against_the_model(name):
    _, Tn, n, h, w, u, seed = next(c for c in AM.CASES if c[0] == name)
    att, img, img_u8, maps, conf, order = reference(name)
    r = run(img[None], att[None], [n], with_maps=True)
    assert r["panel"].dtype == np.uint8 and r["panel"].shape == (1, u * h, n * (u * w + 2), 3)
    assert r["maps"].shape == (1, Tn, u * h, u * w) and r["conf"].dtype == np.float64 and r["order"].dtype == np.int32
    check_maps(r["maps"][0], maps, n, name)
    rel = np.abs(r["conf"][0] - conf) / np.maximum(np.abs(conf), 1e-300)
    print("%s: conf relative error %.3g" % (name, rel[:n].max()))
    assert rel[:n].max() <= 1e-12 and (r["conf"][0][n:] == 0).all()
    assert r["order"][0].tolist() == AM.slot_order(conf, n, False).tolist()
    check_panel(r["panel"][0], r["maps"][0], img_u8, r["order"][0], n, n, name)
    # by confidence, every word: the model's order, the same map bytes, Pillow's paste in that order
    s = run(img[None], att[None], [n], with_maps=True, top_k=n)
    assert s["order"][0].tolist() == order.tolist()
    assert np.array_equal(s["maps"], r["maps"]) and np.array_equal(s["conf"], r["conf"])
    check_panel(s["panel"][0], s["maps"][0], img_u8, order, n, n, name + " by conf")


def test_one_word_is_black():
    """n = 1: thresh = 2, every value of a softmax map is under it; the reference divides 0 / 0, the tile here is black."""
    att = np.ones((1, 1, 8, 8), dtype=np.float32)
    img = AM.image(32, 32, 3)
    r = run(img[None], att, [1], with_maps=True)
    assert (r["maps"] == 0).all() and r["conf"][0, 0] == 0.0 and r["order"].tolist() == [[0]]
    check_panel(r["panel"][0], r["maps"][0], AM.image_bytes(img), [0], 1, 1, "n = 1")


def test_a_map_under_the_threshold_beside_live_ones():
    att = AM.softmax_maps(5, 8, 8, 21).copy()
    att[2] = 0.25                                                      # thresh = 0.4: all of word 2 is under it
    img = AM.image(32, 32, 21)
    want, conf = AM.map_bytes(att, 5, 4)
    assert (want[2] == 0).all() and conf[2] == 0.0 and want[0].max() == 255
    assert int((operator_bytes(att, 5, 4) != want).sum()) == 0
    r = run(img[None], att[None], [5], with_maps=True, top_k=5)
    check_maps(r["maps"][0], want, 5, "dead map")
    assert (r["maps"][0, 2] == 0).all() and r["conf"][0, 2] == 0.0
    order = AM.slot_order(conf, 5, True)
    assert r["order"][0].tolist() == order.tolist()
    check_panel(r["panel"][0], r["maps"][0], AM.image_bytes(img), order, 5, 5, "dead map")


def test_batch_of_unequal_captions_is_padded_on_the_right():
    lens = [7, 3, 5]
    att = AM.softmax_maps(7, 8, 8, 31, B=3)
    img = AM.image(32, 32, 31, B=3)
    r = run(img, att, lens, with_maps=True)
    assert r["panel"].shape == (3, 32, 7 * 34, 3)
    for b, n in enumerate(lens):
        want, conf = AM.map_bytes(att[b], n, 4)
        assert int((operator_bytes(att[b], n, 4) != want).sum()) == 0
        check_maps(r["maps"][b], want, n, "batch row %d" % b)
        assert np.abs(r["conf"][b] - conf).max() <= 1e-12 * conf.max()
        check_panel(r["panel"][b], r["maps"][b], AM.image_bytes(img[b]), r["order"][b], n, 7, "batch row %d" % b)
        assert (r["panel"][b][:, n * 34:] == 0).all() and r["order"][b].tolist() == list(range(n)) + [-1] * (7 - n)


def test_top_k():
    att = AM.softmax_maps(18, 8, 8, 41, B=2)
    img = AM.image(32, 32, 41, B=2)
    lens = [18, 4]
    r = run(img, att, lens, with_maps=True, top_k=5)                   # 5 of 18; the second caption has only 4 words
    assert r["panel"].shape == (2, 32, 5 * 34, 3)
    for b, n in enumerate(lens):
        _, conf = AM.map_bytes(att[b], n, 4)
        order = AM.slot_order(conf, n, True)
        assert r["order"][b].tolist() == order.tolist()
        check_panel(r["panel"][b], r["maps"][b], AM.image_bytes(img[b]), order, n, 5, "top 5, row %d" % b)
    s = run(img[1:], att[1:, :6], [4], with_maps=True, top_k=9)        # top_k > n: K = n
    assert s["panel"].shape == (1, 32, 4 * 34, 3)
    _, conf = AM.map_bytes(att[1, :6], 4, 4)
    check_panel(s["panel"][0], s["maps"][0], AM.image_bytes(img[1]), AM.slot_order(conf, 4, True), 4, 4, "top_k > n")
    # ties go to the higher word index: two words with the same map
    tied = att[:1, :6].copy()
    tied[0, 4] = tied[0, 1]
    t = run(img[:1], tied, [6], top_k=6)
    _, conf = AM.map_bytes(tied[0], 6, 4)
    assert conf[4] == conf[1] and t["order"][0].tolist() == AM.slot_order(conf, 6, True).tolist()
    assert t["order"][0].tolist().index(4) + 1 == t["order"][0].tolist().index(1)


def test_blend_equals_pillow_on_every_image_byte_and_254_map_bytes():
    ramps = np.empty((2, 128), dtype=np.float64)
    ramps[0] = [2 * r for r in range(127)] + [255]                      # 0, 2, ..., 252, 255
    ramps[1] = [0] + [2 * r - 1 for r in range(1, 127)] + [255]         # 0, 1, 3, ..., 251, 255
    x = 3.0 + ramps + 0.5 * ((ramps > 0) & (ramps < 255))              # thresh = 1 for two words: everything stays
    att = np.broadcast_to(x[None, :, :, None], (2, 2, 128, 128)).astype(np.float32)
    img = np.broadcast_to((np.arange(128)[None, :] + 128 * np.arange(2)[:, None])[:, None, None, :], (2, 3, 128, 128)).astype(np.uint8)
    r = run(img, att, [2, 2], with_maps=True)
    seen = np.zeros((256, 256), dtype=bool)                             # [image byte][map byte]
    for b in range(2):
        for j in range(2):
            seen[img[b, 0].reshape(-1), r["maps"][b, j].reshape(-1)] = True
        check_panel(r["panel"][b], r["maps"][b], img[b], [0, 1], 2, 2, "ramps, image %d" % b)
    per_image_byte = seen.sum(axis=1)
    print("map bytes met per image byte: min %d" % per_image_byte.min())
    assert per_image_byte.min() >= 250 and seen[:, 0].all() and seen[:, 255].all()


def test_image_quantisation_is_torch_cpu_fp32():
    """alpha = 0 passes the image byte through (t = 255 i + 128 -> i): add, div, mul, round half to even, clamp - with values
    exactly on .5 and outside [-1, 1]."""
    k = np.arange(256, dtype=np.float32)
    halves = ((k + np.float32(0.5)) * np.float32(2) / np.float32(255) - np.float32(1)).astype(np.float32)
    exact = np.nextafter(halves[:128], np.float32(2))                  # ... and their upper neighbours
    rest = np.random.RandomState(5).uniform(-1.6, 1.6, 768 - 256 - 128 - 4).astype(np.float32)
    v = np.concatenate([halves, exact, rest, np.float32([-1.0, 1.0, -3.0, 2.5])]).reshape(1, 3, 16, 16)
    want = AM.image_bytes(v)
    q = ((v.astype(np.float32) + np.float32(1)) / np.float32(2)) * np.float32(255)
    assert int((q == np.floor(q) + 0.5).sum()) >= 8 and want.min() == 0 and want.max() == 255
    att = AM.softmax_maps(9, 16, 16, 15)
    r = run(v, att[None], [9], alpha=0)
    for s in range(9):
        assert np.array_equal(r["panel"][0][:, s * 18:s * 18 + 16].transpose(2, 0, 1), want[0]), s
    assert (r["panel"][0].reshape(16, 9, 18, 3)[:, :, 16:] == 0).all()


def test_uint8_input_determinism_and_graph_replay():
    from tgsr_amd.attnviz import attention_panels
    att, img, img_u8, _maps, _conf, _order = reference("rect")
    a, f, b8 = T(att[None]), T(img[None]), T(img_u8[None])
    first = attention_panels(f, a, [4], with_maps=True, top_k=3)
    again = attention_panels(f, a, [4], with_maps=True, top_k=3)
    from_u8 = attention_panels(b8, a, [4], with_maps=True, top_k=3)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        attention_panels(f, a, [4], with_maps=True, top_k=3)           # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        captured = attention_panels(f, a, [4], with_maps=True, top_k=3)
    for v in captured.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in ("panel", "conf", "order", "maps"):
        assert torch.equal(first[k], again[k]), k
        assert torch.equal(first[k], from_u8[k]), k
        assert torch.equal(first[k], captured[k]), k
    assert int(first["panel"].max()) > 0


def test_opcheck_of_the_operator():
    from tgsr_amd.attnviz import _device_operator
    att, img, img_u8, _maps, _conf, _order = reference("rect")
    Mh, Mw = _device_operator(5, 3, DEV), _device_operator(12, 3, DEV)
    basic = ("test_schema", "test_faketensor")
    op = torch.ops.tgsr.attn_panels.default
    torch.library.opcheck(op, (T(img[None]), T(att[None]), [4], Mh, Mw, 3, ALPHA, 4, False, True), test_utils=basic)
    torch.library.opcheck(op, (T(img_u8[None]), T(att[None]), [4], Mh, Mw, 3, ALPHA, 2, True, False), test_utils=basic)
    from tgsr_amd._lib import TgsrError
    with pytest.raises(TgsrError):
        op(T(img[None]), T(att[None]), [7], Mh, Mw, 3, ALPHA, 4, False, True)          # a length past T: refused on the host
    with pytest.raises(TgsrError):
        op(T(img[None]), T(att[None]), [4], Mh, Mw, 4, ALPHA, 4, False, True)          # u against the image's size


def test_reference_signatures():
    """build_super_imagesall / build_super_images2 as the reference's caller calls them (trainer_objective.py:159-165): the image on
    the CPU, the maps a list of device tensors; the result is the text strip stacked on each panel row."""
    import torch.nn.functional as F
    from tgsr_amd import attnviz
    att = AM.softmax_maps(6, 8, 8, 51, B=2)
    att[1, 4:] = 0                                                      # what the generator leaves behind a caption of 4 words
    img = torch.from_numpy(AM.image(32, 32, 51, B=2))
    caps = torch.tensor([[1, 2, 3, 4, 5, 6], [4, 2, 3, 6, 0, 0]])
    ixtoword = {1: "this", 2: "bird", 3: "has", 4: "a", 5: "mellowish", 6: "crown"}
    lens, maps = [np.int64(6), np.int64(4)], [T(att[0]), T(att[1])]
    img_set, sentences = attnviz.build_super_imagesall(img, caps, lens, ixtoword, maps, 8, vis_size=32)
    assert img_set.dtype == np.uint8 and img_set.shape == (2 * (50 + 32), 6 * 34, 3)
    assert sentences == [["this", "bird", "has", "a", "mellowish", "crown"], ["a", "bird", "has", "crown"]]
    want = run(img.numpy(), att, [6, 4])
    strip = attnviz.text_strip(caps, ixtoword, 32, n_cols=6)[0]
    for b in range(2):
        assert np.array_equal(img_set[b * 82:b * 82 + 50], strip[b * 50:(b + 1) * 50])
        assert np.array_equal(img_set[b * 82 + 50:(b + 1) * 82], want["panel"][b])
    top, _ = attnviz.build_super_images2(img, caps, lens, ixtoword, T(att), 8, vis_size=32, topK=3)
    want = run(img.numpy(), att, [6, 4], top_k=3)
    strip = attnviz.text_strip(caps, ixtoword, 32, order=want["order"], numbered=True, n_cols=3)[0]
    assert top.shape == (2 * 82, 3 * 34, 3)
    for b in range(2):
        assert np.array_equal(top[b * 82:b * 82 + 50], strip[b * 50:(b + 1) * 50])
        assert np.array_equal(top[b * 82 + 50:(b + 1) * 82], want["panel"][b])
    # an image of another size is resized to the tile first, as the reference's nn.Upsample does
    small = F.interpolate(img, size=(16, 16), mode="bilinear", align_corners=False)
    resized, _ = attnviz.build_super_imagesall(small, caps, lens, ixtoword, maps, 8, vis_size=32)
    want = run(F.interpolate(small.to(DEV), size=(32, 32), mode="bilinear", align_corners=False).cpu().numpy(), att, [6, 4])
    assert np.array_equal(resized[50:82], want["panel"][0])
    with pytest.raises(ValueError, match=r"integer multiple"):
        attnviz.build_super_imagesall(img, caps, lens, ixtoword, maps, 8, vis_size=33)


# ---- SRPipeline.attention_panels ----
@pytest.fixture()
def cfg_small():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 64
    cfg.TREE.BRANCH_NUM = 4
    yield cfg
    cfg_reset()


def test_pipeline_attention_panels(nets_small, cfg_small):
    from tgsr_amd.attnviz import attention_panels
    from tgsr_amd.trainer import SRPipeline
    g = nets_small
    p = SRPipeline(41, device=DEV, low="lr")
    p.load_state_dicts(split_sd(g, "E."), split_sd(g, "GL."), split_sd(g, "GH."))
    caps, lens = T(g["captions"]), g["cap_lens"].tolist()
    out = p(caps, lens, T(g["LR"]), T(g["LRb"]))
    B, Tn = out["att"][0].shape[:2]
    ixtoword = {i: "w%d" % i for i in range(41)}
    for stage, u in ((0, 8), (1, 4)):
        got = p.attention_panels(out, caps, lens, ixtoword=ixtoword, stage=stage, top_k=3 if stage else None)
        by_hand = attention_panels(out["fine"][-1], out["att"][stage], lens, top_k=3 if stage else None)
        K = min(3, max(lens)) if stage else max(lens)
        assert tuple(got["panel"].shape) == (B, 128, K * 130, 3)
        for k in ("panel", "conf", "order"):
            assert torch.equal(got[k], by_hand[k]), (stage, k)
        assert got["image"].dtype == np.uint8 and got["image"].shape == (B * (50 + 128), K * 130, 3)
        assert np.array_equal(got["image"][50:178], got["panel"][0].cpu().numpy()) and len(got["sentences"]) == B
    assert int(got["panel"].max()) > 0
    # an upscale result: one image, rectangular
    lr = T(AM.image(40, 24, 7))
    up = p.upscale(lr, caps[0], lens[0], with_att=True)
    r = p.attention_panels(up, caps[:1], lens[0])
    assert tuple(r["panel"].shape) == (1, 320, lens[0] * (192 + 2), 3) and tuple(r["conf"].shape) == (1, lens[0])
    by_hand = attention_panels(up["fine"][-1][None], up["att"][0][None], [lens[0]])
    assert torch.equal(r["panel"], by_hand["panel"])
    with pytest.raises(ValueError, match=r"integer multiple"):
        p.attention_panels({"att": [up["att"][0][:, :39]], "fine": [up["fine"][-1]]}, caps[:1], lens[0])
    with pytest.raises(ValueError, match=r"no attention maps"):
        p.attention_panels({"fine": up["fine"]}, caps[:1], lens[0])
