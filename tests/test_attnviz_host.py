"""CPU: what the attention panels (tgsr_amd/attnviz.py, csrc/tgsr_attnviz.hip) do on the host, and what tests/test_hip_attnviz.py
rests on.

  * `expand_operator` against the scipy model (tests/attnviz_model.py) applied to unit vectors: entries within 1e-14 (rows sum to 1
    and entries are <= 1, so that is a few ulps of the largest entry), row sums within 1e-14 of 1;
  * the operator form M_h X M_w^T gives the bytes of the separable scipy model on the small cases (the GPU test asserts the same
    for every case it runs);
  * the panel's layout arithmetic, the workspace size, the tie rule of the ordering (the model's, which the kernel is held to);
  * `text_strip`: shape, background value 1, the sentence lists, text only inside the cells of the words drawn;
  * the C entry points are declared, bound and exported, and refuse every bad argument before any HIP call; the host check of the
    caption lengths;
  * the fixture regenerates bit-identically; the `miscc.utils` stubs still refuse, and name tgsr_amd.attnviz.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import attnviz_model as AM


def _L():
    from tgsr_amd import _lib
    return _lib, _lib.lib()


# ---- expand_operator ----
@pytest.mark.parametrize("a,u", [(8, 4), (5, 3), (32, 8), (128, 2), (16, 1)])
def test_expand_operator_is_the_scipy_model_on_unit_vectors(a, u):
    from tgsr_amd.attnviz import expand_operator
    M = expand_operator(a, u)
    assert M.dtype == np.float64 and M.shape == (a * u, a)
    ref = np.stack([AM.expand(np.eye(a)[k], u) for k in range(a)], axis=1)
    assert float(np.abs(M - ref).max()) <= 1e-14
    assert float(np.abs(M.sum(axis=1) - 1.0).max()) <= 1e-14
    assert expand_operator(a, u) is M                                   # cached
    if u == 1:
        assert (M == np.eye(a)).all()


def test_expand_operator_refuses_nonsense():
    from tgsr_amd.attnviz import expand_operator
    for a, u in ((0, 2), (4, 0)):
        with pytest.raises(ValueError):
            expand_operator(a, u)


def operator_bytes(att, n, u):
    """The bytes of the numpy operator form M_h X M_w^T (what the kernel evaluates on the fp64 MFMA)."""
    from tgsr_amd.attnviz import expand_operator
    Mh, Mw = expand_operator(att.shape[1], u), expand_operator(att.shape[2], u)
    return AM.map_bytes(att, n, u, expand_fn=lambda X, _u: Mh @ X @ Mw.T)[0]


@pytest.mark.parametrize("case", [c for c in AM.CASES if c[0] in ("reflect", "rect", "noblur")], ids=lambda c: c[0])
def test_operator_form_gives_the_models_bytes(case):
    name, T, n, h, w, u, seed = case
    att = AM.softmax_maps(T, h, w, seed)
    ref, conf = AM.map_bytes(att, n, u)
    assert int((operator_bytes(att, n, u) != ref).sum()) == 0
    assert ref[:n].max() == 255 and (ref[n:] == 0).all() and (conf[:n] >= 0).all()


# ---- layout, workspace, ordering ----
def test_panel_layout_arithmetic():
    from tgsr_amd import attnviz
    assert attnviz.panel_width(18, 256) == 18 * 258 and attnviz.FONT_MAX == 50
    maps = np.full((3, 4, 6), 200, dtype=np.uint8)
    img = np.full((3, 4, 6), 100, dtype=np.uint8)
    p = AM.panel(maps, img, np.array([2, 0, 1], dtype=np.int32), 2, 3, 180)
    assert p.shape == (4, 3 * 8, 3)
    t = 200 * 180 + 100 * 75 + 128
    assert (p[:, 0:6] == (((t >> 8) + t) >> 8)).all() and (p[:, 8:14] == p[:, 0:6]).all()
    assert (p[:, 6:8] == 0).all() and (p[:, 14:] == 0).all()             # separators; the third slot is behind the caption
    M, L = _L()
    for B, T, h, w, u in ((2, 5, 8, 8, 4), (1, 6, 5, 12, 3), (16, 18, 32, 32, 8), (1, 1, 2, 2, 1)):
        Vh, Vw = u * h, u * w
        assert L.tgsr_attn_panels_ws_elems(B, T, h, w, u) == B * T * (Vh * Vw + 2 * ((Vh + 15) // 16))
    for bad in ((0, 5, 8, 8, 4), (1, 0, 8, 8, 4), (1, 5, 1, 8, 4), (1, 5, 8, 129, 1), (1, 5, 8, 8, 0), (1, 5, 128, 128, 5),
                (1, 65, 8, 8, 4)):
        assert L.tgsr_attn_panels_ws_elems(*bad) == 0, bad


def test_ordering_ties_go_to_the_higher_word_index():
    """The rule the GPU test holds the kernel's `order` to, and the strip's cells follow the same table."""
    conf = np.array([0.5, 2.0, 0.5, 0.0, 2.0, 9.0])
    assert AM.slot_order(conf, 5, True).tolist() == [4, 1, 2, 0, 3, -1]   # word 5 is behind the caption
    assert AM.slot_order(conf, 6, True).tolist() == [5, 4, 1, 2, 0, 3]
    assert AM.slot_order(conf, 3, False).tolist() == [0, 1, 2, -1, -1, -1]
    assert AM.slot_order(np.zeros(4), 4, True).tolist() == [3, 2, 1, 0]
    from tgsr_amd.attnviz import text_strip
    strip, _ = text_strip(np.array([[1, 2, 3, 4, 5, 6]]), IXTOWORD, 64, order=AM.slot_order(conf, 5, True)[None], n_cols=6)
    assert _cells_with_text(strip, 0, 64) == [0, 1, 2, 3, 4]


# ---- text_strip ----
IXTOWORD = {1: "this", 2: "bird", 3: "has", 4: "a", 5: "mellowish", 6: "crown"}


def _cells_with_text(strip, b, vis_w):
    rows = strip[b * 50:(b + 1) * 50]
    cols = np.flatnonzero((rows != 1).any(axis=(0, 2)))
    return sorted(set((cols // (vis_w + 2)).tolist()))


def test_text_strip():
    from tgsr_amd.attnviz import text_strip
    caps = torch.tensor([[1, 2, 3, 4, 5, 6], [4, 2, 0, 0, 0, 0]])
    strip, sentences = text_strip(caps, IXTOWORD, 256)
    assert strip.dtype == np.uint8 and strip.shape == (100, 6 * 258, 3)
    assert sentences == [["this", "bird", "has", "a", "mellowish", "crown"], ["a", "bird"]]
    assert strip.min() == 1 and strip.max() == 255                      # an np.ones background under white text
    assert _cells_with_text(strip, 0, 256) == [0, 1, 2, 3, 4, 5] and _cells_with_text(strip, 1, 256) == [0, 1]
    # the cells follow `order`; a slot of -1 and a word behind the sentence stay empty; n_cols sets the width
    strip2, s2 = text_strip(caps, IXTOWORD, 256, order=[[5, 0, -1], [1, 4, 0]], numbered=True, n_cols=3)
    assert strip2.shape == (100, 3 * 258, 3) and s2 == sentences
    assert _cells_with_text(strip2, 0, 256) == [0, 1] and _cells_with_text(strip2, 1, 256) == [0, 2]
    one, s1 = text_strip(np.array([3, 0]), IXTOWORD, 64)
    assert one.shape == (50, 66, 3) and s1 == [["has"]]


# ---- the ABI ----
def test_abi_bindings_exist():
    M, L = _L()
    assert len(M.SIGNATURES["tgsr_attn_panels"][1]) == 20 and M.SIGNATURES["tgsr_attn_panels"][0] is ctypes.c_int
    assert len(M.SIGNATURES["tgsr_attn_panels_ws_elems"][1]) == 5 and M.SIGNATURES["tgsr_attn_panels_ws_elems"][0] is ctypes.c_int64
    assert hasattr(L, "tgsr_attn_panels") and hasattr(L, "tgsr_attn_panels_ws_elems")
    import tgsr_amd.custom_ops  # noqa: F401
    have = {str(s) for s in torch._C._jit_get_all_schemas() if s.name.startswith("tgsr::")}
    assert ("tgsr::attn_panels(Tensor images, Tensor att, int[] cap_lens, Tensor Mh, Tensor Mw, int u, int alpha, int K, "
            "bool by_conf, bool with_maps) -> (Tensor, Tensor, Tensor, Tensor)") in have


def test_entry_point_refuses_before_any_hip_call():
    """No device here: every refusal below returns from the argument check, the pointers (host memory) are never followed."""
    M, L = _L()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(att=p, lens=p, img=p, f32=1, Mh=p, Mw=p, B=2, T=5, h=8, w=8, u=4, alpha=180, K=5, by_conf=0, ws=p, panel=p, maps=None,
              conf=p, order=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.tgsr_attn_panels(a["att"], a["lens"], a["img"], a["f32"], a["Mh"], a["Mw"], a["B"], a["T"], a["h"], a["w"], a["u"],
                                  a["alpha"], a["K"], a["by_conf"], a["ws"], a["panel"], a["maps"], a["conf"], a["order"], None)
    for kw in (dict(att=None), dict(lens=None), dict(img=None), dict(Mh=None), dict(Mw=None), dict(ws=None), dict(panel=None),
               dict(conf=None), dict(order=None), dict(B=0), dict(T=0), dict(K=0), dict(K=6), dict(u=0), dict(u=-1),
               dict(alpha=-1), dict(alpha=256)):
        assert call(**kw) == M.EINVAL, kw
    for kw in (dict(h=1), dict(w=1), dict(h=129), dict(w=129), dict(h=0), dict(u=65), dict(h=128, u=5), dict(w=128, u=5),
               dict(T=65, K=5)):
        assert call(**kw) == M.EUNSUPPORTED, kw
    assert all(v == 0.0 for v in buf)


def test_cap_lens_are_checked_on_the_host():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    assert ops.check_cap_lens(torch.tensor([5, 1, 3]), 3, 5) == [5, 1, 3]
    for bad in ([0, 2, 3], [1, 6, 3], [1, 2], [-1, 2, 3]):
        with pytest.raises(TgsrError, match=r"cap_lens"):
            ops.check_cap_lens(bad, 3, 5)
    # the op looks at the lengths before it looks for a device, and refuses CPU tensors after
    att, img = torch.zeros(3, 5, 8, 8), torch.zeros(3, 3, 32, 32)
    M = torch.zeros(32, 8, dtype=torch.float64)
    with pytest.raises(TgsrError, match=r"cap_lens"):
        ops.attn_panels(img, att, [1, 6, 3], M, M, 4, 180, 5, False, False)
    with pytest.raises(TgsrError, match=r"HIP tensors"):
        ops.attn_panels(img, att, [1, 5, 3], M, M, 4, 180, 5, False, False)
    from tgsr_amd import attnviz
    with pytest.raises(ValueError, match=r"integer multiple"):
        attnviz.attention_panels(torch.zeros(3, 3, 30, 32), att, [1, 5, 3])
    with pytest.raises(ValueError, match=r"integer multiple"):
        attnviz.attention_panels(torch.zeros(3, 3, 32, 16), att, [1, 5, 3])
    assert list(inspect.signature(attnviz.build_super_imagesall).parameters) == [
        "real_imgs", "captions", "cap_lens", "ixtoword", "attn_maps", "att_sze", "att_sze1", "vis_size"]
    assert list(inspect.signature(attnviz.build_super_images2).parameters) == [
        "real_imgs", "captions", "cap_lens", "ixtoword", "attn_maps", "att_sze", "att_sze1", "vis_size", "topK"]
    assert inspect.signature(attnviz.build_super_images2).parameters["topK"].default == 5


# ---- the fixture, the stubs ----
def test_fixture_regenerates_bit_identically():
    sys.path.insert(0, os.path.dirname(AM.GOLDEN))
    import make_attnviz_golden as G
    old, new = AM.golden(), G.build()
    assert sorted(old.files) == sorted(new)
    for k, v in new.items():
        assert old[k].dtype == v.dtype and old[k].shape == v.shape and old[k].tobytes() == v.tobytes(), k
    assert old["reflect_maps"].shape == (5, 32, 32) and old["rect_maps"].shape == (6, 15, 36)
    for name, n, u in (("reflect", 5, 4), ("rect", 4, 3)):               # ... and the operator form gives the recorded bytes
        assert int((operator_bytes(old[name + "_att"], n, u) != old[name + "_maps"]).sum()) == 0
    assert (old["rect_maps"][4:] == 0).all() and old["rect_order"].tolist()[4:] == [-1, -1]


def test_miscc_utils_stubs_still_refuse_and_name_the_module():
    from tgsr_amd.miscc import utils
    for name in ("build_super_images", "build_super_images2", "build_super_imagesall"):
        with pytest.raises(NotImplementedError, match=r"tgsr_amd\.attnviz"):
            getattr(utils, name)(None, None, None, None, None)
