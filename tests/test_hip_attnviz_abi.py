"""GPU: the attention-panel launch (tgsr_amd/csrc/tgsr_attnviz.hip) held to its C ABI contract, called directly through ctypes.

    tgsr_attn_panels   tgsr_attn_panels_ws_elems

tests/test_hip_attnviz.py reaches it through attention_panels on allocator memory - panel and maps always on 256 bytes, cap_lens
checked on the host, the map bytes within one of a scipy model.  Here every device operand of a call - att, the DEVICE cap_lens, the
image, Mh, Mw, the fp64 workspace of exactly tgsr_attn_panels_ws_elems doubles, conf, order, panel, maps - lies in ONE guarded arena
(tests/arena.py); panel and maps at every byte offset from a 16-byte boundary (the kernel picks 16-byte stores or single bytes from
the address), ws and conf on 8 bytes and not on 16.  After every accepted call: the arena's check (guard bands, the bytes around a
byte operand, every input bit-unchanged, every output written whole, maps untouched where it is NULL), a second call from the
re-armed state with the workspace holding a finite constant gives the same bits, and panel, maps, conf and order are the numpy
model's (tests/test_attnviz_abi_host.py: panels_model), BIT-EXACT: the inputs are chosen so that every fp64 product and sum is
exact in any order, which the host file proves for every row.  The arena's pattern read as a double is a finite 3e307, as a float a
NaN: a workspace double read before it is written, or a map behind the caption that is read, shows in the bytes.

The table, the cases, the model, the wrong kernels each row is there to catch and the refusals live in the host file, which checks
them without a GPU; this file runs them.  It imports neither Pillow nor scipy.
"""
import numpy as np
import pytest
import torch

import test_attnviz_abi_host as H
from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    word = {1: np.uint8, 4: np.int32, 8: np.int64}[got.dtype.itemsize]
    diff = got.view(word) != ref.view(word)
    assert not diff.any(), "%s: %d of %d elements differ in their bits from the model, first at %s: %r, not %r" % (
        what, int(diff.sum()), diff.size, tuple(int(i) for i in np.argwhere(diff)[0]), got[diff][0], ref[diff][0])


def _twice(a, call, outs):
    M, _ = H._lib()
    assert call() == M.OK
    a.check()
    got = [o.read().numpy().copy() for o in outs]
    a.rearm(ws_fill=1.5)
    assert call() == M.OK
    a.check()
    for g, o in zip(got, outs):
        assert g.tobytes() == o.read().numpy().tobytes(), "a second call gives other bits"
    return got


@pytest.mark.parametrize("row", H.rows(), ids=H.row_id)
def test_attn_panels(row):
    c = row[3]
    _, L = H._lib()
    att, img, Mh, Mw = H.inputs(c["name"])
    e = H.expected(c["name"])
    B, T, h, w, u, K = c["B"], c["T"], c["h"], c["w"], c["u"], c["K"]
    a = Arena(DEV)
    r_att = a.place_input(H._t(att), skew=1)
    r_len = a.place_input(H._t(np.array(c["dev_lens"], np.int32)), skew=3)
    r_img = a.place_input_u8(H._t(img), lead=3) if img.dtype == np.uint8 else a.place_input(H._t(img), skew=1)
    r_mh, r_mw = a.place_input(H._t(np.array(Mh)), skew=2), a.place_input(H._t(np.array(Mw)), skew=2)
    n = L.tgsr_attn_panels_ws_elems(B, T, h, w, u)
    assert n == H.ws_elems(B, T, h, w, u)
    ws = a.place_ws(2 * n, align=16, skew=2)
    conf = a.place_output((B, T), dtype=torch.float64, skew=2)
    order = a.place_output((B, T), dtype=torch.int32, skew=1)
    po, mo = c["offs"]
    panel = a.place_output_u8(e["panel"].shape, skew=po // 4, lead=po % 4, expect=H._t(e["panel"]))
    maps = a.place_output_u8(e["maps"].shape, skew=mo // 4, lead=mo % 4, expect=H._t(e["maps"]), written=c["with_maps"])
    assert panel.address % 16 == po and maps.address % 16 == mo and ws.address % 16 == 8 == conf.address % 16 == r_mh.address % 16
    call = lambda: L.tgsr_attn_panels(r_att.ptr, r_len.ptr, r_img.ptr, int(img.dtype == np.float32), r_mh.ptr, r_mw.ptr, B, T, h, w, u,  # noqa: E731
                                      c["alpha"], K, c["by_conf"], ws.ptr, panel.ptr, maps.ptr if c["with_maps"] else None, conf.ptr, order.ptr,
                                      H._stream(DEV))
    outs = [conf, order, panel] + ([maps] if c["with_maps"] else [])
    got = _twice(a, call, outs)
    for g, name in zip(got, ("conf", "order", "panel", "maps")):
        _same_bits(g, e[name], "%s %s" % (c["name"], name))
    assert np.isfinite(got[0]).all()


def test_refusals():
    """Every NULL among the nine required pointers, every count, K, u and alpha outside its range, the four shapes the kernels do
    not take (tgsr_attn_panels_ws_elems answers 0 for them), every 4- and 8-byte operand off its alignment: TGSR_EINVAL /
    TGSR_EUNSUPPORTED, and no byte of ws, conf, order, panel or maps written."""
    H.run_refusals(DEV)
