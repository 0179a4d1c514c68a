"""GPU: the ragged-batch augment launch and its coefficient step (tgsr_amd/csrc/tgsr_augment.hip) held to their C ABI contract,
called directly through ctypes.

    tgsr_resize_coeffs   tgsr_augment_ws_elems   tgsr_augment_u8

tests/test_hip_augment.py reaches them through ops.* on allocator memory: large, 256-byte aligned, table_dev derived from table_host.
Here every device operand of a call - the packed bytes, the device table, the int32 workspace of exactly tgsr_augment_ws_elems words,
the output - lies in ONE guarded arena (tests/arena.py); table_host is a host array, as include/tgsr_hip.h says.  After every accepted
call: the arena's check (guard bands, the bytes in front of and behind a byte operand, every input bit-unchanged, everything the call
owns written, nothing else), a second call from the re-armed state with the workspace holding a finite constant in every word gives the
same bits, and the bytes are the numpy model's (tests/test_augment_abi_host.py: augment_model, oracle.tgsr_oracle_io.resize_coeffs),
BIT-EXACT.  The arena's pattern read as an int32 tap is 2 143 659 429: a workspace word read before it is written shows in every byte
it touches.

The tables, the cases, the models, the wrong kernels each row is there to catch and the refusals live in the host file, which checks
them without a GPU; this file runs them.  It imports neither Pillow nor scipy.
"""
import numpy as np
import pytest
import torch

import test_augment_abi_host as H
from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    diff = got != ref
    assert not diff.any(), "%s: %d of %d elements differ from the model, first at %s: %r, not %r" % (
        what, int(diff.sum()), diff.size, tuple(int(i) for i in np.argwhere(diff)[0]), got[diff][0], ref[diff][0])


def _twice(a, call, outs):
    """The call, the arena's contract, the call again from the re-armed state with every workspace word holding 1.5f's bits: the
    contract again and the same bits in every output."""
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


@pytest.mark.parametrize("row", H.rows(H.COEFF_TABLE), ids=H.row_id)
def test_resize_coeffs(row):
    c = row[3]
    _, L = H._lib()
    rb, rk = H.coeffs(c["i"], c["o"])
    ks = H.ksize(c["i"], c["o"])
    a = Arena(DEV)
    if c["dirty"]:
        g = np.random.default_rng(5)
        bounds = a.place_inout(H._t(g.integers(-9, 9, rb.shape).astype(np.int32)), skew=c["skew"])
        taps = a.place_inout(H._t(g.integers(1, 1 << 22, rk.shape).astype(np.int32)), skew=c["skew"])
    else:
        bounds = a.place_output(rb.shape, dtype=torch.int32, skew=c["skew"])
        taps = a.place_output(rk.shape, dtype=torch.int32, skew=(c["skew"] + 1) % 4)
    got = _twice(a, lambda: L.tgsr_resize_coeffs(c["i"], c["o"], ks, bounds.ptr, taps.ptr, H._stream(DEV)), [bounds, taps])
    _same_bits(got[0], rb, c["name"] + " bounds")
    _same_bits(got[1], rk, c["name"] + " taps")


@pytest.mark.parametrize("row", H.rows(H.AUG_TABLE), ids=H.row_id)
def test_augment_u8(row):
    c = row[3]
    _, L = H._lib()
    packed, table = H.aug_inputs(c)
    B, S = len(table), c["S"]
    ref = H.expected(c["name"])
    a = Arena(DEV)
    pk = a.place_input_u8(H._t(packed), lead=c["leads"][0])
    td = a.place_input(H._t(H.dev_table(c, table)))
    n = L.tgsr_augment_ws_elems(B, S)
    assert n == B * 2 * H.WS_ROW * S
    ws = a.place_ws(n, skew=1)
    if c["bad"]:                                                   # over random bytes: the skipped image keeps them
        prior = np.random.default_rng(3).integers(0, 256, ref.shape, dtype=np.uint8)
        may = np.ones(ref.shape, bool)
        may[c["bad"][0]] = False
        ref = np.where(may, ref, prior)
        out = a.place_inout_u8(H._t(prior), lead=c["leads"][1], may=H._t(may), expect=H._t(ref))
    else:
        out = a.place_output_u8(ref.shape, lead=c["leads"][1], expect=H._t(ref))
    assert pk.address % 4 == c["leads"][0] and out.address % 4 == c["leads"][1] and ws.address % 16 == 4
    host = np.ascontiguousarray(table)
    got = _twice(a, lambda: L.tgsr_augment_u8(pk.ptr, packed.size, H._hp(host), td.ptr, B, S, ws.ptr, out.ptr, H._stream(DEV)), [out])[0]
    for b in range(B):
        _same_bits(got[b], ref[b], "%s image %d %s" % (c["name"], b, table[b].tolist()))
    assert np.array_equal(host, table)


def test_refusals():
    """Every NULL, every count and size outside its range, one bad value for each descriptor field, a buffer one byte short, the int32
    operands off 4 bytes: TGSR_EINVAL / TGSR_EUNSUPPORTED, no byte written - ws and out among what must stay untouched."""
    H.run_refusals(DEV)
