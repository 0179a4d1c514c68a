"""CPU: the switch of the register-fed F(4x4) kernels' tile walk (tgsr_wino4w_set_persist) without a GPU - it is an exchange: every
call answers the value it replaces, and 0 (one tile per workgroup), -1 (automatic) and any n > 0 (at most n workgroups) come back as
they went in.  What the walk computes is held on the device by tests/test_hip_wino4w_persist.py."""
import pytest


@pytest.fixture
def L():
    from tgsr_amd import _lib
    lib = _lib.lib()
    was = lib.tgsr_wino4w_set_persist(-1)
    try:
        yield lib
    finally:
        lib.tgsr_wino4w_set_persist(was)


def test_the_switch_is_an_exchange_and_round_trips(L):
    from tgsr_amd import ops
    assert L.tgsr_wino4w_set_persist(0) == -1
    seq = [0, -1, 1, 3, 0, 512, 2 ** 31 - 1, -1]
    for before, after in zip(seq, seq[1:]):
        assert L.tgsr_wino4w_set_persist(after) == before
    assert ops.wino4w_set_persist(7) == -1 and ops.wino4w_set_persist(-1) == 7


def test_the_header_and_the_binding_declare_it(L):
    from tgsr_amd import _lib
    import ctypes
    assert _lib.SIGNATURES["tgsr_wino4w_set_persist"] == (ctypes.c_int, [ctypes.c_int])
    assert L.tgsr_wino4w_set_persist.restype is ctypes.c_int
