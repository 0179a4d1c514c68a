"""GPU: the tile walk of wino4w_conv3x3_kernel (tgsr_wino4w_set_persist) leaves every output bit as it was.

A register-fed F(4x4) launch starts min(tiles, cap) workgroups; workgroup i takes the workgroup tiles i, i + n, ... of the plan, each
through the remap and decomposition the one-tile-per-workgroup grid gives blockIdx.x and from its own prologue to its own epilogue, one
barrier apart from the tile before (whose stores may still be draining while the next prologue's copies land in the same LDS).  Every
tile keeps its arithmetic, so for every cap the output must be torch.equal to cap = 0 of the same build.  The cases are the smallest
shapes at which the walk can go wrong (the tile counts are asserted from the exported planner); the caps are 1 (one workgroup walks
everything), 3 (uneven shares), more than there are tiles, and automatic.  Each call runs twice on one output buffer that was filled with NaN first: a tile never visited keeps its NaN.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_hip_parity import ATOL            # the bound tests/test_hip_parity.py holds the F(4x4) form to against fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAPS = (1, 3, 64, -1)                       # 64 >= the tile count of every case

# name: (GLU, NB, Cin, Cout, B, H, W, tiles, residual, affine)
CASES = {
    "a": (True, 8, 8, 128, 2, 16, 64, 8, False, True),     # two stages; the walk crosses the batch boundary; top / bottom zero rows
    "b": (True, 8, 64, 128, 1, 8, 128, 4, False, True),    # two tile columns: left / right zero columns; sixteen stages
    "c": (False, 4, 16, 64, 2, 16, 64, 8, True, True),     # the residual is read in the epilogue, the next tile's copies follow it
    "d": (False, 4, 8, 64, 1, 24, 64, 6, False, False),    # scale == NULL
    "e": (True, 4, 16, 64, 3, 8, 64, 6, False, True),      # three images of two tile rows each
}
STATS_CASES = {"f8": (8, 8, 128, 2, 16, 64, 8), "f4": (4, 8, 64, 2, 16, 64, 8)}   # NB, Cin, Cout, B, H, W, tiles


@pytest.fixture(scope="module")
def lib():
    from tgsr_amd import _lib
    return _lib.lib()


@pytest.fixture
def persist(lib):
    """Sets the switch for a test and puts back what was there."""
    was = lib.tgsr_wino4w_set_persist(-1)
    try:
        yield lib.tgsr_wino4w_set_persist
    finally:
        lib.tgsr_wino4w_set_persist(was)


def plan_of(lib, x, pack, cout, out, glu, stats):
    from tgsr_amd import _lib as M
    buf = (ctypes.c_int * M.CONV_PLAN_FIELDS)(*([-7] * M.CONV_PLAN_FIELDS))
    B, cin, H, W = x.shape
    rc = lib.tgsr_conv3x3_form_plan(M.CONV_FORMS.index("wino4w"), x.data_ptr(), cin * H * W, B, cin, H, W, pack.data_ptr(), cout, None, None,
                                    None, 0, out.data_ptr(), out.shape[1] * H * W, M.EPI_AFFINE_GLU if glu else M.EPI_AFFINE, 0, int(stats), buf)
    assert rc == M.OK
    return list(buf)


def make(name):
    from tgsr_amd import ops
    glu, nb, cin, cout, B, H, W, tiles, res, affine = CASES[name]
    g = torch.Generator().manual_seed(1000 + ord(name))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    scale = 0.5 + torch.rand(cout, generator=g) if affine else None
    shift = 0.3 * torch.randn(cout, generator=g) if affine else None
    co = cout // 2 if glu else cout
    r = torch.randn(B, co, H, W, generator=g) if res else None
    dev = lambda t: None if t is None else t.to(DEV)
    t = dict(x=x, w=w, scale=scale, shift=shift, r=r, co=co, glu=glu, cout=cout)
    t["dev"] = dict(x=dev(x), up=ops.pack_wino4w_weight(w.to(DEV), glu=glu), scale=dev(scale), shift=dev(shift), r=dev(r))
    return t


def run(t, out):
    from tgsr_amd import ops
    d = t["dev"]
    return ops.conv3x3_wino4(d["x"], d["up"], t["cout"], d["scale"], d["shift"], glu=t["glu"], residual=d["r"], out=out, wide=True)


def twice_on_nan(call, *bufs):
    """call() twice in a row on buffers filled with NaN beforehand; the buffers' contents after each run."""
    for b in bufs:
        b.fill_(float("nan"))
    seen = []
    for _ in range(2):
        call()
        seen.append([b.clone() for b in bufs])
    return seen


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_cap_is_bit_identical_to_one_tile_per_workgroup(lib, persist, name):
    from tgsr_amd import _lib as M
    glu, nb, cin, cout, B, H, W, tiles, res, affine = CASES[name]
    t = make(name)
    out = torch.empty(B, t["co"], H, W, device=DEV)
    plan = plan_of(lib, t["dev"]["x"], t["dev"]["up"], cout, out, glu, 0)
    assert plan[M.CONV_PLAN_T:M.CONV_PLAN_T + 3] == [int(glu), nb, 0] and plan[M.CONV_PLAN_GRID_X] == tiles
    assert t["dev"]["r"] is None or t["dev"]["r"].data_ptr() != out.data_ptr()
    persist(0)
    (ref,), (ref2,) = twice_on_nan(lambda: run(t, out), out)
    assert not torch.isnan(ref).any() and torch.equal(ref, ref2)
    for cap in CAPS:
        assert persist(cap) in (0,) + CAPS
        for (got,) in twice_on_nan(lambda: run(t, out), out):
            assert torch.equal(got, ref), "cap %d: %d of %d values differ" % (cap, int((got != ref).sum()), ref.numel())


@pytest.mark.parametrize("name", sorted(STATS_CASES))
def test_statistics_slots_come_from_the_tile_not_the_workgroup(lib, persist, name):
    from tgsr_amd import _lib as M, ops
    nb, cin, cout, B, H, W, tiles = STATS_CASES[name]
    g = torch.Generator().manual_seed(2000 + nb)
    x = torch.randn(B, cin, H, W, generator=g).to(DEV)
    up = ops.pack_wino4w_weight((torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(DEV))
    out = torch.empty(B, cout, H, W, device=DEV)
    nslots = lib.tgsr_wino4_wide_stats_nslots(B, H, W, cout)
    part = torch.empty(cout, nslots, 2, device=DEV)
    plan = plan_of(lib, x, up, cout, out, False, 1)
    assert plan[M.CONV_PLAN_T:M.CONV_PLAN_T + 3] == [0, nb, 1] and plan[M.CONV_PLAN_GRID_X] == tiles and plan[M.CONV_PLAN_NSLOTS] == nslots

    def call():
        ops.check(lib.tgsr_wino4_wide_conv3x3_stats_fwd(x.data_ptr(), cin * H * W, B, cin, H, W, up.data_ptr(), cout, out.data_ptr(),
                                                        cout * H * W, part.data_ptr(), ops._stream()), "tgsr_wino4_wide_conv3x3_stats_fwd")
    persist(0)
    ref = twice_on_nan(call, out, part)[1]
    assert not torch.isnan(ref[0]).any() and not torch.isnan(ref[1]).any()
    for cap in CAPS:
        persist(cap)
        for got in twice_on_nan(call, out, part):
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), cap


@pytest.mark.parametrize("name", ["a", "c"])
def test_three_workgroups_against_fp64(persist, name):
    """cap = 3 (three workgroups share eight tiles 3 / 3 / 2) against F.conv2d in fp64, within the F(4x4) form's bound."""
    t = make(name)
    x, w, co = t["x"].double(), t["w"].double(), t["co"]
    ref = F.conv2d(x, w, None, 1, 1) * t["scale"].double()[None, :, None, None] + t["shift"].double()[None, :, None, None]
    ref = ref[:, :co] * torch.sigmoid(ref[:, co:]) if t["glu"] else ref
    ref = ref + t["r"].double() if t["r"] is not None else ref
    persist(3)
    out = run(t, None)
    err = float((out.cpu().double() - ref).abs().max())
    assert err < ATOL, err


def test_a_captured_walk_replays_on_changed_inputs(persist):
    """Case b at the automatic cap (the first automatic launch of a process may fall inside a capture: what it asks the device is legal
    there), captured once and replayed three times on changed inputs: each replay equals the eager call on the same input."""
    t = make("b")
    d = t["dev"]
    B, _, H, W = d["x"].shape
    persist(-1)
    static_out = torch.empty(B, t["co"], H, W, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(t, static_out)
    g = torch.Generator().manual_seed(77)
    for _ in range(3):
        d["x"].copy_(torch.randn(d["x"].shape, generator=g))
        static_out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, run(t, None))
