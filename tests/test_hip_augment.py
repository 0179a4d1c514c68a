"""GPU: the ragged crop / resize / window / flip launch (tgsr_augment_u8) and its coefficient step (tgsr_resize_coeffs)
against Pillow's own output (tests/golden/io_augment.npz) and the numpy restatement of Pillow's arithmetic - integer
equality everywhere, no tolerance.  No Pillow import: the GPU machine need not have it."""
import numpy as np
import pytest
import torch

from conftest import load_npz
from oracle import tgsr_oracle_io as IO

pytestmark = pytest.mark.gpu
DEV = "cuda"

# awkward sizes for the coefficient tables, every ordered pair up to the 16x cap: 1-tap corners, both sides of powers of two,
# the training sizes (32/38, 64/76, 256/304) and the photograph sizes around them, the 4096 limit
COEF_SIZES = [1, 2, 3, 7, 15, 31, 32, 33, 37, 38, 63, 64, 76, 255, 256, 257, 303, 304, 305, 333, 375, 405, 500, 640, 1201,
              1999, 4096]


@pytest.fixture(scope="module")
def gold():
    return load_npz("io_augment.npz")


def _batch(z, name, order=None):
    """The fixture's sources of one table packed in `order`, with the offsets rewritten for that order."""
    from tgsr_amd.datasets import RaggedImages
    table, src = z[name + "_table"], z[name + "_src"]
    order = list(range(len(table))) if order is None else order
    batch = RaggedImages.pack([z["src%d" % src[i]] for i in order], device=DEV)
    t = torch.from_numpy(table[order].copy())
    t[:, 0] = torch.tensor(batch.offsets, dtype=torch.int32)
    return batch, t


def _oracle(src, d, S):
    _off, _H, _W, x1, y1, x2, y2, oh, ow, top, left, flip = d
    crop = np.ascontiguousarray(src[y1:y2, x1:x2].transpose(2, 0, 1))
    r = IO.resize_bilinear(crop, oh, ow)[..., top:top + S, left:left + S]
    return r[..., ::-1] if flip else r


def test_device_coefficients_equal_the_host_tables_exactly():
    from tgsr_amd import ops
    n = 0
    for a in COEF_SIZES:
        for b in COEF_SIZES:
            if a > 16 * b:
                continue
            bounds, taps = ops.resize_coeffs_device(a, b)
            rb, rk = IO.resize_coeffs(a, b)
            assert np.array_equal(bounds.cpu().numpy(), rb), "bounds %d -> %d" % (a, b)
            assert np.array_equal(taps.cpu().numpy(), rk), "taps %d -> %d" % (a, b)
            n += 1
    assert n > 600


def test_fixture_batch_is_byte_identical_to_pillow(gold):
    from tgsr_amd import ops
    S = int(gold["S"])
    batch, table = _batch(gold, "train")                      # nine descriptors over seven different sizes in one launch
    assert np.array_equal(table.numpy(), gold["train_table"])
    got = ops.augment_u8(batch.data, table, S)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(table), 3, S, S)
    for i, g in enumerate(got.cpu().numpy()):
        assert np.array_equal(g, gold["train_out"][i]), "descriptor %d %s" % (i, table[i].tolist())
    order = list(range(len(table)))[::-1]
    batch, table = _batch(gold, "train", order)               # other offsets, same images
    got = ops.augment_u8(batch.data, table, S).cpu().numpy()
    for k, i in enumerate(order):
        assert np.array_equal(got[k], gold["train_out"][i]), "reversed: descriptor %d" % i


def test_eval_mode_is_byte_identical_to_pillow(gold):
    from tgsr_amd.datasets import DeviceAugment, RaggedImages
    aug = DeviceAugment(int(gold["S"]), ratio=72 / 64, mode="eval", device=DEV)
    batch = RaggedImages.pack([gold["src%d" % i] for i in gold["eval_src"]], device=DEV)
    plan = aug.plan(batch, [None, tuple(int(v) for v in gold["bbox6"])])
    assert np.array_equal(plan.numpy(), gold["eval_table"])
    assert np.array_equal(aug(batch, plan).cpu().numpy(), gold["eval_out"])


@pytest.fixture(scope="module")
def ragged_case():
    """B = 5 at S = 64 / Resize(76), random bytes: 640 x 37 (a 17x up-scale of the short side, 1314 resized rows); 76 x 100
    (oh == H: both passes skipped); 1216 x 1296 (exactly 16x down on both axes: 33 taps, and the LDS intermediate of a tile at
    its tallest, 145 source rows); two photographs' sizes with CUB-style boxes.  Reference computed once."""
    from tgsr_amd.datasets import DeviceAugment, RaggedImages
    g = np.random.default_rng(17)
    shapes = [(640, 37), (76, 100), (1216, 1296), (375, 500), (97, 80)]
    bboxes = [None, None, None, (120, 60, 210, 190), (5, 10, 60, 70)]
    srcs = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    aug = DeviceAugment(64, device=DEV)
    plan = aug.plan(shapes, bboxes, generator=torch.Generator().manual_seed(23))
    assert plan[1, 7:9].tolist() == [76, 100] and plan[2, 7:9].tolist() == [76, 81] and plan[0, 7:9].tolist() == [1314, 76]
    want = np.stack([_oracle(s, d, 64) for s, d in zip(srcs, plan.tolist())])
    return aug, RaggedImages.pack(srcs, device=DEV), plan, want


def test_one_launch_equals_the_unfused_composition(ragged_case):
    aug, batch, plan, want = ragged_case
    got = aug(batch, plan).cpu().numpy()
    for i in range(len(plan)):
        assert np.array_equal(got[i], want[i]), "image %d %s" % (i, plan[i].tolist())
    # the other flip and the far window of every image
    other = plan.clone()
    other[:, 11] = 1 - other[:, 11]
    other[:, 9], other[:, 10] = other[:, 7] - 64, other[:, 8] - 64
    got = aug(batch, other).cpu().numpy()
    srcs = [batch.data[o:o + 3 * h * w].view(h, w, 3).cpu().numpy() for (h, w), o in zip(batch.sizes, batch.offsets)]
    for i, d in enumerate(other.tolist()):
        assert np.array_equal(got[i], _oracle(srcs[i], d, 64)), "image %d %s" % (i, d)


@pytest.mark.parametrize("S", [5, 70])
def test_window_sizes_that_are_no_multiple_of_the_tile(S):
    """A workgroup owns 8 rows x 64 columns: S = 70 leaves a 6-row and a 6-column remainder, S = 5 is one partial tile.
    Descriptors set by hand: up on one axis and down on the other, a box inside the image, both flips."""
    from tgsr_amd import ops
    from tgsr_amd.datasets import RaggedImages
    g = np.random.default_rng(S)
    srcs = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((90, 100), (200, 71), (75, 333))]
    batch = RaggedImages.pack(srcs, device=DEV)
    rows = [(90, 100, 0, 0, 100, 90, 75, 140, 75 - S, 33, 1), (200, 71, 3, 10, 70, 187, max(S, 12), 90, 0, 90 - S, 0),
            (75, 333, 11, 0, 333, 75, 151, max(2 * S, 24), 40, S, 1)]
    table = torch.tensor([(o,) + r for o, r in zip(batch.offsets, rows)], dtype=torch.int32)
    got = ops.augment_u8(batch.data, table, S).cpu().numpy()
    for i, d in enumerate(table.tolist()):
        assert np.array_equal(got[i], _oracle(srcs[i], d, S)), "image %d %s" % (i, d)


def test_nothing_is_written_outside_the_output(ragged_case):
    from tgsr_amd import ops
    _aug, batch, plan, want = ragged_case
    n, pad = want.size, 4096
    buf = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[pad:pad + n].view(want.shape)
    assert ops.augment_u8(batch.data, plan, 64, out=out) is out
    host = buf.cpu().numpy()
    assert np.all(host[:pad] == 0xA5) and np.all(host[pad + n:] == 0xA5)
    assert np.array_equal(host[pad:pad + n].reshape(want.shape), want)


def test_side_stream_beside_a_busy_default_stream(ragged_case):
    aug, batch, plan, want = ragged_case
    torch.cuda.synchronize()
    busy = torch.ones(32 << 20, device=DEV)
    side = torch.cuda.Stream()
    for _ in range(40):
        busy.mul_(1.0001).add_(1.0)                       # the default stream has work queued while the side stream launches
    with torch.cuda.stream(side):
        got = aug(batch, plan)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    torch.cuda.synchronize()


def test_batcher_equals_the_pyramid_of_the_pillow_crops(gold):
    from tgsr_amd.datasets import GpuImagePyramid, SRBatcher
    S = int(gold["S_e2e"])
    batch, table = _batch(gold, "e2e")
    assert np.array_equal(table.numpy(), gold["e2e_table"])
    batcher = SRBatcher((32, S), device=DEV)
    crops = torch.from_numpy(gold["e2e_out"]).to(DEV)
    assert torch.equal(batcher.augment(batch, table), crops)
    got = batcher(batch, plan=table, u8=True)
    want = GpuImagePyramid((32, S), device=DEV)(crops, u8=True)
    for name, gl, wl in zip(("imgs", "bic", "imgsblur", "bicblur"), got, want):
        assert len(gl) == 2
        for i, (a, b) in enumerate(zip(gl, wl)):
            assert a.dtype == torch.uint8 and torch.equal(a, b), "%s[%d]" % (name, i)
    fl = batcher(batch, plan=table)
    for lst in fl:
        for t, s in zip(lst, (32, S)):
            assert t.dtype == torch.float32 and tuple(t.shape) == (len(table), 3, s, s)
    # the planned form: train-mode draws from a seeded generator give a valid batch of the same layout
    drawn = batcher(batch, bboxes=[None, None, None, tuple(int(v) for v in gold["bbox6"])],
                    generator=torch.Generator().manual_seed(3), u8=True)
    assert tuple(drawn[0][1].shape) == (len(table), 3, S, S)


def test_c_entry_repeats_the_descriptor_checks(gold):
    from tgsr_amd import _lib, ops
    batch, table = _batch(gold, "eval")
    S, L = int(gold["S"]), _lib.lib()
    tdev = table.to(DEV)
    ws = torch.empty(L.tgsr_augment_ws_elems(len(table), S), dtype=torch.int32, device=DEV)
    out = torch.empty(len(table), 3, S, S, dtype=torch.uint8, device=DEV)

    def call(t, nbytes=batch.nbytes):
        return L.tgsr_augment_u8(ops._p(batch.data), nbytes, ops._p(t), ops._p(tdev), len(t), S, ops._p(ws), ops._p(out), ops._stream())
    assert call(table) == _lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), gold["eval_out"])
    assert call(table, batch.nbytes - 1) == _lib.EINVAL                      # the last image would end outside the buffer
    for col, val in ((5, 501), (9, 5), (10, -1), (7, 31), (1, 4097), (11, 2), (5, 240)):
        bad = table.clone()
        bad[1, col] = val
        assert call(bad) == _lib.EINVAL, (col, val)
    assert L.tgsr_resize_coeffs(33, 2, 35, ops._p(ws), ops._p(ws), ops._stream()) == _lib.EINVAL       # above 16x
    assert L.tgsr_resize_coeffs(8, 4, 3, ops._p(ws), ops._p(ws), ops._stream()) == _lib.EINVAL         # ksize is 5
