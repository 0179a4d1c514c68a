"""CPU: the host side of the ragged crop / resize / window / flip path (datasets.crop_box, resized_size, RaggedImages,
DeviceAugment.plan, ops.check_augment_table) - integer for integer against the fixture made with Pillow
(tests/golden/make_augment_golden.py), and every refusal raised before a device is touched."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_npz
from tgsr_amd import _lib, ops
from tgsr_amd._lib import TgsrError
from tgsr_amd.datasets import DeviceAugment, RaggedImages, SRBatcher, crop_box, resized_size


@pytest.fixture(scope="module")
def gold():
    return load_npz("io_augment.npz")


def _sources(z, name):
    return [z["src%d" % i] for i in z[name + "_src"]]


def test_crop_box_and_resized_size_equal_the_fixture(gold):
    for case, want in zip(gold["box_cases"], gold["box_expected"]):
        assert crop_box(tuple(case[:4]), int(case[4]), int(case[5])) == tuple(int(v) for v in want), case
    ints = crop_box(tuple(int(v) for v in gold["bbox6"]), 500, 45)
    assert ints == (240, 0, 500, 45) and all(type(v) is int for v in ints)
    for (w, h, size), want in zip(gold["resize_cases"].tolist(), gold["resize_expected"].tolist()):
        assert resized_size(w, h, size) == tuple(want), (w, h, size)
    assert resized_size(500, 375, 304) == (405, 304) and resized_size(375, 500, 304) == (304, 405)


def test_crop_box_and_resized_size_equal_pil(gold):
    Image = pytest.importorskip("PIL.Image")
    src = gold["src6"]
    box = crop_box(tuple(int(v) for v in gold["bbox6"]), src.shape[1], src.shape[0])
    img = Image.fromarray(src).crop(box)
    assert img.size == (box[2] - box[0], box[3] - box[1])
    ow, oh = resized_size(img.size[0], img.size[1], 38)
    d = gold["train_table"][6].tolist()
    assert (oh, ow) == (d[7], d[8]) and tuple(d[3:7]) == box
    got = np.asarray(img.resize((ow, oh), Image.BILINEAR).crop((d[10], d[9], d[10] + 32, d[9] + 32)).transpose(Image.FLIP_LEFT_RIGHT))
    assert np.array_equal(got.transpose(2, 0, 1), gold["train_out"][6])


def test_train_plan_windows_lie_inside_and_reach_both_ends():
    aug = DeviceAugment(64, mode="train")
    rng = np.random.default_rng(5)
    sizes = [(int(h), int(w)) for h, w in rng.integers(64, 700, (200, 2))]
    plan = aug.plan(sizes, generator=torch.Generator().manual_seed(11))
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (200, ops.AUG_DESC) and not plan.is_cuda
    off, H, W, x1, y1, x2, y2, oh, ow, top, left, flip = plan.to(torch.int64).unbind(1)
    assert [(int(h), int(w)) for h, w in zip(H, W)] == sizes
    assert torch.equal(off, torch.cumsum(3 * H * W, 0) - 3 * H * W)
    assert bool(((x1 == 0) & (y1 == 0) & (x2 == W) & (y2 == H)).all())
    for i, (h, w) in enumerate(sizes):
        assert (int(ow[i]), int(oh[i])) == resized_size(w, h, 76)
    assert bool(((top >= 0) & (top + 64 <= oh) & (left >= 0) & (left + 64 <= ow)).all())
    assert bool((top == 0).any()) and bool((top == oh - 64).any())
    assert bool((left == 0).any()) and bool((left == ow - 64).any())
    assert bool((flip == 0).any()) and bool((flip == 1).any()) and bool(((flip == 0) | (flip == 1)).all())
    again = aug.plan(sizes, generator=torch.Generator().manual_seed(11))
    other = aug.plan(sizes, generator=torch.Generator().manual_seed(12))
    assert torch.equal(plan, again) and not torch.equal(plan, other)


def test_eval_plan_is_the_centre_crop(gold):
    srcs = _sources(gold, "eval")
    sizes = [a.shape[:2] for a in srcs]
    plan = DeviceAugment(32, ratio=72 / 64, mode="eval").plan(sizes, [None, tuple(int(v) for v in gold["bbox6"])])
    assert np.array_equal(plan.numpy(), gold["eval_table"])
    bare = DeviceAugment(32, ratio=1, mode="eval").plan([(40, 33), (32, 90)])
    assert bare[:, 7:].tolist() == [[40, 33, 4, 0, 0], [32, 90, 0, 29, 0]]       # oh ow top left flip: no Resize; round(0.5) = 0
    for oh, S in ((37, 32), (38, 32), (39, 32), (41, 32)):
        p = DeviceAugment(S, ratio=1, mode="eval").plan([(oh, 32)])
        assert int(p[0, 9]) == int(round((oh - S) / 2.))


def test_train_plan_reproduces_the_fixture_descriptors_apart_from_the_draws(gold):
    srcs = [gold["src%d" % i] for i in range(7)]
    boxes = [None] * 6 + [tuple(int(v) for v in gold["bbox6"])]
    plan = DeviceAugment(32, mode="train").plan(RaggedImages.pack(srcs, device=None, pin=False), boxes,
                                                generator=torch.Generator().manual_seed(0))
    assert np.array_equal(plan[:, :9].numpy(), gold["train_table"][:7, :9])


def test_pack_round_trips_offsets_and_sizes(gold):
    srcs = [gold["src%d" % i] for i in range(7)]
    mixed = [torch.from_numpy(a) if i % 2 else a for i, a in enumerate(srcs)]
    mixed[2] = np.asfortranarray(srcs[2])                                        # any memory order
    batch = RaggedImages.pack(mixed, device=None, pin=False)
    assert len(batch) == 7 and batch.sizes == [a.shape[:2] for a in srcs]
    assert batch.offsets == gold["train_table"][:7, 0].tolist()
    assert batch.data.dtype == torch.uint8 and batch.data.dim() == 1 and batch.nbytes == sum(a.size for a in srcs)
    for a, (h, w), o in zip(srcs, batch.sizes, batch.offsets):
        assert np.array_equal(batch.data[o:o + 3 * h * w].view(h, w, 3).numpy(), a)


@pytest.mark.parametrize("bad", [np.zeros((4, 5, 3), np.float32), np.zeros((3, 4, 5), np.uint8), np.zeros((4, 5), np.uint8),
                                 torch.zeros(4, 5, 3, dtype=torch.int16), np.zeros((0, 5, 3), np.uint8), [[1, 2, 3]]])
def test_pack_refuses_other_dtypes_and_layouts(bad):
    with pytest.raises(TgsrError, match="image 1 is not an H x W x 3 uint8"):
        RaggedImages.pack([np.zeros((4, 5, 3), np.uint8), bad], device=None, pin=False)


def test_pack_refuses_an_empty_batch():
    with pytest.raises(TgsrError, match="empty batch"):
        RaggedImages.pack([], device=None)


def test_plan_refusals():
    train = DeviceAugment(32, mode="train")
    with pytest.raises(TgsrError, match="empty crop box"):
        train.plan([(8, 8)], [(3, 2, 1, 1)])                                     # r = int(0.75) = 0
    with pytest.raises(TgsrError, match="smaller than the 32 window"):
        DeviceAugment(32, ratio=1, mode="eval").plan([(40, 31)])                 # torchvision would pad
    with pytest.raises(TgsrError, match=r"source side outside \[1, 4096\]"):
        train.plan([(64, 4097)])
    with pytest.raises(TgsrError, match="reduction above 16x"):
        train.plan([(700, 700)])                                                 # 700 -> 38
    with pytest.raises(TgsrError, match="1 bounding boxes for 2 images"):
        train.plan([(64, 64), (64, 64)], [None])
    with pytest.raises(TgsrError, match="mode"):
        DeviceAugment(32, mode="test")
    with pytest.raises(TgsrError, match="cannot hold"):
        DeviceAugment(32, ratio=0.5)
    assert train.plan([(608, 608)]).shape == (1, ops.AUG_DESC)                   # exactly 16x is inside


def _row(**kw):
    d = dict(off=0, H=40, W=50, x1=0, y1=0, x2=50, y2=40, oh=38, ow=47, top=3, left=7, flip=0)
    d.update(kw)
    return torch.tensor([list(d.values())], dtype=torch.int32)


@pytest.mark.parametrize("kw,what", [
    (dict(x2=0), "empty crop box"), (dict(x1=20, x2=20), "empty crop box"), (dict(y2=41), "empty crop box or one outside"),
    (dict(x1=-1), "outside its image"), (dict(oh=31, top=0), "smaller than the window"), (dict(ow=31, left=0), "smaller than the window"),
    (dict(top=7), "window outside"), (dict(left=16), "window outside"), (dict(top=-1), "window outside"),
    (dict(off=1), "outside the packed buffer"), (dict(off=-1), "outside the packed buffer"), (dict(H=41, y2=40), "outside the packed buffer"),
    (dict(W=4097, x2=50), "source side outside"), (dict(H=0), "source side outside"), (dict(flip=2), "flip flag"),
    (dict(H=1000, W=6, x2=6, y2=1000, oh=62, ow=32, left=0), "reduction above 16x"), (dict(oh=65537), "resized side above")])
def test_table_check_refuses(kw, what):
    nbytes = 18000 if kw.get("H") == 1000 else 6000
    with pytest.raises(TgsrError, match=what):
        ops.check_augment_table(_row(**kw), 32, nbytes)


def test_table_check_accepts_and_refuses_by_form():
    t = ops.check_augment_table(_row(), 32, 6000)
    assert t.dtype == torch.int32 and t.is_contiguous()
    for bad in (_row().to(torch.int64), _row()[0], _row()[:, :11], _row()[:0]):
        with pytest.raises(TgsrError, match="descriptor table"):
            ops.check_augment_table(bad, 32, 6000)
    with pytest.raises(TgsrError, match="window size"):
        ops.check_augment_table(_row(), 0, 6000)
    with pytest.raises(TgsrError, match="packed buffer"):
        ops.check_augment_table(_row(), 32, 2 ** 31)
    # the op itself refuses before it looks for a device: a bad table first, then a host buffer
    with pytest.raises(TgsrError, match="window outside"):
        ops.augment_u8(torch.zeros(6000, dtype=torch.uint8), _row(top=7), 32)
    with pytest.raises(TgsrError, match="flat uint8"):
        ops.augment_u8(torch.zeros(6000, dtype=torch.float32), _row(), 32)
    with pytest.raises(TgsrError, match="no CPU fallback"):
        ops.augment_u8(torch.zeros(6000, dtype=torch.uint8), _row(), 32)


def test_resize_coeffs_device_refuses_on_the_host():
    assert [ops.resize_ksize(a, b) for a, b in ((5, 5), (5, 50), (500, 405), (32, 2), (33, 2), (4096, 256))] == [3, 3, 5, 33, 35, 33]
    with pytest.raises(TgsrError, match="reduction above 16x"):
        ops.resize_coeffs_device(33, 2)
    with pytest.raises(TgsrError, match="sizes must lie"):
        ops.resize_coeffs_device(0, 2)
    with pytest.raises(TgsrError, match="HIP device"):
        ops.resize_coeffs_device(8, 4, device="cpu")


def test_batcher_is_augment_then_pyramid():
    b = SRBatcher((32, 64), mode="eval", ratio=72 / 64)
    assert b.augment.imsize == 64 and b.augment.size == 72 and b.augment.mode == "eval" and b.pyramid.sizes == (32, 64)


def test_new_entries_are_in_the_header_and_the_binding():
    src = open(os.path.join(ROOT, "include", "tgsr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("tgsr_augment_u8", "tgsr_resize_coeffs", "tgsr_augment_ws_elems"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["tgsr_augment_u8"][1]) == 9 and len(_lib.SIGNATURES["tgsr_resize_coeffs"][1]) == 6
