"""CPU: the geometric self-ensemble's transform (tgsr_amd.tiles.d8_*) against numpy's own transpose and flips, the numpy model's
exactness on a constant ensemble, and the refusals of ops.d8_gather / ops.d8_merge that need no device."""
import numpy as np
import pytest
import torch

import ensemble_model as E
from tgsr_amd import tiles as T

SHAPES = [(5, 5), (3, 7), (8, 2)]


def test_the_eight_maps_are_distinct_and_follow_the_shape_rule():
    for th, tw in SHAPES:
        win = np.arange(th * tw, dtype=np.int64).reshape(th, tw)
        seen = []
        for k in range(8):
            hh, ww = T.d8_shape(k, th, tw)
            assert (hh, ww) == ((tw, th) if k & 4 else (th, tw))
            y, x = T.d8_index(k, th, tw)
            assert tuple(y.shape) == (hh, ww) == tuple(x.shape)
            v = win[y.numpy(), x.numpy()]
            assert np.array_equal(v, E.variant(win, k)), "variant %d of %d x %d" % (k, th, tw)      # numpy's transpose and flips
            assert np.array_equal(T.d8_apply(win, k), v) and torch.equal(T.d8_apply(torch.from_numpy(win), k), torch.from_numpy(v))
            assert sorted(v.ravel().tolist()) == list(range(th * tw))                               # a permutation of the pixels
            seen.append((v.shape, v.tobytes()))
        assert len(set(seen)) == 8
    with pytest.raises(ValueError, match="0..7"):
        T.d8_shape(8, 4, 4)


def test_each_map_composed_with_its_inverse_is_the_identity():
    g = np.random.default_rng(1)
    for th, tw in SHAPES:
        win = g.standard_normal((2, 3, th, tw)).astype(np.float32)
        for k in range(8):
            v = T.d8_apply(win, k)
            assert np.array_equal(T.d8_invert(v, k), win) and np.array_equal(E.back(E.variant(win, k), k), win)
            assert np.array_equal(E.back(v, k), win)
            t = torch.from_numpy(win)
            assert torch.equal(T.d8_invert(T.d8_apply(t, k), k), t)


def _model_round_trip(img, H, W, th, tw, halo, out):
    table = T.plan_tiles(H, W, (th, tw), halo).numpy()
    if th == tw:
        a = E.gather(img, table, th, tw)
        assert a.shape == (img.shape[0], len(table), 8, 3, th, tw)
        return E.merge(a.reshape((-1,) + a.shape[3:]), None, table, th, tw, out)
    a, b = E.gather(img, table, th, tw, 0, 4), E.gather(img, table, th, tw, 4, 4)
    assert a.shape[2:] == (4, 3, th, tw) and b.shape[2:] == (4, 3, tw, th)
    return E.merge(a.reshape((-1,) + a.shape[3:]), b.reshape((-1,) + b.shape[3:]), table, th, tw, out)


def test_the_models_merge_of_its_gather_returns_the_image_bit_for_bit():
    """Eight equal float32 values v summed in order and scaled by 0.125 give v exactly when every partial sum 2v .. 8v is a
    float32, i.e. when v has at most 21 significant bits (3 bits of head room for the factor 8; a v of 24 significant bits can lose
    its last bit in 3v): the images are multiples of 2^-10 in [-2, 2).  Square windows (one group of eight) and rectangular ones
    (the two groups of four); the uint8 output is to_uint8 of that mean."""
    g = np.random.default_rng(2)
    for (H, W, th, tw, halo) in ((13, 21, 8, 8, 2), (9, 14, 5, 7, 1)):
        img = (g.integers(-2048, 2048, (2, 3, H, W)) / 1024.0).astype(np.float32)
        out = _model_round_trip(img, H, W, th, tw, halo, np.full((2, 3, H, W), np.nan, np.float32))
        assert np.array_equal(out.view(np.uint32), img.view(np.uint32))
        o8 = _model_round_trip(img, H, W, th, tw, halo, np.zeros((2, 3, H, W), np.uint8))
        assert np.array_equal(o8, E.to_uint8(img))
        b8 = g.integers(0, 256, (2, 3, H, W), dtype=np.uint8)                # bytes in: normalised first, then the same mean
        out = _model_round_trip(b8, H, W, th, tw, halo, np.full((2, 3, H, W), np.nan, np.float32))
        assert np.max(np.abs(out - E.normalize_u8(b8))) <= 2.0 ** -21        # five rounded sums below 8 (half an ulp: 2^-22 at most), times 0.125


def test_refusals_of_the_ops_that_need_no_device():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    H, W, th = 13, 21, 8
    table = T.plan_tiles(H, W, th, 2)
    img = torch.zeros(2, 3, H, W)
    with pytest.raises(TgsrError, match=r"\[N, 3, H, W\]"):
        ops.d8_gather(img[0], table, th, th)
    with pytest.raises(TgsrError, match="uint8 or float32"):
        ops.d8_gather(img.double(), table, th, th)
    with pytest.raises(TgsrError, match="img2 is"):
        ops.d8_gather(img, table, th, th, img2=img.to(torch.uint8))
    for k0, nk in ((4, 8), (2, 4), (0, 2), (0, 0)):
        with pytest.raises(TgsrError, match="groups are"):
            ops.d8_gather(img, table, th, th, k0, nk)
    with pytest.raises(TgsrError, match="square window"):
        ops.d8_gather(img, T.plan_tiles(H, W, (8, 12), 2), 8, 12)
    with pytest.raises(TgsrError, match=r"int32 \[Tb, 6\]"):
        ops.d8_gather(img, table[:, :5].contiguous(), th, th)
    with pytest.raises(TgsrError, match="1 <= window"):
        ops.d8_gather(img, table, H + 1, H + 1)
    with pytest.raises(TgsrError, match="HIP tensors"):
        ops.d8_gather(img, table, th, th)
    src = torch.zeros(2 * len(table) * 8, 3, 2 * th, 2 * th)
    out = torch.zeros(2, 3, 2 * H, 2 * W)
    with pytest.raises(TgsrError, match="per launch"):
        ops.d8_merge([], [], table, H, W, th, th)
    with pytest.raises(TgsrError, match="per launch"):
        ops.d8_merge([src] * 13, [out] * 13, table, H, W, th, th)
    with pytest.raises(TgsrError, match="transposed group of EVERY output"):
        ops.d8_merge([src, src], [out, out], table, H, W, th, th, srcs_t=[src, None])
    with pytest.raises(TgsrError, match="square window"):
        ops.d8_merge([src], [out], T.plan_tiles(H, W, (8, 12), 2), H, W, 8, 12)
    with pytest.raises(TgsrError, match=r"int32 \[Tb, 6\]"):
        ops.d8_merge([src], [out], table.long(), H, W, th, th)
    with pytest.raises(TgsrError, match="HIP tensors"):
        ops.d8_merge([src], [out], table, H, W, th, th)
