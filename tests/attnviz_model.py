"""The fp64 model of an attention panel (tgsr_amd/attnviz.py states the arithmetic): scipy for the expand and the blur, Pillow for
the blend, numpy for the layout.  Independent of tgsr_amd.attnviz.expand_operator - nothing here builds an operator matrix.
Shared by tests/test_attnviz_host.py, tests/test_hip_attnviz.py and tests/golden/make_attnviz_golden.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attnviz.npz")

# (name, T, n, h, w, u, seed): every case another caption length, so a cap_len-dependent threshold bug shows
CASES = (("reflect", 5, 5, 8, 8, 4, 11),        # blur radius 80 against a 32-pixel tile: multiple reflections
         ("rect", 6, 4, 5, 12, 3, 12),          # rectangular, odd sizes, unaligned stores, cap_len < T
         ("shipped", 18, 18, 32, 32, 8, 13),    # the shipped form
         ("lds", 7, 7, 128, 128, 2, 14),        # the LDS limit
         ("noblur", 9, 9, 16, 16, 1, 15))       # u = 1
GOLDEN_CASES = ("reflect", "rect")


def softmax_maps(T, h, w, seed, B=None):
    """Softmax over the words of seeded 3 N(0, 1) logits: float32 [T, h, w] (or [B, T, h, w])."""
    rng = np.random.RandomState(seed)
    shape = (T, h, w) if B is None else (B, T, h, w)
    z = 3.0 * rng.randn(*shape)
    z = z - z.max(axis=-3, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=-3, keepdims=True)).astype(np.float32)


def image(h, w, seed, B=None):
    """A float32 image around [-1, 1], a little of it outside."""
    rng = np.random.RandomState(seed + 1000)
    shape = (3, h, w) if B is None else (B, 3, h, w)
    return (1.1 * np.tanh(rng.randn(*shape))).astype(np.float32)


def image_bytes(img):
    """utils.py:341-343 in fp32 on torch CPU: add, div, mul, round, clamp."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).clone()
    return t.add(1).div(2).mul(255).round().clamp(0, 255).to(torch.uint8).numpy()


def thresholded(x, n):
    """(fp64 map with everything at or under 2 / n zeroed, conf)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    thresh = 2.0 / float(n)
    conf = float((x64 * (x64 > 2.0 * thresh)).sum())
    return x64 * (x64 > thresh), conf


def expand(X, u):
    """Step 4: the two scipy calls that define it."""
    import scipy.ndimage as ndi
    if u == 1:
        return X
    return ndi.gaussian_filter(ndi.zoom(X, u, order=1, mode='mirror', grid_mode=True), 20, mode='reflect', truncate=4.0)


def stretch(y):
    """Steps 5-7."""
    mn, mx = y.min(), y.max()
    if mx == mn:
        return np.zeros(y.shape, dtype=np.uint8)
    return (((y - mn) / (mx - mn)) * 255.0).astype(np.uint8)


def map_bytes(att, n, u, expand_fn=expand):
    """(uint8 [T, u h, u w] - zero behind word n -, conf float64 [T]) of one image's att [T, h, w]."""
    T, h, w = att.shape
    out = np.zeros((T, u * h, u * w), dtype=np.uint8)
    conf = np.zeros(T, dtype=np.float64)
    for j in range(n):
        X, conf[j] = thresholded(att[j], n)
        out[j] = stretch(expand_fn(X, u))
    return out, conf


def slot_order(conf, n, by_conf):
    """int32 [T]: the word of every slot s < n, -1 behind.  Descending conf, ties to the higher word index."""
    order = np.full(len(conf), -1, dtype=np.int32)
    words = list(range(n))
    if by_conf:
        words.sort(key=lambda j: (-conf[j], -j))
    order[:n] = words
    return order


def paste(map_u8, img_u8, alpha):
    """Pillow's paste of the grey map [V, W] over the image bytes [3, V, W] through a constant mask (utils.py:412-416): [V, W, 3]."""
    from PIL import Image
    V, W = map_u8.shape
    im = Image.fromarray(np.ascontiguousarray(img_u8.transpose(1, 2, 0)))
    at = Image.fromarray(np.ascontiguousarray(np.repeat(map_u8[:, :, None], 3, axis=2)))
    merged = Image.new('RGBA', (W, V), (0, 0, 0, 0))
    mask = Image.new('L', (W, V), int(alpha))
    merged.paste(im, (0, 0))
    merged.paste(at, (0, 0), mask)
    return np.array(merged)[:, :, :3]


def panel(maps_u8, img_u8, order, n, K, alpha):
    """uint8 [Vh, K (Vw + 2), 3] of one image: slot s < min(K, n) shows word order[s]; separators and right padding black."""
    T, Vh, Vw = maps_u8.shape
    out = np.zeros((Vh, K * (Vw + 2), 3), dtype=np.uint8)
    for s in range(min(K, n)):
        out[:, s * (Vw + 2):s * (Vw + 2) + Vw] = paste(maps_u8[int(order[s])], img_u8, alpha)
    return out


def golden():
    return np.load(GOLDEN)
