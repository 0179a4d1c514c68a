"""Numpy model of the geometric self-ensemble (tgsr_ensemble.hip; the transform of tgsr_amd/tiles.py): the variant gather, the
merge with the fixed float32 summation order, `to_uint8` of the mean, and the shared oracle cases of the ensemble tests.
TEST INFRASTRUCTURE: pure numpy / the CPU oracle, imports nothing of the HIP library and not tgsr_amd.tiles' index maps - the
variants are built from numpy's own transpose and flips, which the host tests compare the maps against."""
import functools

import numpy as np
import torch

from tiles_model import normalize_u8, to_uint8

SCALES = {"fine": (2, 4, 8), "fake": (2, 4, 8), "att": (1, 2, 4)}


def variant(win, k):
    """Variant k of win [..., h, w]: transpose first (k & 4), then mirror the rows (k & 2) and the columns (k & 1)."""
    v = np.swapaxes(win, -1, -2) if k & 4 else win
    if k & 2:
        v = v[..., ::-1, :]
    if k & 1:
        v = v[..., ::-1]
    return np.ascontiguousarray(v)


def back(var, k):
    """The window whose variant k is `var`: the mirrors undone, then the transpose."""
    v = var
    if k & 1:
        v = v[..., ::-1]
    if k & 2:
        v = v[..., ::-1, :]
    return np.ascontiguousarray(np.swapaxes(v, -1, -2) if k & 4 else v)


def gather(imgs, table, th, tw, k0=0, nk=8):
    """[N, Tb, nk, 3, th', tw'] float32: variants k0 .. k0 + nk - 1 of every window of imgs [N, 3, H, W] (uint8: normalised;
    float32: copied).  One group has one shape: (0, 8) needs th == tw."""
    f = normalize_u8(imgs) if imgs.dtype == np.uint8 else imgs.astype(np.float32, copy=True)
    return np.stack([np.stack([np.stack([variant(f[n][:, y0:y0 + th, x0:x0 + tw], k) for k in range(k0, k0 + nk)])
                               for y0, x0 in np.asarray(table)[:, :2]]) for n in range(f.shape[0])])


def mean8(vs):
    """((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125 in float32, one rounding per operation."""
    assert len(vs) == 8 and all(v.dtype == np.float32 for v in vs)
    acc = vs[0]
    for v in vs[1:]:
        acc = (acc + v).astype(np.float32)
    return (acc * np.float32(0.125)).astype(np.float32)


def merge(src_a, src_b, table, th, tw, out):
    """Every window's owned rectangle of the mean of its eight variant outputs, each mapped back, into out [N, C, s H, s W] (in
    place; uint8 out: to_uint8 of the float32 mean).  src_a: [N * Tb * nk, C, s th, s tw] with nk = 8 when src_b is None, else
    nk = 4 and src_b [N * Tb * 4, C, s tw, s th] holds variants 4..7."""
    table = np.asarray(table)
    N, Tb = out.shape[0], len(table)
    nk = 8 if src_b is None else 4
    s = src_a.shape[2] // th
    a = src_a.reshape((N, Tb, nk) + src_a.shape[1:])
    b = None if src_b is None else src_b.reshape((N, Tb, 4) + src_b.shape[1:])
    for n in range(N):
        for t, (y0, x0, oy0, oy1, ox0, ox1) in enumerate(table.tolist()):
            vs = [back(a[n, t, k] if k < nk else b[n, t, k - 4], k) for k in range(8)]
            m = mean8(vs)[:, s * (oy0 - y0):s * (oy1 - y0), s * (ox0 - x0):s * (ox1 - x0)]
            out[n, :, s * oy0:s * oy1, s * ox0:s * ox1] = to_uint8(m) if out.dtype == np.uint8 else m
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(H, W):
    """The shipped face checkpoint, one caption of 9 words, an LR image of uniform noise [1, 3, H, W] (seed H * 1000 + W),
    low="lr": the float64 mean of eight runs of the CPU oracle on the torch.flip / transpose variants of the WHOLE image, each
    mapped back.  Returns (captions, lens, LR, {"fine" | "fake" | "att": [3 float64 arrays]}); computed once per size."""
    from conftest import load_npz, split_sd
    from oracle import tgsr_oracle as O
    w = load_npz("face_S8_weights.npz")
    sds = (split_sd(w, "E."), split_sd(w, "GL."), split_sd(w, "GH."))
    cap, lens, _, _ = O.synthetic_batch(1, fixed_len=9)
    g = torch.Generator().manual_seed(H * 1000 + W)
    LR = torch.rand(1, 3, H, W, generator=g) * 2 - 1
    acc = {k: [0.0] * 3 for k in SCALES}
    with torch.no_grad():
        for k in range(8):
            x = LR.transpose(2, 3) if k & 4 else LR
            x = torch.flip(x, [2]) if k & 2 else x
            x = torch.flip(x, [3]) if k & 1 else x
            x = x.contiguous()
            ref = O.sr_forward(*sds, cap, lens.tolist(), x, x)
            for name in SCALES:
                for i in range(3):
                    y = ref[name][i][0].double()
                    y = torch.flip(y, [2]) if k & 1 else y
                    y = torch.flip(y, [1]) if k & 2 else y
                    y = y.transpose(1, 2) if k & 4 else y
                    acc[name][i] = acc[name][i] + y
    return cap, lens, LR, {name: [(v / 8.0).numpy() for v in acc[name]] for name in SCALES}
