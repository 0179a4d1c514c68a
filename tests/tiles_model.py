"""Numpy model of the tile gather / stitch (tgsr_tiles.hip) and the shared whole-image oracle case of the tiling tests.
TEST INFRASTRUCTURE: pure numpy / the CPU oracle, imports nothing of the HIP library."""
import functools

import numpy as np
import torch

from conftest import load_npz, split_sd
from oracle import tgsr_oracle as O


def normalize_u8(a):
    """u8_normalize's arithmetic: float32 division, subtraction, division."""
    f = a.astype(np.float32)
    return (f / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)


def to_uint8(a):
    """trainer_objective.py:153-155 (numpy: round half to even), on float32."""
    a = np.asarray(a, np.float32)
    return np.round(np.maximum(0, np.minimum(255, (a + np.float32(1.0)) * np.float32(127.5)))).astype(np.uint8)


def gather(img, table, th, tw):
    """Windows [Tb, 3, th, tw] float32 of a planar [3, H, W] image (uint8: normalised; float32: copied)."""
    out = np.stack([img[:, y0:y0 + th, x0:x0 + tw] for y0, x0 in np.asarray(table)[:, :2]])
    return normalize_u8(out) if img.dtype == np.uint8 else out.astype(np.float32, copy=True)


def stitch(tiles, table, th, out):
    """Every window's owned rectangle of tiles [Tb, C, s th, s tw] into out [C, s H, s W] (in place; uint8 out: to_uint8)."""
    s = tiles.shape[2] // th
    for t, (y0, x0, oy0, oy1, ox0, ox1) in enumerate(np.asarray(table).tolist()):
        v = tiles[t][:, s * (oy0 - y0):s * (oy1 - y0), s * (ox0 - x0):s * (ox1 - x0)]
        out[:, s * oy0:s * oy1, s * ox0:s * ox1] = to_uint8(v) if out.dtype == np.uint8 else v
    return out


SCALES = {"fine": (2, 4, 8), "fake": (2, 4, 8), "att": (1, 2, 4)}


@functools.lru_cache(maxsize=None)
def face_case():
    """The case the exactness claim was verified on: the shipped face checkpoint, one caption of 9 words, LR and LRb uniform noise
    [1, 3, 64, 136] (seed 5), low="lr".  Returns (state dicts, captions, lens, LR, LRb, whole-image oracle outputs); computed once."""
    w = load_npz("face_S8_weights.npz")
    sds = (split_sd(w, "E."), split_sd(w, "GL."), split_sd(w, "GH."))
    cap, lens, _, _ = O.synthetic_batch(1, fixed_len=9)
    g = torch.Generator().manual_seed(5)
    LR = torch.rand(1, 3, 64, 136, generator=g) * 2 - 1
    LRb = torch.rand(1, 3, 64, 136, generator=g) * 2 - 1
    with torch.no_grad():
        ref = O.sr_forward(*sds, cap, lens.tolist(), LR, LRb)
    whole = {k: [t[0].numpy().copy() for t in ref[k]] for k in SCALES}
    return sds, cap, lens, LR, LRb, whole


def oracle_tiled(sds, cap, lens, LR, LRb, table, th, tw):
    """gather -> O.sr_forward per window -> stitch, all on the CPU: {"fine" | "fake" | "att": [3 whole-image arrays]}."""
    H, W = LR.shape[2:]
    lr_t, lrb_t = gather(LR[0].numpy(), table, th, tw), gather(LRb[0].numpy(), table, th, tw)
    outs = []
    with torch.no_grad():
        for t in range(len(table)):
            outs.append(O.sr_forward(*sds, cap, lens.tolist(), torch.from_numpy(lr_t[t:t + 1]), torch.from_numpy(lrb_t[t:t + 1])))
    res = {}
    for k, scales in SCALES.items():
        res[k] = []
        for i, s in enumerate(scales):
            tiles = np.concatenate([o[k][i].numpy() for o in outs])
            res[k].append(stitch(tiles, table, th, np.full((tiles.shape[1], s * H, s * W), np.nan, np.float32)))
    return res
