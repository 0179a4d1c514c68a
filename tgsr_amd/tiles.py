"""Whole-image inference by overlapping tiles: the host side of `SRPipeline.upscale`.

The x8 generators are fully convolutional (3x3 and 5x5 convolutions with zero padding, eval-mode BatchNorm, nearest
up-sampling, word attention that is a softmax over the words at each pixel separately), so an image of any size can be cut
into overlapping windows, run as an ordinary fixed-shape batch and put back together WITHOUT changing a value - if every
pixel a window owns is at least one receptive radius (`receptive_halo`) away from each window edge that is not an image
edge, and a window edge on the image edge sees the zero padding the whole image would see there.  `plan_axis` /
`plan_tiles` produce such windows; ops.tile_gather / ops.tile_stitch (tgsr_tiles.hip) cut and reassemble on the device.

The geometric self-ensemble (x8, `SRPipeline.upscale(ensemble=8)`, `SRPipeline.self_ensemble`) runs the network on the eight
flips and rotations of a window and averages the eight outputs, each mapped back.  THE TRANSFORM, stated once (repeated in
include/tgsr_hip.h; ops.d8_gather / ops.d8_merge, tgsr_ensemble.hip, implement it):

    variant k = 0..7 has bits b0 = k & 1 (mirror the columns), b1 = k & 2 (mirror the rows), b2 = k & 4 (transpose, applied
    first).  For a window `win` of th x tw, variant k has shape (th', tw') = (tw, th) if b2 else (th, tw); its pixel (i, j) is
    win[y][x] with  i' = th' - 1 - i if b1 else i,  j' = tw' - 1 - j if b0 else j,  (y, x) = (j', i') if b2 else (i', j').
    Outputs at scale s follow the same rule with every size multiplied by s.  The ensemble value of an output pixel is
    (((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125f in float32 - v_k = variant k's output at the position that maps
    back to the pixel, summed in ascending k: a fixed order, the same bits on every run.

`d8_shape` / `d8_index` / `d8_apply` / `d8_invert` are that definition as host reference maps.
"""
import math

import numpy as np
import torch
import torch.nn as nn

DEFAULT_TILE = 128      # SRPipeline.upscale's window side in LR pixels (measured: tools/upscale_timing.py)
D8 = 8                  # variants of the geometric self-ensemble: the symmetries of the square


def d8_shape(k: int, th: int, tw: int):
    """(th', tw'): the shape of variant k of a th x tw window."""
    if not 0 <= int(k) < D8:
        raise ValueError("d8: variant %r is not in 0..7" % (k,))
    return (int(tw), int(th)) if k & 4 else (int(th), int(tw))


def d8_index(k: int, th: int, tw: int):
    """(y, x): two int64 [th', tw'] tensors - pixel (i, j) of variant k is win[y[i, j], x[i, j]]."""
    hh, ww = d8_shape(k, th, tw)
    i, j = torch.meshgrid(torch.arange(hh), torch.arange(ww), indexing="ij")
    ii = hh - 1 - i if k & 2 else i
    jj = ww - 1 - j if k & 1 else j
    return (jj, ii) if k & 4 else (ii, jj)


def d8_apply(win, k: int):
    """Variant k of win [..., th, tw] (torch tensor or numpy array) by the index maps: [..., th', tw']."""
    y, x = d8_index(k, win.shape[-2], win.shape[-1])
    return win[..., y, x] if torch.is_tensor(win) else win[..., y.numpy(), x.numpy()]


def d8_invert(var, k: int):
    """The window [..., th, tw] whose variant k is var [..., th', tw']: every pixel put back where d8_index took it from."""
    hh, ww = var.shape[-2], var.shape[-1]
    th, tw = (ww, hh) if k & 4 else (hh, ww)
    y, x = d8_index(k, th, tw)
    if torch.is_tensor(var):
        out = var.new_empty(tuple(var.shape[:-2]) + (th, tw))
        out[..., y, x] = var
    else:
        out = np.empty(var.shape[:-2] + (th, tw), var.dtype)
        out[..., y.numpy(), x.numpy()] = var
    return out


def plan_axis(n: int, tile: int, halo: int):
    """Windows along one axis of n pixels: a list of (x0, own0, own1) - the window is [x0, x0 + tile), it owns [own0, own1).
    n >= tile > 2 * halo.  The windows never leave [0, n): the last one is clamped back to end at n.  A window edge is either the
    image edge or at least `halo` pixels away from every pixel the window owns; the owned intervals partition [0, n)."""
    n, tile, halo = int(n), int(tile), int(halo)
    if halo < 0 or tile <= 2 * halo or n < tile:
        raise ValueError("plan_axis: need n >= tile > 2 * halo >= 0, got n = %d, tile = %d, halo = %d" % (n, tile, halo))
    out, c0 = [], 0
    while True:
        x0 = min(max(c0 - halo, 0), n - tile)
        own1 = n if x0 + tile == n else x0 + tile - halo
        out.append((x0, c0, own1))
        c0 = own1
        if own1 == n:
            return out


def plan_tiles(H: int, W: int, tile, halo: int) -> torch.Tensor:
    """The product of the two axes' plans: host int32 [T, 6] rows (y0, x0, oy0, oy1, ox0, ox1), row-major over the windows.
    tile: one side, or (th, tw); an axis whose window is the whole side (th == H: an image shorter than the tile) has the one
    window that owns everything, whatever the halo - both its edges are image edges."""
    th, tw = (tile, tile) if isinstance(tile, int) else tile

    def axis(n, t):
        return [(0, 0, int(n))] if int(t) == int(n) else plan_axis(n, t, halo)
    rows = [(y0, x0, oy0, oy1, ox0, ox1) for y0, oy0, oy1 in axis(H, th) for x0, ox0, ox1 in axis(W, tw)]
    return torch.tensor(rows, dtype=torch.int32)


def _chain(mods, radius: float, res: float):
    """Receptive radius (in pixels of the chain's input) behind `mods` run one after the other, entered with `radius` at
    `res` output pixels per input pixel: a k x k convolution adds (k - 1) / 2 pixels of its own resolution, nearest
    up-sampling multiplies the resolution."""
    for m in mods:
        for leaf in m.modules():
            if isinstance(leaf, nn.Upsample):
                res *= float(leaf.scale_factor)
            elif isinstance(leaf, nn.Conv2d):
                k, s, d = leaf.kernel_size, leaf.stride, leaf.dilation
                if k[0] != k[1] or s != (1, 1) or d != (1, 1) or k[0] % 2 != 1:
                    raise ValueError("receptive_halo: %r is no stride-1 odd square convolution" % (leaf,))
                radius += (k[0] - 1) / 2.0 / res
    return radius, res


def receptive_radius(netGL, netGH) -> float:
    """The largest receptive radius, in LR pixels, of any output of the x8 generators (G_SR_NET_low's three images,
    NetG_highweight's three heads), counted from the modules: 3x3 and 5x5 convolutions at their resolution.  The word
    attention is per pixel (its 1x1 convolution runs over the words) and adds nothing."""
    try:
        stages = [([netGL.h_net1.im2f, netGL.h_net1.residual, netGL.h_net1.upsample], netGL.img_net1),
                  ([netGL.h_net2.residual, netGL.h_net2.upsample], netGL.img_net2),
                  ([netGL.h_net3.residual, netGL.h_net3.upsample], netGL.img_net3)]
        high = [([netGH.convin, netGH.residual, netGH.upscale2x], netGH.conv_output),
                ([netGH.residual24, netGH.upscale4x], netGH.conv_output),
                ([netGH.residual48, netGH.upscale8x], netGH.conv_output)]
    except AttributeError as e:
        raise ValueError("receptive_halo walks the x8 generators of tgsr_amd.model (G_SR_NET_low, NetG_highweight): %s" % e)
    worst = 0.0
    for net in (stages, high):
        r, res = 0.0, 1.0
        for trunk, head in net:
            r, res = _chain(trunk, r, res)
            worst = max(worst, _chain([head], r, res)[0])
    return worst


def receptive_halo(netGL, netGH) -> int:
    """The halo `upscale` needs: the ceiling of `receptive_radius` in LR pixels (16 for the shipped x8 networks:
    NetG_highweight reaches 15.625 - 13 from convin and the 12 ResBlock convolutions at LR resolution, 1.5 at 2x, 0.75 at 4x,
    0.125 + 0.25 at 8x; G_SR_NET_low 9)."""
    return int(math.ceil(receptive_radius(netGL, netGH) - 1e-9))
