"""Attention panels on the device: which word steered which region.

The reference's caller writes two files per image (trainer_objective.py gen_exampleSRHL): the SR image and the attention panel
built by `build_super_imagesall` (miscc/utils.py:328-451) from `attention_maps[0]` - one tile per caption word, that word's
attention map blurred, stretched and blended over the SR image.  This module builds the panel with csrc/tgsr_attnviz.hip
(torch.ops.tgsr.attn_panels); only the text strip above it is drawn on the host (PIL).  `build_super_images` (pretrain_DAMSM's
two-row variant: anti-aliased resize, global min / max, mask 210) is not built.

THE ARITHMETIC.  Per image: att [T, h, w] float32, cap_len n (words at and behind n are ignored), the image
[3, Vh, Vw] with (Vh, Vw) = (u h, u w), u >= 1 an integer.

Per word j < n (utils.py:389-401):
  1. thresh = 2 / n in fp64; every map value is widened to fp64 before it is compared.
  2. conf[j] = sum of x [x > 2 thresh]                                     (strict, as the reference's)
  3. x <- x [x > thresh]
  4. u > 1: expand, then blur.  The expand is linear interpolation at half-pixel centres with mirrored borders - exactly
     scipy.ndimage.zoom(x, u, order=1, mode='mirror', grid_mode=True); the blur exactly
     scipy.ndimage.gaussian_filter(., 20, mode='reflect', truncate=4.0), radius 80 - larger than a small tile, the reflection
     wraps several times.  Both are linear and separable: the tile is M_h x M_w^T with M = `expand_operator(a, u)`.
     Those two scipy calls are what current skimage's pyramid_expand(sigma=20, upscale=u) is read to make; skimage was not
     at hand, so that equivalence is UNVERIFIED.  The scipy calls are this module's definition.
  5. y = (x - min) / (max - min) * 255 over the tile, in that order, fp64
  6. truncated to uint8
  7. max == min (every value under the threshold; always for n = 1, where thresh = 2): the reference divides 0 / 0, here the
     tile is black.
Image bytes (utils.py:341-343): fp32 ((v + 1) / 2) * 255, round half to even, clamp to [0, 255].  An image that is not
Vh x Vw is resized first with F.interpolate(mode='bilinear', align_corners=False) on the device.
Blend (utils.py:412-416): Pillow's paste through a constant mask alpha (180): per channel t = m alpha + i (255 - alpha) + 128,
out = ((t >> 8) + t) >> 8.
Panel: uint8 [Vh, K (Vw + 2), 3]; tile k at columns k (Vw + 2) ... + Vw - 1, then two black columns.  K = n for
build_super_imagesall, min(topK, n) for build_super_images2, whose tiles go by descending conf, ties to the HIGHER word index
(the reference's tie order is whatever an unstable argsort gives).  In a batch, rows of shorter captions are black on the
right (an extension: the reference builds one image at a time).
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import custom_ops as C

FONT_MAX = 50                # rows of the text strip per caption (utils.py:28)
_OPERATORS = {}
_DEVICE_OPERATORS = {}


def _fold_mirror(i, n):
    """Index folding of scipy's 'mirror' (d c b | a b c d | c b a): period 2 n - 2, the edge sample not repeated."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def _fold_reflect(i, n):
    """Index folding of scipy's 'reflect' (d c b a | a b c d | d c b a): period 2 n, the edge sample repeated."""
    p = 2 * n
    i = np.mod(i, p)
    return np.where(i >= n, p - 1 - i, i)


def expand_operator(a, u, sigma=20.0, truncate=4.0):
    """float64 [a u, a]: the expand-then-blur of one axis as a matrix - linear interpolation at half-pixel centres with mirrored
    borders (ndimage.zoom order 1, mode 'mirror', grid_mode), then the Gaussian of radius int(truncate sigma + 0.5) with
    reflected borders (ndimage.gaussian_filter1d, mode 'reflect').  The identity for u = 1 (the reference neither expands nor
    blurs then).  numpy only; cached per (a, u, sigma, truncate) - do not write into the result."""
    a, u = int(a), int(u)
    if a < 1 or u < 1:
        raise ValueError("expand_operator: a %d, u %d" % (a, u))
    key = (a, u, float(sigma), float(truncate))
    M = _OPERATORS.get(key)
    if M is not None:
        return M
    V = a * u
    if u == 1:
        M = np.eye(a, dtype=np.float64)
    else:
        o = np.arange(V, dtype=np.float64)
        c = (o + 0.5) * (float(a) / float(V)) - 0.5                      # the source coordinate of output sample o
        i0 = np.floor(c)
        f = c - i0
        i0 = i0.astype(np.int64)
        Z = np.zeros((V, a), dtype=np.float64)
        rows = np.arange(V)
        np.add.at(Z, (rows, _fold_mirror(i0, a)), 1.0 - f)
        np.add.at(Z, (rows, _fold_mirror(i0 + 1, a)), f)
        r = int(float(truncate) * float(sigma) + 0.5)
        x = np.arange(-r, r + 1)
        phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x.astype(np.float64) ** 2)
        phi = phi / phi.sum()
        G = np.zeros((V, V), dtype=np.float64)
        for t, p in zip(x, phi):
            np.add.at(G, (rows, _fold_reflect(rows + t, V)), p)
        M = G @ Z
    M.setflags(write=False)
    _OPERATORS[key] = M
    return M


def _device_operator(a, u, dev):
    key = (a, u, str(dev))
    t = _DEVICE_OPERATORS.get(key)
    if t is None:
        t = _DEVICE_OPERATORS[key] = torch.from_numpy(np.array(expand_operator(a, u))).to(dev)
    return t


def panel_width(K, vis_w):
    return int(K) * (int(vis_w) + 2)


@torch.no_grad()
def attention_panels(images, att, cap_lens, *, top_k=None, alpha=180, with_maps=False, upscale=None):
    """images [B, 3, H, W] (float32 in [-1, 1], or uint8), att [B, T, h, w] float32, cap_lens B host ints in [1, T], all tensors
    on the device.  upscale: u, the tile is (u h, u w); None: H / h, which must be an integer and equal W / w (ValueError
    otherwise).  A float32 image of another size is resized to the tile (bilinear, align_corners=False).
    top_k=None: every word in caption order (build_super_imagesall), K = max(cap_lens); else the top_k words of each caption by
    descending conf (build_super_images2), K = min(top_k, max(cap_lens)).
    Returns {"panel": uint8 [B, Vh, K (Vw + 2), 3], "conf": float64 [B, T], "order": int32 [B, T] (the word of every slot s < n,
    -1 behind), "maps": uint8 [B, T, Vh, Vw] (with_maps; the un-blended map bytes)}, all on the device, nothing synchronised."""
    if att.dim() != 4 or images.dim() != 4 or images.shape[0] != att.shape[0] or images.shape[1] != 3:
        raise ValueError("attention_panels: images [B, 3, H, W] and att [B, T, h, w] expected, got %s and %s"
                         % (tuple(images.shape), tuple(att.shape)))
    B, T, h, w = att.shape
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    H, W = int(images.shape[2]), int(images.shape[3])
    if upscale is None:
        if H % h or W % w or H // h != W // w:
            raise ValueError("attention_panels: a %d x %d image is no integer multiple of the %d x %d attention maps (pass "
                             "upscale= to have it resized)" % (H, W, h, w))
        u = H // h
    else:
        u = int(upscale)
        if u < 1:
            raise ValueError("attention_panels: upscale %r" % (upscale,))
    Vh, Vw = u * h, u * w
    if (H, W) != (Vh, Vw):
        if images.dtype != torch.float32:
            raise ValueError("attention_panels: only a float32 image is resized (%d x %d to %d x %d)" % (H, W, Vh, Vw))
        images = F.interpolate(images, size=(Vh, Vw), mode="bilinear", align_corners=False)
    if top_k is not None and int(top_k) < 1:
        raise ValueError("attention_panels: top_k %r" % (top_k,))
    nmax = max(lens) if lens else 0
    K = nmax if top_k is None else min(int(top_k), nmax)
    dev = att.device
    panel, conf, order, maps = C.attn_panels(images, att, lens, _device_operator(h, u, dev), _device_operator(w, u, dev), u,
                                             int(alpha), K, top_k is not None, bool(with_maps))
    out = {"panel": panel, "conf": conf, "order": order}
    if with_maps:
        out["maps"] = maps
    return out


def _ascii(word):
    return str(word).encode("ascii", "ignore").decode("ascii")


def text_strip(captions, ixtoword, vis_w, order=None, font=None, numbered=False, n_cols=None):
    """The text rows above the panel, on the host (PIL), after drawCaption_no_order / drawCaption (utils.py:31-71): an `np.ones`
    background (value 1, not 0), FONT_MAX = 50 rows per caption, `word[:6]` in white at x = s (vis_w + 2) for slot s; a caption
    ends at its first 0 token.  order: None (slot s shows word s) or [B, >= n_cols] ints, the word of every slot (-1 = none): what
    build_super_images2's reordering of the text cells comes to.  numbered: the '%d:%s' form of drawCaption.  n_cols: the number of
    slots (default: the longest caption).  font: a path to a TrueType font, or None for ImageFont.load_default(size=50) - the
    reference's hard-coded font path is not reproduced.  Returns (uint8 [B 50, n_cols (vis_w + 2), 3], sentences)."""
    from PIL import Image, ImageDraw, ImageFont
    caps = np.asarray(captions.cpu() if torch.is_tensor(captions) else captions)
    if caps.ndim == 1:
        caps = caps[None]
    sentences = []
    for row in caps:
        words = []
        for tok in row:
            if int(tok) == 0:
                break
            words.append(_ascii(ixtoword[int(tok)]))
        sentences.append(words)
    if n_cols is None:
        n_cols = max([len(s) for s in sentences] + [1])
    n_cols = int(n_cols)
    if order is not None:
        order = np.asarray(order.cpu() if torch.is_tensor(order) else order)
    canvas = np.ones([len(sentences) * FONT_MAX, panel_width(n_cols, vis_w), 3], dtype=np.uint8)
    img = Image.fromarray(canvas)
    fnt = ImageFont.load_default(size=FONT_MAX) if font is None else ImageFont.truetype(font, FONT_MAX)
    d = ImageDraw.Draw(img)
    for i, words in enumerate(sentences):
        for s in range(n_cols):
            j = s if order is None else int(order[i][s]) if s < len(order[i]) else -1
            if j < 0 or j >= len(words):
                continue
            text = ("%d:%s" % (j, words[j][:6])) if numbered else words[j][:6]
            d.text((s * (int(vis_w) + 2), i * FONT_MAX), text, font=fnt, fill=(255, 255, 255, 255))
    return np.asarray(img).astype(np.uint8), sentences


def _super_images(real_imgs, captions, cap_lens, ixtoword, attn_maps, att_sze, att_sze1, vis_size, topK):
    if att_sze1 is None:
        att_sze1 = att_sze
    att_sze, att_sze1, vis_size = int(att_sze), int(att_sze1), int(vis_size)
    if vis_size % att_sze:
        raise ValueError("vis_size %d is no integer multiple of att_sze %d" % (vis_size, att_sze))
    u = vis_size // att_sze
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else np.asarray(cap_lens).reshape(-1).tolist())]
    if torch.is_tensor(attn_maps):
        att = attn_maps
    else:
        T = max(int(m.numel()) // (att_sze * att_sze1) for m in attn_maps)
        att = torch.zeros(len(attn_maps), T, att_sze, att_sze1, dtype=torch.float32, device=attn_maps[0].device)
        for b, m in enumerate(attn_maps):
            m = m.reshape(-1, att_sze, att_sze1)
            att[b, :m.shape[0]] = m
    att = att.reshape(att.shape[0], -1, att_sze, att_sze1).float()
    dev = att.device
    imgs = real_imgs[:att.shape[0]].to(dev)
    if imgs.dtype != torch.uint8:
        imgs = imgs.float()
    res = attention_panels(imgs, att, lens[:att.shape[0]], top_k=topK, upscale=u)
    panel = res["panel"].cpu().numpy()
    Vw = u * att_sze1
    strip, sentences = text_strip(captions, ixtoword, Vw, order=res["order"] if topK is not None else None,
                                  numbered=topK is not None, n_cols=panel.shape[2] // (Vw + 2))
    rows = []
    for b in range(panel.shape[0]):
        rows += [strip[b * FONT_MAX:(b + 1) * FONT_MAX], panel[b]]
    return np.concatenate(rows, 0).astype(np.uint8), sentences


def build_super_imagesall(real_imgs, captions, cap_lens, ixtoword, attn_maps, att_sze, att_sze1=None, vis_size=256):
    """utils.py:328-451 under its signature: every word of every caption, in caption order.  attn_maps: a [B, T, h, w] tensor or a
    list of per-image maps on the device.  Returns (uint8 numpy [B (50 + V), W, 3], sentences): per image the text strip on its
    panel row, ready for Image.fromarray(...).save."""
    return _super_images(real_imgs, captions, cap_lens, ixtoword, attn_maps, att_sze, att_sze1, vis_size, None)


def build_super_images2(real_imgs, captions, cap_lens, ixtoword, attn_maps, att_sze, att_sze1=None, vis_size=256, topK=5):
    """utils.py:202-326 under its signature: the topK words of every caption by descending conf, the text cells reordered with
    the tiles."""
    return _super_images(real_imgs, captions, cap_lens, ixtoword, attn_maps, att_sze, att_sze1, vis_size, int(topK))
