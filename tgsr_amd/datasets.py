"""The data edge of the SR path: the pieces of the reference's datasets.py the hot path touches.

  * `GpuImagePyramid`  - `get_imgs_blur` (datasets.py:151-197) on the GPU: HR pyramid, the pyramid re-grown from the LR
    image, and their GaussianBlur(radius=2) versions, normalised to [-1, 1].  The arithmetic is Pillow's (what
    `transforms.Resize` and `ImageFilter.GaussianBlur` delegate to), restated in integer HIP kernels
    (tgsr_resize_bilinear_u8 / tgsr_gaussian_blur_u8 / tgsr_u8_normalize): byte-identical pyramids, so an end-to-end
    run is no longer bound by the CPU image library.
  * `example_pyramid` - `get_imgsexampletestblur` (datasets.py:236-278) for one decoded image of any size: crop to a multiple of
    the scale, the LR image, and the same four lists; what `SRPipeline.upscale` takes its LR image from.
  * `RaggedImages`, `DeviceAugment`, `SRBatcher` - what stands in front of that pyramid in the reference's loaders, for a
    batch of decoded images of different sizes: the CUB bounding-box crop (datasets.py:115-123, `crop_box`),
    `transforms.Resize` (`resized_size`), RandomCrop + RandomHorizontalFlip (test1.py:184-186) or CenterCrop
    (datasets.py:1558-1560), fused into one launch that computes only the window (tgsr_augment_u8), byte-identical to the
    Pillow chain.  A caller's `Dataset.__getitem__` shrinks to "decode, return the array and the bbox".
  * `prepare_data` / `prepare_datablur` - datasets.py:33-109: sort the batch by caption length (descending, the
    pack_padded_sequence order) and move it to the device; same tuple layout as the reference.
  * `load_caption_pickle` - the `[captions, ixtoword, wordtoix]` pickle test1.py:118-127 writes and the datasets read.
Dataset classes, tokenising (nltk) and file walking stay with the caller: CPU-side data preparation, not the hot path.
"""
import math
import pickle

import numpy as np
import torch

from . import ops
from ._lib import TgsrError

_PB = 32 - 8 - 2       # Pillow's PRECISION_BITS


def _resize_tables(in_size: int, out_size: int):
    """Pillow precompute_coeffs (bilinear) in double -> (bounds int32 [out,2], taps int32 [out,ksize], ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        tot = sum(w)
        if tot != 0.0:
            w = [v / tot for v in w]
        kk[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    ik = np.where(kk < 0, -0.5 + kk * (1 << _PB), 0.5 + kk * (1 << _PB)).astype(np.int32)
    return bounds, ik, ksize


def gaussian_box_params(radius: float = 2.0, passes: int = 3):
    """Pillow _gaussian_blur_radius + ImagingHorizontalBoxBlur's weights: (int radius, ww, fw) (float32 like the C code)."""
    f = np.float32
    sigma2 = float(f(radius) * f(radius) / f(passes))
    L = math.sqrt(12.0 * sigma2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1) * (l + 1)))
    fr = f(l + a)
    r = int(fr)
    ww = int(f(1 << 24) / f(fr * f(2) + f(1)))
    return r, ww, ((1 << 24) - (r * 2 + 1) * ww) // 2


class GpuImagePyramid:
    """datasets.py:151-197 for a batch of already cropped HR images [B, 3, S, S] uint8 on the device.

        imgs, bic, imgsblur, bicblur = GpuImagePyramid((32, 64, 128, 256))(hr_u8)

    Each is a list over the scales of float32 [B, 3, s, s] in [-1, 1] (= the reference's `ret, bic, retb, bicb`);
    `u8=True` returns the uint8 pyramids instead."""

    def __init__(self, sizes=(32, 64, 128, 256), blur_radius: float = 2.0, device="cuda"):
        self.sizes = tuple(int(s) for s in sizes)
        self.device = torch.device(device)
        self.blur = gaussian_box_params(blur_radius, 3)
        self._tables = {}

    def _table(self, n_in, n_out):
        key = (n_in, n_out)
        t = self._tables.get(key)
        if t is None:
            b, k, ks = _resize_tables(n_in, n_out)
            t = self._tables[key] = (torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device), ks)
        return t

    def resize(self, x: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
        """PIL `resize((out_w, out_h), BILINEAR)` of planar uint8 images [..., H, W]."""
        H, W = x.shape[-2], x.shape[-1]
        return ops.resize_bilinear_u8(x, out_h, out_w, self._table(W, out_w) if out_w != W else None,
                                      self._table(H, out_h) if out_h != H else None)

    def gaussian_blur(self, x: torch.Tensor) -> torch.Tensor:
        """PIL `filter(ImageFilter.GaussianBlur(radius))` of planar uint8 images [..., H, W]."""
        r, ww, fw = self.blur
        return ops.gaussian_blur_u8(x, r, ww, fw, 3)

    @staticmethod
    def normalize(x: torch.Tensor) -> torch.Tensor:
        """ToTensor + Normalize((0.5,)*3, (0.5,)*3) (datasets.py:286-288)."""
        return ops.u8_normalize(x)

    def __call__(self, hr_u8: torch.Tensor, u8: bool = False):
        S = self.sizes[-1]
        if hr_u8.dim() != 4 or hr_u8.shape[1] != 3 or tuple(hr_u8.shape[2:]) != (S, S):
            raise TgsrError("GpuImagePyramid: expected [B,3,%d,%d] uint8, got %s" % (S, S, tuple(hr_u8.shape)))
        lr = self.resize(hr_u8, self.sizes[0], self.sizes[0])                     # `lrimg`, datasets.py:170
        ret, bic, retb, bicb = [], [], [], []
        for i, s in enumerate(self.sizes):
            re = self.resize(hr_u8, s, s) if i < len(self.sizes) - 1 else hr_u8    # :177-181
            bi = self.resize(lr, s, s)                                            # :191
            ret.append(re)
            retb.append(self.gaussian_blur(re))                                   # :186
            bic.append(bi)
            bicb.append(self.gaussian_blur(bi))                                   # :192
        if u8:
            return ret, bic, retb, bicb
        n = self.normalize
        return [n(t) for t in ret], [n(t) for t in bic], [n(t) for t in retb], [n(t) for t in bicb]


def example_pyramid(hr_u8: torch.Tensor, scale: int = 8, blur_radius: float = 2.0, u8: bool = False):
    """`get_imgsexampletestblur` (datasets.py:236-278; without the blurred lists, `get_imgsexampletest`, :200-233) for ONE decoded
    image of any size, planar uint8 [3, H, W] on the device: crop to a multiple of `scale` (the top-left corner stays),
    `lrimg = Resize((h / scale, w / scale))`, then per power of two from there up to `scale` the HR image resized to that size
    (the last one is the crop itself), the LR image re-grown to it, and their GaussianBlur(radius) versions.

        ret, bic, retb, bicb = example_pyramid(hr_u8)              # each a list of float32 [3, h s / scale, w s / scale] in [-1, 1]
        out = pipe.upscale(bic[0], caption, cap_len, lr_blur=bicb[0])   # bic[0] IS the LR image (a Resize to its own size returns it)

    Byte-identical to the Pillow chain (resize_bilinear_u8, gaussian_blur_u8, u8_normalize); `u8=True` returns the uint8 lists."""
    scale = int(scale)
    if (not torch.is_tensor(hr_u8) or hr_u8.dtype != torch.uint8 or hr_u8.dim() != 3 or hr_u8.shape[0] != 3 or not hr_u8.is_cuda):
        raise TgsrError("example_pyramid: expected a planar uint8 [3, H, W] device image")
    if scale < 1 or scale & (scale - 1):
        raise TgsrError("example_pyramid: scale %r is no power of two (the pyramid doubles from the LR size up)" % (scale,))
    h, w = int(hr_u8.shape[1]) // scale * scale, int(hr_u8.shape[2]) // scale * scale
    if h < scale or w < scale:
        raise TgsrError("example_pyramid: a %d x %d image has no whole %d x %d block" % (hr_u8.shape[1], hr_u8.shape[2], scale, scale))
    with torch.cuda.device(hr_u8.device):
        pyr = GpuImagePyramid((1,), blur_radius, hr_u8.device)
        img = hr_u8[:, :h, :w].contiguous()                                       # img.crop([0, 0, w, h]), :251
        lr = pyr.resize(img, h // scale, w // scale)                              # `lrimg`, :255
        ret, bic, retb, bicb = [], [], [], []
        s = 1
        while s <= scale:
            hs, ws = h // scale * s, w // scale * s
            re = pyr.resize(img, hs, ws) if s < scale else img                    # :261-265
            bi = pyr.resize(lr, hs, ws)                                           # :272
            ret.append(re)
            retb.append(pyr.gaussian_blur(re))                                    # :267
            bic.append(bi)
            bicb.append(pyr.gaussian_blur(bi))                                    # :274
            s *= 2
        if u8:
            return ret, bic, retb, bicb
        n = pyr.normalize
        return [n(t) for t in ret], [n(t) for t in bic], [n(t) for t in retb], [n(t) for t in bicb]


def crop_box(bbox, width: int, height: int):
    """datasets.py:115-123, integer for integer: the square of radius 0.75 max(w, h) about the centre of the CUB bounding
    box `bbox` = (x, y, w, h), clamped to the image -> (x1, y1, x2, y2) as `img.crop` takes them."""
    r = int(max(bbox[2], bbox[3]) * 0.75)
    center_x = int((2 * bbox[0] + bbox[2]) / 2)
    center_y = int((2 * bbox[1] + bbox[3]) / 2)
    y1 = max(0, center_y - r)
    y2 = min(int(height), center_y + r)
    x1 = max(0, center_x - r)
    x2 = min(int(width), center_x + r)
    return int(x1), int(y1), int(x2), int(y2)


def resized_size(w: int, h: int, size: int):
    """torchvision's `Resize(size)` rule for an int size: the shorter side becomes `size`, the other
    int(size * long / short) -> (ow, oh)."""
    if w <= h:
        return int(size), int(size * h / w)
    return int(size * w / h), int(size)


class RaggedImages:
    """A batch of decoded images of different sizes as ONE buffer: each H x W x 3 uint8 (interleaved, as a decoder leaves
    it), back to back.  `sizes` = [(H, W)], `offsets` = byte offset of each image, `data` = the flat uint8 buffer.

        batch = RaggedImages.pack(list_of_arrays)             # pinned host buffer + one non_blocking copy to the device
        DataLoader(..., collate_fn=lambda items: (RaggedImages.pack([it[0] for it in items], device=None), ...))
                                                              # in a worker: host only; `.to("cuda")` in the main process
    """

    def __init__(self, data: torch.Tensor, sizes, offsets):
        self.data, self.sizes, self.offsets = data, list(sizes), list(offsets)

    def __len__(self):
        return len(self.sizes)

    @property
    def nbytes(self) -> int:
        return int(self.data.numel())

    @classmethod
    def pack(cls, images, device="cuda", pin=None):
        """images: a list of H x W x 3 uint8 numpy arrays or tensors.  pin: page-lock the host buffer (default: whenever a HIP
        device is there, so that the copy is asynchronous); device=None keeps the batch on the host."""
        if len(images) < 1:
            raise TgsrError("RaggedImages.pack: an empty batch")
        views, sizes, offsets, n = [], [], [], 0
        for i, im in enumerate(images):
            t = im if torch.is_tensor(im) else (torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else None)
            if t is None or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise TgsrError("RaggedImages.pack: image %d is not an H x W x 3 uint8 array (%s)" % (
                    i, type(im).__name__ if t is None else "%s %s" % (t.dtype, tuple(t.shape))))
            views.append(t)
            sizes.append((int(t.shape[0]), int(t.shape[1])))
            offsets.append(n)
            n += 3 * sizes[-1][0] * sizes[-1][1]
        if n >= 2 ** 31:
            raise TgsrError("RaggedImages.pack: %d bytes in one batch (the descriptors hold int32 offsets)" % n)
        pin = torch.cuda.is_available() if pin is None else pin
        host = torch.empty(n, dtype=torch.uint8, pin_memory=bool(pin))
        for t, (h, w), o in zip(views, sizes, offsets):
            host[o:o + 3 * h * w].view(h, w, 3).copy_(t)
        batch = cls(host, sizes, offsets)
        return batch if device is None else batch.to(device)

    def to(self, device):
        return RaggedImages(self.data.to(device, non_blocking=True), self.sizes, self.offsets)


class DeviceAugment:
    """The transform chain of the reference's loaders for a ragged batch on the device, in one launch (ops.augment_u8):
    CUB bounding-box crop (datasets.py:115-123), `Resize(int(imsize * ratio))`, then
      mode="train": RandomCrop(imsize) + RandomHorizontalFlip() (test1.py:184-186, ratio 76/64);
      mode="eval" : CenterCrop(imsize) (datasets.py:1558-1560 with ratio 72/64).
    ratio 1 (or None) leaves the Resize out: the bare CenterCrop(imsize) of datasets.py:1726-1727.

        aug = DeviceAugment(256)
        plan = aug.plan(batch.sizes, bboxes, generator=g)     # host: int32 [B, 12] descriptors (ops.AUG_DESC)
        hr_u8 = aug(batch, plan)                              # [B, 3, 256, 256] uint8 = what GpuImagePyramid takes

    The random draws are this class's own stream: per image `top` from [0, oh - S], then `left` from [0, ow - S], then the flip
    with probability 1/2 - torchvision's order, from the given host torch.Generator, but not torchvision's numbers bit for bit.
    A source that reaches the crop smaller than `imsize` is refused (torchvision would pad it; the reference never
    meets one)."""

    def __init__(self, imsize: int, ratio: float = 76 / 64, mode: str = "train", device="cuda"):
        if mode not in ("train", "eval"):
            raise TgsrError("DeviceAugment: mode is 'train' or 'eval', got %r" % (mode,))
        self.imsize, self.ratio, self.mode = int(imsize), ratio, mode
        self.size = None if ratio is None or ratio == 1 else int(self.imsize * ratio)      # None: no Resize in the chain
        if self.imsize < 1 or (self.size is not None and self.size < self.imsize):
            raise TgsrError("DeviceAugment: Resize(%s) cannot hold a window of %d" % (self.size, self.imsize))
        self.device = torch.device(device)

    def plan(self, sizes, bboxes=None, generator=None) -> torch.Tensor:
        """sizes: [(H, W)] in pack order (or a RaggedImages); bboxes: None, or per image None / (x, y, w, h)."""
        if isinstance(sizes, RaggedImages):
            sizes = sizes.sizes
        if bboxes is not None and len(bboxes) != len(sizes):
            raise TgsrError("DeviceAugment.plan: %d bounding boxes for %d images" % (len(bboxes), len(sizes)))
        S, rows, off = self.imsize, [], 0
        for i, (H, W) in enumerate(sizes):
            H, W = int(H), int(W)
            box = (0, 0, W, H) if bboxes is None or bboxes[i] is None else crop_box(bboxes[i], W, H)
            cw, ch = box[2] - box[0], box[3] - box[1]
            if cw < 1 or ch < 1:
                raise TgsrError("DeviceAugment.plan: image %d (%d x %d) has an empty crop box %s" % (i, W, H, box))
            ow, oh = (cw, ch) if self.size is None else resized_size(cw, ch, self.size)
            if oh < S or ow < S:
                raise TgsrError("DeviceAugment.plan: image %d resizes to %d x %d, smaller than the %d window" % (i, ow, oh, S))
            if self.mode == "train":
                top = int(torch.randint(0, oh - S + 1, (1,), generator=generator))
                left = int(torch.randint(0, ow - S + 1, (1,), generator=generator))
                flip = int(float(torch.rand(1, generator=generator)) < 0.5)
            else:
                top, left, flip = int(round((oh - S) / 2.)), int(round((ow - S) / 2.)), 0
            rows.append((off, H, W) + box + (oh, ow, top, left, flip))
            off += 3 * H * W
        if off >= 2 ** 31:
            raise TgsrError("DeviceAugment.plan: %d bytes in one batch (the descriptors hold int32 offsets)" % off)
        return ops.check_augment_table(torch.tensor(rows, dtype=torch.int64).to(torch.int32), S, max(off, 1))

    def __call__(self, ragged: RaggedImages, plan: torch.Tensor) -> torch.Tensor:
        if len(plan) != len(ragged):
            raise TgsrError("DeviceAugment: a plan of %d images for a batch of %d" % (len(plan), len(ragged)))
        if ragged.data.device != self.device and not (ragged.data.is_cuda and self.device.index is None):
            ragged = ragged.to(self.device)
        with torch.cuda.device(ragged.data.device):
            return ops.augment_u8(ragged.data, plan, self.imsize)


class SRBatcher:
    """From decoded images to the pyramids of a training or evaluation step: DeviceAugment, then GpuImagePyramid.

        imgs, bic, imgsblur, bicblur = SRBatcher((32, 64, 128, 256), mode="train")(batch, bboxes, generator=g)

    the four lists `prepare_datablur` hands on (each float32 [B, 3, s, s] in [-1, 1] per scale; `u8=True`: the uint8 pyramids)."""

    def __init__(self, sizes=(32, 64, 128, 256), mode: str = "train", ratio: float = 76 / 64, blur_radius: float = 2.0, device="cuda"):
        self.augment = DeviceAugment(int(sizes[-1]), ratio, mode, device)
        self.pyramid = GpuImagePyramid(sizes, blur_radius, device)

    def __call__(self, ragged: RaggedImages, bboxes=None, generator=None, plan=None, u8: bool = False):
        if plan is None:
            plan = self.augment.plan(ragged.sizes, bboxes, generator)
        hr = self.augment(ragged, plan)
        with torch.cuda.device(hr.device):
            return self.pyramid(hr, u8=u8)


def _sorted_to(dev, cap_lens, lists):
    lens, idx = torch.sort(cap_lens, 0, True)
    return lens, idx, [[t[idx].to(dev) for t in lst] for lst in lists]


def prepare_data(data, cfg=None, device=None):
    """datasets.py:33-68: (imgs, captions, cap_lens, class_ids, keys, bic) -> the same six, sorted by caption length
    (descending) and on the device (`cfg.CUDA` picks cuda like the reference unless `device` is given)."""
    imgs, captions, captions_lens, class_ids, keys, bic = data
    dev = torch.device(device if device is not None else ("cuda" if (cfg is None or cfg.CUDA) else "cpu"))
    lens, idx, (real_imgs, real_bic) = _sorted_to(dev, captions_lens, (imgs, bic))
    captions = captions[idx].squeeze().to(dev)
    class_ids = class_ids[idx].numpy() if torch.is_tensor(class_ids) else np.asarray(class_ids)[idx.numpy()]
    keys = [keys[i] for i in idx.numpy()]
    return [real_imgs, captions, lens.to(dev), class_ids, keys, real_bic]


def prepare_datablur(data, cfg=None, device=None):
    """datasets.py:71-109: the eight-tuple form with the blurred pyramids (what gen_exampleSRHL unpacks,
    trainer_objective.py:109)."""
    imgs, captions, captions_lens, class_ids, keys, bic, blur, bicblur = data
    dev = torch.device(device if device is not None else ("cuda" if (cfg is None or cfg.CUDA) else "cpu"))
    lens, idx, (real_imgs, real_blur, real_bic, real_bicblur) = _sorted_to(dev, captions_lens, (imgs, blur, bic, bicblur))
    captions = captions[idx].squeeze().to(dev)
    class_ids = class_ids[idx].numpy() if torch.is_tensor(class_ids) else np.asarray(class_ids)[idx.numpy()]
    keys = [keys[i] for i in idx.numpy()]
    return [real_imgs, captions, lens.to(dev), class_ids, keys, real_bic, real_blur, real_bicblur]


def get_caption(sent_caption, words_num=18, rng=None):
    """datasets.py:461-477: zero-pad a caption to `words_num` tokens; a LONGER caption keeps a random subset of
    `words_num` word positions in their original order (np.random.shuffle of the positions, the first `words_num` of them,
    sorted).  `rng`: None = numpy's global generator, exactly the reference's draw (seed it with np.random.seed like
    test1.py:171 does); a np.random.RandomState / Generator for a private stream.  Returns (x int64 [words_num], x_len)."""
    c = np.asarray(sent_caption).astype('int64')
    x = np.zeros(words_num, dtype='int64')
    n = len(c)
    if n <= words_num:
        x[:n] = c
        return x, n
    ix = list(np.arange(n))
    (np.random if rng is None else rng).shuffle(ix)
    ix = np.sort(ix[:words_num])
    x[:] = c[ix]
    return x, words_num


def load_caption_pickle(path, words_num=18, rng=None):
    """The pickle test1.py:118-127 writes: `[captions (lists of word indices), ixtoword, wordtoix]`.  Returns
    (captions int64 [N, words_num], cap_lens int64 [N], ixtoword, wordtoix), every caption padded / cropped by
    `get_caption` (datasets.py:461-477: captions longer than `words_num` keep a random ordered subset of their words)."""
    with open(path, "rb") as f:
        x = pickle.load(f)
    caps, ixtoword, wordtoix = x[0], x[-2], x[-1]
    out = torch.zeros(len(caps), words_num, dtype=torch.int64)
    lens = torch.zeros(len(caps), dtype=torch.int64)
    for i, c in enumerate(caps):
        row, n = get_caption(list(c), words_num, rng)
        out[i] = torch.from_numpy(row)
        lens[i] = n
    return out, lens, ixtoword, wordtoix
