"""How good an SR image is: PSNR / RMSE on RGB and on Y, SSIM on Y, against ground truth - on uint8 images, as the reference's
caller saves them (trainer_objective.py:153-155) and its `psnr` / `rgb2y` (:168-181) score them.

The device part is `torch.ops.tgsr.sr_metrics` (exact integer sums of squared byte differences and the fp64 sum of the SSIM
windows, per image); the few scalar operations behind it - sqrt, log10, the division by the window count - run here in numpy
float64, in the reference's order, so PSNR and RMSE equal the reference's bit for bit.  SSIM has no counterpart in the reference:
Wang et al. 2004 as in ssim.m (11 x 11 Gaussian window of sigma 1.5, 'valid', K1 = 0.01, K2 = 0.03, L = 255).
"""
import numpy as np

import torch

from . import custom_ops as _C  # noqa: F401   (registers torch.ops.tgsr.*)
from .parallel import dp_world, gather_rows

WINDOW = 11
KEYS = ("psnr", "rmse", "psnr_y", "rmse_y", "ssim_y")


def psnr_from_sse(sse, n):
    """(psnr, rmse) in float64 from a sum of squared byte differences over n values: rmse = sqrt(sse / n),
    psnr = 20 log10(255 / rmse) - the reference's `psnr` (trainer_objective.py:177-181), whose float64 mean of integer squares is
    this quotient exactly.  Identical images give (inf, 0) without a warning."""
    sse = np.asarray(sse, dtype=np.float64)
    rmse = np.sqrt(sse / np.float64(n))
    with np.errstate(divide="ignore"):
        psnr = 20 * np.log10(255 / rmse)
    return psnr, rmse


def crop_counts(H, W, shave=0):
    """(pixels, SSIM windows) of an H x W image with `shave` pixels removed from every border."""
    shave = int(shave)
    Hc, Wc = int(H) - 2 * shave, int(W) - 2 * shave
    if shave < 0 or Hc < WINDOW or Wc < WINDOW:
        raise ValueError("metrics: %d x %d images shaved by %d leave a crop under %d x %d" % (H, W, shave, WINDOW, WINDOW))
    return Hc * Wc, (Hc - WINDOW + 1) * (Wc - WINDOW + 1)


def scores_from_rows(rows, H, W, shave=0):
    """The score dict of [B, 3] rows (SSE RGB, SSE Y, SSIM sum) of H x W images: float64 arrays of length B."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    pixels, windows = crop_counts(H, W, shave)
    psnr, rmse = psnr_from_sse(rows[:, 0], 3 * pixels)
    psnr_y, rmse_y = psnr_from_sse(rows[:, 1], pixels)
    return {"psnr": psnr, "rmse": rmse, "psnr_y": psnr_y, "rmse_y": rmse_y, "ssim_y": rows[:, 2] / np.float64(windows)}


def image_scores(sr, hr, shave=0):
    """sr, hr: device tensors [B, 3, H, W], float32 in the generators' [-1, 1] range or uint8.  Returns float64 arrays of length
    B: psnr, rmse (RGB), psnr_y, rmse_y, ssim_y.  One synchronisation (the copy of B x 3 numbers)."""
    rows = torch.ops.tgsr.sr_metrics(sr, hr, int(shave))
    return scores_from_rows(rows.cpu().numpy(), sr.shape[2], sr.shape[3], shave)


class ScoreBook:
    """The rows of many batches, per output scale, kept on the device: `add` launches the kernels and returns, `result`
    synchronises once."""

    def __init__(self, shave=0):
        self.shave = int(shave)
        self._rows = {}          # scale name -> list of device tensors [b, 3]
        self._size = {}          # scale name -> (H, W)
        self._host = {}          # scale name -> list of numpy [b, 3] (merged books)

    def add(self, scale, sr, hr):
        """Score one batch of scale `scale` (any hashable name).  No synchronisation."""
        size = (int(sr.shape[2]), int(sr.shape[3]))
        if self._size.setdefault(scale, size) != size:
            raise ValueError("ScoreBook: scale %r held %s images, now %s" % (scale, self._size[scale], size))
        crop_counts(size[0], size[1], self.shave)
        self._rows.setdefault(scale, []).append(torch.ops.tgsr.sr_metrics(sr, hr, self.shave))

    def rows(self, scale):
        """All rows of a scale as one float64 numpy array [N, 3] (synchronises)."""
        parts = list(self._host.get(scale, []))
        dev = self._rows.get(scale, [])
        if dev:
            parts.append(torch.cat(dev, 0).cpu().numpy())
        return np.concatenate(parts, 0) if parts else np.zeros((0, 3), dtype=np.float64)

    def device_rows(self, scale):
        """The device rows of a scale as one tensor [N, 3] (no synchronisation)."""
        return torch.cat(self._rows[scale], 0)

    def scales(self):
        return [s for s in self._size]

    def result(self):
        """{scale: {"psnr": [N], ..., "mean": {"psnr": float, ...}, "n": N}}.  One device-to-host copy per scale."""
        out = {}
        for scale in self.scales():
            H, W = self._size[scale]
            sc = scores_from_rows(self.rows(scale), H, W, self.shave)
            sc["n"] = int(sc["psnr"].shape[0])
            sc["mean"] = {k: float(np.mean(sc[k])) if sc["n"] else float("nan") for k in KEYS}
            out[scale] = sc
        return out

    def all_gather(self):
        """The book of every rank's rows, merged in rank order: a host-side book, the same on every rank (one all_gather_object;
        synchronises).  Without an initialised group: this book itself."""
        if dp_world() == 1:
            return self
        rows, sizes = gather_rows({s: self.rows(s) for s in self.scales()}, self._size)
        size = {}
        for rank_sizes in sizes:
            for scale, hw in rank_sizes.items():
                if size.setdefault(scale, hw) != hw:
                    raise ValueError("ScoreBook.all_gather: scale %r holds %s and %s images" % (scale, size[scale], hw))
        return ScoreBook.from_rows(rows, size, self.shave)

    @classmethod
    def from_rows(cls, rows_by_scale, sizes, shave=0):
        """A host-side book: rows_by_scale {scale: array [N, 3]}, sizes {scale: (H, W)}."""
        book = cls(shave)
        for scale, rows in rows_by_scale.items():
            book._size[scale] = (int(sizes[scale][0]), int(sizes[scale][1]))
            book._host[scale] = [np.asarray(rows, dtype=np.float64).reshape(-1, 3)]
        return book

    @classmethod
    def merge(cls, books):
        """One book of the books of several ranks, rows in rank order."""
        books = list(books)
        if not books:
            raise ValueError("ScoreBook.merge: no books")
        shave = books[0].shave
        out = cls(shave)
        for b in books:
            if b.shave != shave:
                raise ValueError("ScoreBook.merge: books shaved by %d and %d" % (shave, b.shave))
            for scale in b.scales():
                if out._size.setdefault(scale, b._size[scale]) != b._size[scale]:
                    raise ValueError("ScoreBook.merge: scale %r holds %s and %s images" % (scale, out._size[scale], b._size[scale]))
                out._host.setdefault(scale, []).append(b.rows(scale))
        return out
