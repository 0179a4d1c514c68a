"""No-reference image quality on the device: NIQE (Mittal, Soundararajan and Bovik, "Making a completely blind image quality
analyzer", 2013) - how natural ONE image looks, without its ground truth.  Lower is better.

PSNR / SSIM (metrics.py) measure the distance to the ground truth and FID / KID (featdist.py) compare populations; NIQE is the
per-image figure of a GAN-SR table.  Its "model" is the mean and covariance of 36 hand-defined statistics over blocks of pristine
images - fitted here from any set of good images (NIQEModel.fit, e.g. the training set's HR images) or loaded from a published
parameter file.  A score is comparable with PUBLISHED NIQE numbers only against the published parameters, which are not shipped.

The definition (MATLAB's niqe / computefeature, BasicSR's calculate_niqe), everything fp64:
  plane     the uint8 Y plane (the library's rgb2y; float32 in [-1, 1] is quantised by to_uint8's rule), `shave` border pixels
            removed, cropped at the top-left to whole 96 x 96 blocks.  A 256 x 256 image has FOUR blocks: its covariance is thin.
  window    w[k] ~ exp(-k^2 / (2 (7/6)^2)), k = -3..3, sum 1, separable, replicate borders
  MSCN      mu = w * y, sigma = sqrt(|w * y^2 - mu^2|), m = (y - mu) / (sigma + 1)
  scale 2   y2 = the plane down-sampled by 2 with the taps [-3 -9 29 111 111 29 -9 -3] / 256 along rows, then columns (MATLAB's
            antialiased bicubic at 1/2; symmetric reflection; not rounded); MSCN of y2; blocks of 48 x 48 on the same grid
  features  per block and scale 18: aggd(m) -> (alpha, (beta_l + beta_r) / 2); for the shifts (0,1), (1,0), (1,1), (1,-1):
            aggd(m roll(m, s)) -> (alpha, (beta_r - beta_l) G(2/alpha) / G(1/alpha), beta_l, beta_r), the roll circular in the block
  aggd      the asymmetric generalised Gaussian fit by moment matching over the grid gam = np.arange(0.2, 10.001, 0.001)
  score     d = mu_p - nanmean(rows), S = (cov_p + cov(rows without NaN)) / 2, sqrt(d^T pinv(S) d); pinv by a symmetric
            eigendecomposition, eigenvalues with |w| <= 36 2^-52 max|w| dropped (MATLAB's rule); fewer than two such rows: NaN
  fit       over pristine images, the blocks whose sharpness (mean sigma of scale 1) exceeds 0.75 x the image's largest; mean and
            unbiased covariance of their finite rows

Device tensors run torch.ops.tgsr.niqe_features (csrc/tgsr_niqe.hip: two launches for a whole batch, no synchronisation) - a missing
library is an error, never a fall-back.  CPU tensors run the same definition in torch fp64 (host tests).
"""
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from . import custom_ops as C
from . import ops
from .featdist import solver_device
from .parallel import gather_rows

BLOCK = ops.NIQE_BLOCK
NFEAT = 36
TAPS = (-3, -9, 29, 111, 111, 29, -9, -3)          # / 256
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def gaussian_window():
    """The seven weights as the kernel's host code forms them: libm's exp, the sum from left to right.  In that order they add up
    to exactly 1, so a constant plane whose value is a power of two (Y = 16 of black) passes the filter unchanged: MSCN exactly 0."""
    e = [math.exp(-float(k * k) / (2.0 * (7.0 / 6.0) * (7.0 / 6.0))) for k in range(-3, 4)]
    return torch.tensor([v / sum(e) for v in e], dtype=torch.float64)


def _check_size(H, W, shave):
    if shave < 0 or H - 2 * shave < BLOCK or W - 2 * shave < BLOCK:
        raise ValueError("niqe: %d x %d images shaved by %d leave fewer than %d pixels on a side" % (H, W, shave, BLOCK))


# ----------------------------------------------------------------------------------------- the torch fp64 form
# (what CPU tensors run; it is written with operators that run on any device, and tools/niqe_timing.py times it on the GPU as the
# baseline of the kernels)
def _y_plane(img, shave):
    """[B, 3, H, W] uint8 or float32 -> the cropped Y plane, float64 [B, Hc, Wc] of byte values (rgb2y, byte for byte)."""
    if img.dtype == torch.float32:
        img = torch.clamp((img + 1.0) * 127.5, 0, 255).round().to(torch.uint8)
    f = (img.to(torch.float32) / 255.0).to(torch.float64)
    y = f[:, 0] * (65.481 / 255.0) + f[:, 1] * (128.553 / 255.0) + f[:, 2] * (24.966 / 255.0) + 16 / 255.0
    y = torch.floor(y * 255.0 + 0.5)
    H, W = y.shape[1] - 2 * shave, y.shape[2] - 2 * shave
    return y[:, shave:shave + H // BLOCK * BLOCK, shave:shave + W // BLOCK * BLOCK]


def _filter(a, w):
    """The separable window over [B, H, W] with replicate borders: along the rows, then along the columns."""
    p = torch.nn.functional.pad(a[:, None], (3, 3, 3, 3), mode="replicate")
    p = torch.nn.functional.conv2d(p, w.view(1, 1, 1, 7))
    return torch.nn.functional.conv2d(p, w.view(1, 1, 7, 1))[:, 0]


def _mscn(y):
    w = gaussian_window().to(y.device)
    mu = _filter(y, w)
    sigma = torch.sqrt(torch.abs(_filter(y * y, w) - mu * mu))
    return (y - mu) / (sigma + 1.0), sigma


def _down2(y):
    def one(a):
        n = a.shape[-1]
        idx = 2 * torch.arange(n // 2, device=a.device)[:, None] - 3 + torch.arange(8, device=a.device)[None, :]
        idx = torch.where(idx < 0, -idx - 1, torch.where(idx >= n, 2 * n - 1 - idx, idx))
        return (a[..., idx] * (torch.tensor(TAPS, dtype=torch.float64, device=a.device) / 256.0)).sum(-1)
    return one(one(y).transpose(1, 2)).transpose(1, 2)


def _blocks(m, n):
    """[B, H, W] -> [B, nblk, n, n], blocks row-major."""
    B, H, W = m.shape
    return m.view(B, H // n, n, W // n, n).permute(0, 1, 3, 2, 4).reshape(B, -1, n, n)


def _aggd(x):
    """x [..., n, n] -> (alpha, beta_l, beta_r), each [...]."""
    gam, r_gam = ops.niqe_table_on(x.device)
    x = x.flatten(-2)
    neg, pos, sq = x < 0, x > 0, x * x
    l = torch.sqrt((sq * neg).sum(-1) / neg.sum(-1))
    r = torch.sqrt((sq * pos).sum(-1) / pos.sum(-1))
    g = l / r
    rhat = x.abs().mean(-1) ** 2 / sq.mean(-1)
    rn = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
    ok = ~torch.isnan(rn)
    rs = torch.where(ok, rn, torch.zeros_like(rn))
    k = torch.searchsorted(r_gam, rs.contiguous()).clamp(max=r_gam.numel() - 1)
    km = (k - 1).clamp(min=0)
    k = torch.where((r_gam[km] - rs) ** 2 <= (r_gam[k] - rs) ** 2, km, k)
    alpha = gam[torch.where(ok, k, torch.zeros_like(k))]            # np.argmin over an all-NaN row is 0
    q = torch.sqrt(torch.exp(torch.lgamma(1 / alpha) - torch.lgamma(3 / alpha)))
    return alpha, l * q, r * q


def features_torch(img, shave=0):
    """niqe_features by torch operators on the image's own device."""
    y = _y_plane(img, shave)
    m1, sigma = _mscn(y)
    m2, _ = _mscn(_down2(y))
    cols = []
    for m, n in ((m1, BLOCK), (m2, BLOCK // 2)):
        b = _blocks(m, n)
        alpha, bl, br = _aggd(b)
        cols += [alpha, (bl + br) / 2]
        for s in SHIFTS:
            alpha, bl, br = _aggd(b * torch.roll(b, s, dims=(-2, -1)))
            cols += [alpha, (br - bl) * torch.exp(torch.lgamma(2 / alpha) - torch.lgamma(1 / alpha)), bl, br]
    return torch.stack(cols, -1), _blocks(sigma, BLOCK).mean((-2, -1))


@torch.no_grad()
def niqe_features(img, shave=0):
    """(feats float64 [B, nblk, 36], sharp float64 [B, nblk]) of `img` [B, 3, H, W], uint8 or float32 in [-1, 1]: the NIQE features
    (scale 1 first) and the sharpness of every 96 x 96 block, blocks row-major.  A device tensor: two launches, no synchronisation.
    Fewer than 96 pixels on a side after shaving is a ValueError."""
    shave = int(shave)
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype not in (torch.uint8, torch.float32):
        raise ValueError("niqe_features: uint8 or float32 [B, 3, H, W] expected, got %s %s" % (img.dtype, tuple(img.shape)))
    _check_size(img.shape[2], img.shape[3], shave)
    if img.is_cuda:
        return C.niqe_features(img.detach().contiguous(), shave)
    return features_torch(img.detach(), shave)


# ----------------------------------------------------------------------------------------- the model
_KEYS = (("mu", "cov"), ("mu_pris_param", "cov_pris_param"), ("mu_prisparam", "cov_prisparam"))


class NIQEModel:
    """The pristine model (mu [36], cov [36, 36], fp64 on `device`).  Built from parameters (`NIQEModel(mu, cov)`, `load`) or fitted
    (`fit`, or `add` batch by batch): a fitted model keeps n, sum x, sum x x^T of the kept blocks in fp64 on the device - `n` too, so
    that nothing synchronises - and `mu` / `cov` are read from them."""

    def __init__(self, mu=None, cov=None, device="cuda"):
        self.device = torch.device(device)
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.device)
        self.n, self.sum, self.outer = z(()), z(NFEAT), z(NFEAT, NFEAT)
        self._mu = self._cov = None
        if (mu is None) != (cov is None):
            raise ValueError("NIQEModel: mu and cov come together")
        if mu is not None:
            mu = torch.as_tensor(np.asarray(mu.cpu() if torch.is_tensor(mu) else mu, dtype=np.float64).reshape(-1))
            cov = torch.as_tensor(np.asarray(cov.cpu() if torch.is_tensor(cov) else cov, dtype=np.float64))
            if tuple(mu.shape) != (NFEAT,) or tuple(cov.shape) != (NFEAT, NFEAT):
                raise ValueError("NIQEModel: mu [36] and cov [36, 36] expected, got %s and %s" % (tuple(mu.shape), tuple(cov.shape)))
            self._mu, self._cov = mu.to(self.device), cov.to(self.device)

    # -- fitting
    def add(self, feats, sharp, sharpness=0.75):
        """Adds the kept blocks of a batch (niqe_features' pair): per image those whose sharpness exceeds `sharpness` x the image's
        largest and whose 36 features are finite.  No synchronisation."""
        if self._mu is not None:
            raise ValueError("NIQEModel.add: this model holds given parameters, not moments")
        feats, sharp = feats.to(self.device), sharp.to(self.device)
        keep = (sharp > float(sharpness) * sharp.max(1, keepdim=True).values) & torch.isfinite(feats).all(-1)
        x = torch.where(keep[..., None], feats, torch.zeros_like(feats)).reshape(-1, NFEAT)
        self.n += keep.sum()
        self.sum += x.sum(0)
        self.outer += x.t() @ x
        return self

    def merge(self, others):
        for o in ([others] if isinstance(others, NIQEModel) else others):
            if o._mu is not None or self._mu is not None:
                raise ValueError("NIQEModel.merge: only fitted models (moments) merge")
            self.n += o.n.to(self.device)
            self.sum += o.sum.to(self.device)
            self.outer += o.outer.to(self.device)
        return self

    def all_reduce(self, group=None):
        """The merge over the process group: one SUM all-reduce of (outer, sum, n); without an initialised group nothing happens."""
        if not (dist.is_available() and dist.is_initialized()) or self._mu is not None:
            return self
        flat = torch.cat([self.outer.reshape(-1), self.sum, self.n.reshape(1)])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        self.outer.copy_(flat[:NFEAT * NFEAT].view(NFEAT, NFEAT))
        self.sum.copy_(flat[NFEAT * NFEAT:-1])
        self.n.copy_(flat[-1])
        return self

    @classmethod
    def fit(cls, images, sharpness=0.75, shave=0, device=None):
        """The model of pristine `images`: an iterable of batches [B, 3, H, W] (uint8 or float32 in [-1, 1]; sizes may differ between
        batches).  Streaming: only the moments are kept."""
        model = None
        for img in images:
            if model is None:
                model = cls(device=img.device if device is None else device)
            model.add(*niqe_features(img, shave), sharpness=sharpness)
        if model is None:
            raise ValueError("NIQEModel.fit: no images")
        return model

    # -- parameters
    @property
    def mu(self):
        return self._mu if self._mu is not None else self.sum / self.n

    @property
    def cov(self):
        if self._cov is not None:
            return self._cov
        mu = self.sum / self.n
        c = (self.outer - self.n * torch.outer(mu, mu)) / (self.n - 1)
        return (c + c.t()) / 2

    def save(self, path):
        """An .npz of mu, cov (and the moments of a fitted model) at exactly `path`."""
        sd = {"mu": self.mu.cpu().numpy(), "cov": self.cov.cpu().numpy()}
        if self._mu is None:
            sd.update(n=self.n.cpu().numpy(), sum=self.sum.cpu().numpy(), outer=self.outer.cpu().numpy())
        with open(path, "wb") as f:
            np.savez(f, **sd)
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        """A model saved by `save`, BasicSR's parameter file (an .npz) or MATLAB's (a .mat, through scipy.io when scipy is present).
        Foreign files are recognised by the key pairs mu_pris_param / cov_pris_param and mu_prisparam / cov_prisparam - spellings
        written down from memory of those two packages and NOT verified against their files here."""
        path = os.fspath(path)
        if path.endswith(".mat"):
            try:
                from scipy import io as sio
            except ImportError as e:
                raise ValueError("NIQEModel.load: %s is a MATLAB file and scipy is not installed" % path) from e
            z = {k: v for k, v in sio.loadmat(path).items() if not k.startswith("__")}
        else:
            with np.load(path) as f:
                z = {k: f[k] for k in f.files}
        if "outer" in z:
            model = cls(device=device)
            model.n.copy_(torch.as_tensor(np.float64(z["n"])))
            model.sum.copy_(torch.from_numpy(np.asarray(z["sum"], dtype=np.float64)))
            model.outer.copy_(torch.from_numpy(np.asarray(z["outer"], dtype=np.float64)))
            return model
        for km, kc in _KEYS:
            if km in z and kc in z:
                return cls(z[km], z[kc], device)
        raise ValueError("NIQEModel.load: %s holds none of the key pairs %s (found %s)" % (path, _KEYS, sorted(z)))

    # -- scoring
    @torch.no_grad()
    def score_features(self, feats):
        """feats float64 [B, nblk, 36] -> the scores, float64 [B] on the features' device.  Batched torch fp64 on
        featdist.solver_device; no synchronisation where the eigensolver runs on the device."""
        home = feats.device
        dev = solver_device(home)
        x, mu_p, cov_p = feats.to(dev), self.mu.to(dev), self.cov.to(dev)
        mu = torch.nanmean(x, 1)
        valid = ~torch.isnan(x).any(-1)
        nv = valid.sum(1).to(torch.float64)
        xz = torch.where(valid[..., None], x, torch.zeros_like(x))
        mean_v = xz.sum(1) / nv[:, None]
        xc = torch.where(valid[..., None], x - mean_v[:, None], torch.zeros_like(x))
        cov = xc.transpose(1, 2) @ xc / (nv - 1)[:, None, None]
        S = (cov_p + cov) / 2
        ok = (nv >= 2) & ~torch.isnan(S).flatten(1).any(1)
        S = torch.where(ok[:, None, None], S, torch.eye(NFEAT, dtype=torch.float64, device=dev).expand_as(S))
        w, V = torch.linalg.eigh((S + S.transpose(1, 2)) / 2)
        keep = w.abs() > NFEAT * 2.0 ** -52 * w.abs().max(1, keepdim=True).values
        winv = torch.where(keep, 1.0 / torch.where(keep, w, torch.ones_like(w)), torch.zeros_like(w))
        t = ((mu_p - mu)[:, None, :] @ V)[:, 0]
        s = torch.sqrt((t * t * winv).sum(1))
        return torch.where(ok, s, torch.full_like(s, float("nan"))).to(home)

    def score(self, img, shave=0):
        """The NIQE score of every image of `img` [B, 3, H, W] (uint8 or float32 in [-1, 1]) against this model: float64 [B] on the
        image's device, lower is better."""
        return self.score_features(niqe_features(img, shave)[0])


class NIQEScores:
    """SRTrainer.evaluate's `niqe`: `add` per batch (the block features of the output and of its ground truth: 36 doubles per block,
    two launches per side, no synchronisation), `result` once at the end.  niqe=<a NIQEModel or the path of one>: both sides are
    scored against it.  niqe=True: the model is fitted from the ground-truth images seen; the fit and the scores happen in `result`,
    which leaves it in `model`."""

    def __init__(self, niqe=True, shave=0, device="cuda"):
        self.shave, self.device, self.model = int(shave), torch.device(device), None
        if niqe is not True:
            if not isinstance(niqe, (NIQEModel, str, os.PathLike)):
                raise ValueError("evaluate: niqe is True, a NIQEModel or the path of one, got %r" % (niqe,))
            self.model = niqe if isinstance(niqe, NIQEModel) else NIQEModel.load(niqe, self.device)
        self.seen = {"fine": [], "hr": []}

    def add(self, sr, hr):
        """A batch of outputs and its ground truth, [B, 3, H, W] each: 96 pixels on a side at least after `shave`."""
        self.seen["fine"].append(niqe_features(sr, self.shave))
        self.seen["hr"].append(niqe_features(hr, self.shave))

    def result(self):
        """{"fine": [N], "hr": [N], "mean": {"fine", "hr"}, "n": N}: the ground truth's own score is the row a table prints beside the
        method's; an image with fewer than two finite blocks scores NaN, and so does a mean over it.  Data parallel (call it once, on
        every rank): with niqe=True the fit's moments are all-reduced first, so every rank scores against the same model, and the rows
        are gathered in rank order."""
        if self.model is None:
            self.model = NIQEModel(device=self.device)
            for feats, sharp in self.seen["hr"]:
                self.model.add(feats, sharp)
            self.model.all_reduce()
        rows = {k: torch.cat([self.model.score_features(f) for f, _s in v]).cpu().numpy() for k, v in self.seen.items()}
        rows, _ = gather_rows(rows)
        return dict(rows, mean={k: float(np.mean(v)) for k, v in rows.items()}, n=int(rows["fine"].shape[0]))
