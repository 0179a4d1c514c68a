"""Distribution distances on the device: does the output look like a real image?

PSNR / SSIM (metrics.py) measure the distance to the ground truth and R-precision (retrieval.py) the fit to the caption; the
Frechet distance (FID) and the kernel distance (KID) compare the DISTRIBUTION of the outputs' features with that of real images.

The feature space, stated once: the pooled 2048 of CNN_ENCODER's trunk (`image_encoder.run_trunk(images)[1]`), which has
torchvision's Inception-v3 topology.  With the Inception weights the reference's image encoder ships, a score is comparable across
this model's runs, snapshots and settings.  It equals a PUBLISHED FID / KID only with that benchmark's own Inception variant, which
differs in three pooling layers and in its weights; that variant is not built here.

  FeatureMoments     streaming n, sum x, sum x x^T of a feature set in fp64 (torch.ops.tgsr.feat_moments_add: one launch per batch,
                     no synchronisation); mergeable across batches, objects and data-parallel ranks; saved as an .npz
  frechet_distance   |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) of two moment sets, by two symmetric eigendecompositions
  kernel_distance    the unbiased MMD^2 under k(a, b) = (<a, b> / D + 1)^3 over random subsets (torch.ops.tgsr.poly_mmd_sums: one
                     call for all subsets), mean and standard deviation over the subsets
  FeatureBank        the feature batches kernel_distance reads, concatenated once
  RealismScores      what SRTrainer.evaluate(fid=, kid=) accumulates batch by batch and reports at the end

CPU tensors run the same arithmetic in torch fp64 (host tests, the gloo group); device tensors run the kernels of
csrc/tgsr_featdist.hip - a missing library is an error, never a fall-back.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from . import custom_ops as C
from . import ops

_SOLVER = {}          # device -> the device the symmetric eigensolver runs on


def solver_device(device):
    """Where torch.linalg.eigh runs for tensors on `device`: the device itself when this torch build has a solver there (probed
    once with a 2 x 2 matrix), the host otherwise - the two moment sets are then moved there and the same lines run."""
    device = torch.device(device)
    if device.type == "cpu":
        return device
    if device not in _SOLVER:
        try:
            torch.linalg.eigvalsh(torch.eye(2, dtype=torch.float64, device=device))
            _SOLVER[device] = device
        except RuntimeError:
            _SOLVER[device] = torch.device("cpu")
    return _SOLVER[device]


class FeatureMoments:
    """n (a host int), sum [D] and outer [D, D] (fp64, on `device`) of a set of float32 feature rows.  On a HIP device `outer` holds
    the block-upper part the kernel maintains (include/tgsr_hip.h); `outer_full()` / `mean_cov()` mirror its upper triangle."""

    def __init__(self, D, device="cuda"):
        self.D, self.device, self.n = int(D), torch.device(device), 0
        if self.D < 1:
            raise ValueError("FeatureMoments: D = %d" % self.D)
        self.sum = torch.zeros(self.D, dtype=torch.float64, device=self.device)
        self.outer = torch.zeros(self.D, self.D, dtype=torch.float64, device=self.device)

    def add(self, feats):
        """feats float32 [n, D] on this object's device: one launch, no synchronisation (a CPU tensor: outer.addmm_(X^T, X))."""
        if feats.dim() != 2 or feats.shape[1] != self.D or feats.dtype != torch.float32:
            raise ValueError("FeatureMoments.add: float32 [n, %d] expected, got %s %s" % (self.D, feats.dtype, tuple(feats.shape)))
        if feats.shape[0] == 0:
            return self
        feats = feats.detach()
        if feats.is_cuda:
            C.feat_moments_add(feats, self.sum, self.outer)
        else:
            X = feats.to(torch.float64)
            self.sum += X.sum(0)
            self.outer.addmm_(X.t(), X)
        self.n += int(feats.shape[0])
        return self

    def merge(self, others):
        """Adds the moments of other objects (or of one): the moments of the union of the sets."""
        for o in ([others] if isinstance(others, FeatureMoments) else others):
            if o.D != self.D:
                raise ValueError("FeatureMoments.merge: D = %d into D = %d" % (o.D, self.D))
            self.n += o.n
            self.sum += o.sum.to(self.device)
            self.outer += o.outer.to(self.device)
        return self

    def all_reduce(self, group=None):
        """The merge over the process group: ONE SUM all-reduce of (sum, outer, n) as a flat fp64 buffer; every rank ends with the
        moments of the union.  Without an initialised group nothing happens."""
        if not (dist.is_available() and dist.is_initialized()):
            return self
        flat = torch.cat([self.outer.reshape(-1), self.sum, torch.tensor([float(self.n)], dtype=torch.float64, device=self.device)])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        DD = self.D * self.D
        self.outer.copy_(flat[:DD].view(self.D, self.D))
        self.sum.copy_(flat[DD:DD + self.D])
        self.n = int(round(float(flat[-1])))
        return self

    def outer_full(self):
        """sum x x^T as a full matrix that equals its transpose bit for bit: the upper triangle, mirrored."""
        return torch.triu(self.outer) + torch.triu(self.outer, 1).t()

    def mean_cov(self):
        """(mu [D], S [D, D]) in fp64: mu = sum / n, S = (outer - n mu mu^T) / (n - 1), S == S^T bit for bit."""
        if self.n < 2:
            raise ValueError("FeatureMoments.mean_cov: %d rows (two at least)" % self.n)
        mu = self.sum / self.n
        return mu, (self.outer_full() - self.n * torch.outer(mu, mu)) / (self.n - 1)

    def state_dict(self):
        return {"n": np.int64(self.n), "sum": self.sum.cpu().numpy().copy(), "outer": self.outer.cpu().numpy().copy()}

    def load_state_dict(self, sd):
        s, o = np.asarray(sd["sum"], dtype=np.float64), np.asarray(sd["outer"], dtype=np.float64)
        if s.shape != (self.D,) or o.shape != (self.D, self.D):
            raise ValueError("FeatureMoments.load_state_dict: D = %d, got sum %s and outer %s" % (self.D, s.shape, o.shape))
        self.n = int(sd["n"])
        self.sum.copy_(torch.from_numpy(s.copy()))
        self.outer.copy_(torch.from_numpy(o.copy()))
        return self

    def save(self, path):
        """An .npz of n, sum, outer at exactly `path`: a ground-truth set's statistics are computed once and reused."""
        with open(path, "wb") as f:
            np.savez(f, **self.state_dict())
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path) as z:
            return cls(z["sum"].shape[0], device).load_state_dict({k: z[k] for k in ("n", "sum", "outer")})


def _sqrt_trace(c1, c2):
    """tr (c1 c2)^(1/2) for symmetric positive semi-definite c1, c2, in its symmetric form: c1 = V diag(w) V^T,
    A = V diag(sqrt(max(w, 0))), then the sum of sqrt(max(eigvalsh(sym(A^T c2 A)), 0))."""
    w, V = torch.linalg.eigh(c1)
    A = V * torch.sqrt(torch.clamp(w, min=0.0))
    M = A.t() @ c2 @ A
    return torch.sqrt(torch.clamp(torch.linalg.eigvalsh((M + M.t()) / 2), min=0.0)).sum()


@torch.no_grad()
def frechet_distance(a, b):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) of two FeatureMoments, everything in fp64 on solver_device(a.device)
    (one synchronisation: the returned float).  The result is NOT clamped at 0 and no epsilon is added to a diagonal: a set against
    itself gives a value of rounding size that may be negative (at D = 2048, n = 64 - rank deficient - about -7e-6)."""
    (m1, c1), (m2, c2) = a.mean_cov(), b.mean_cov()
    if m1.shape != m2.shape:
        raise ValueError("frechet_distance: D = %d against D = %d" % (m1.shape[0], m2.shape[0]))
    dev = solver_device(m1.device)
    m1, c1, m2, c2 = (t.to(dev) for t in (m1, c1, m2, c2))
    d = m1 - m2
    return float(d.dot(d) + torch.trace(c1) + torch.trace(c2) - 2.0 * _sqrt_trace(c1, c2))


class FeatureBank:
    """The feature batches of one set, kept as they come (no copy, no synchronisation) and concatenated once."""

    def __init__(self):
        self.batches, self._cat = [], None

    def add(self, feats):
        self.batches.append(feats.detach())
        self._cat = None
        return self

    def __len__(self):
        return sum(int(b.shape[0]) for b in self.batches)

    def cat(self):
        if self._cat is None:
            if not self.batches:
                raise ValueError("FeatureBank: empty")
            self._cat = self.batches[0] if len(self.batches) == 1 else torch.cat(self.batches)
            self.batches = [self._cat]
        return self._cat


def subset_tables(nx, ny, subsets, m, generator=None):
    """(ix, iy): int32 [subsets, m] host tables, row s of each drawn without replacement from [0, nx) / [0, ny) - ix[s] first, then
    iy[s].  Deterministic under `generator`'s seed."""
    ix, iy = torch.empty(subsets, m, dtype=torch.int32), torch.empty(subsets, m, dtype=torch.int32)
    for s in range(subsets):
        ix[s] = torch.randperm(nx, generator=generator)[:m]
        iy[s] = torch.randperm(ny, generator=generator)[:m]
    return ix, iy


def _poly_mmd_sums_host(x, y, ix, iy):
    D = x.shape[1]
    rows = []
    for tx, ty in zip(ix.long(), iy.long()):
        X, Y = x[tx].to(torch.float64), y[ty].to(torch.float64)
        kxx, kyy, kxy = ((P @ Q.t() / D + 1.0) ** 3 for P, Q in ((X, X), (Y, Y), (X, Y)))
        rows.append(torch.stack([kxx.sum() - kxx.diagonal().sum(), kyy.sum() - kyy.diagonal().sum(), kxy.sum()]))
    return torch.stack(rows)


@torch.no_grad()
def kernel_distance(fx, fy, subsets=100, subset_size=1000, generator=None):
    """KID of two feature sets (float32 [nx, D] and [ny, D] tensors, or FeatureBanks): `subsets` random subsets of m =
    min(subset_size, nx, ny) rows of each side (subset_tables, on the host), per subset the unbiased
    MMD^2 = sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2 of the three kernel sums, k(a, b) = (<a, b> / D + 1)^3.
    Returns {"mean": float, "std": float (over the subsets, population form), "per_subset": float64 [subsets] on the features'
    device}.  One poly_mmd_sums call serves all subsets; one synchronisation, at the end."""
    fx = fx.cat() if isinstance(fx, FeatureBank) else fx
    fy = fy.cat() if isinstance(fy, FeatureBank) else fy
    if fx.dim() != 2 or fy.dim() != 2 or fx.shape[1] != fy.shape[1]:
        raise ValueError("kernel_distance: [nx, D] and [ny, D] expected, got %s and %s" % (tuple(fx.shape), tuple(fy.shape)))
    nx, ny = int(fx.shape[0]), int(fy.shape[0])
    m, S = min(int(subset_size), nx, ny), int(subsets)
    if m < 2 or S < 1:
        raise ValueError("kernel_distance: %d subsets of %d rows (sets of %d and %d rows)" % (S, m, nx, ny))
    ix, iy = subset_tables(nx, ny, S, m, generator)
    sums = C.poly_mmd_sums(fx, fy, ix, iy) if fx.is_cuda else _poly_mmd_sums_host(fx, fy, ix, iy)
    per = sums[:, 0] / (m * (m - 1.0)) + sums[:, 1] / (m * (m - 1.0)) - 2.0 * sums[:, 2] / (float(m) * m)
    mean, std = torch.stack([per.mean(), per.std(unbiased=False)]).tolist()          # the synchronisation
    return {"mean": mean, "std": std, "per_subset": per}


# ----------------------------------------------------------------------------------------- what a validation loop accumulates
def pooled_of_truth(image_encoder, hr):
    """The pooled features of a ground-truth batch `hr` (float32 in [-1, 1], or uint8: normalised first): one trunk walk."""
    return image_encoder.run_trunk(hr if hr.dtype == torch.float32 else ops.u8_normalize(hr))[1]


def moments_add(moments, pooled, device):
    """`pooled` added to `moments` - a new FeatureMoments of the batch's width on `device` without one.  Returns the moments."""
    return (FeatureMoments(pooled.shape[1], device) if moments is None else moments).add(pooled)


def realism_args(fid, kid):
    """(fid, kid) as RealismScores reads them: False is None (not asked for), kid=True is {} (kernel_distance's defaults)."""
    return None if fid is False else fid, None if kid is False else ({} if kid is True else kid)


class RealismScores:
    """SRTrainer.evaluate's `fid` / `kid`: `add` per batch (one launch per moment set, no synchronisation), `result` once at the end.
    fid=True: the Frechet distance between the outputs' moments and the ground truth's, both accumulated here.  fid=<a
    FeatureMoments or the path of a saved one>: the ground-truth side comes from those statistics.  kid=True or {"subsets": ...,
    "subset_size": ...}: both feature banks are kept for kernel_distance.  `needs_truth` says whether `add` wants the ground truth's
    features - with saved statistics and no `kid` it does not, and the caller skips that trunk walk."""

    def __init__(self, fid=None, kid=None, device="cuda"):
        self.fid, self.kid = realism_args(fid, kid)
        self.device = torch.device(device)
        if self.kid is not None and not (isinstance(self.kid, dict) and set(self.kid) <= {"subsets", "subset_size"}):
            raise ValueError("evaluate: kid is True or a dict of subsets / subset_size, got %r" % (self.kid,))
        self.mom_sr = self.mom_gt = self.bank_sr = self.bank_gt = None
        if self.fid is not None and self.fid is not True:
            self.mom_gt = self.fid if isinstance(self.fid, FeatureMoments) else FeatureMoments.load(os.fspath(self.fid), self.device)
        if self.kid is not None:
            self.bank_sr, self.bank_gt = FeatureBank(), FeatureBank()
        self.needs_truth = self.fid is True or self.kid is not None

    def add(self, pooled_sr, pooled_gt=None):
        """The pooled features [B, D] of a batch of outputs and - `needs_truth` - of its ground truth.  The moment sets take their
        width from the first batch."""
        if self.fid is not None:
            self.mom_sr = moments_add(self.mom_sr, pooled_sr, self.device)
        if self.fid is True:
            self.mom_gt = moments_add(self.mom_gt, pooled_gt, self.device)
        if self.kid is not None:
            self.bank_sr.add(pooled_sr)
            self.bank_gt.add(pooled_gt)

    def result(self, generator=None):
        """{"fid": {"fine": the Frechet distance, "n": the images seen}} and / or {"kid": kernel_distance's result, subsets drawn
        from `generator`}, as asked for.  Data parallel: the accumulated moments are all-reduced first (call it once, on every
        rank), so every rank returns the same "fid"; "kid" scores the calling rank's items only."""
        out = {}
        if self.fid is not None:
            self.mom_sr.all_reduce()
            if self.fid is True:
                self.mom_gt.all_reduce()
            out["fid"] = {"fine": frechet_distance(self.mom_sr, self.mom_gt), "n": self.mom_sr.n}
        if self.kid is not None:
            out["kid"] = kernel_distance(self.bank_sr, self.bank_gt, generator=generator, **self.kid)
        return out
