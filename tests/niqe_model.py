"""A numpy / scipy fp64 model of NIQE as tgsr_amd.niqe defines it (MATLAB's niqe / computefeature, BasicSR's calculate_niqe): what the
kernels of csrc/tgsr_niqe.hip and the torch path of niqe.py are held to.  It shares no code with either: scipy.ndimage filters,
scipy.special.gamma, np.roll and np.argmin over the whole table.  Besides the features it reports what decides whether a bitwise
comparison of alpha is meaningful: per fit the relative gap between the two table entries nearest to rn, and per scale the number
of MSCN elements with |m| < 1e-9 (a zero's sign is implementation-defined)."""
import warnings

import numpy as np
from scipy import special

BLOCK = 96
TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256.0
SHIFTS = [(0, 1), (1, 0), (1, 1), (1, -1)]
GAM = np.arange(0.2, 10.001, 0.001)
R_GAM = special.gamma(2.0 / GAM) ** 2 / (special.gamma(1.0 / GAM) * special.gamma(3.0 / GAM))


def window():
    k = np.arange(-3, 4, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * (7.0 / 6.0) ** 2))
    return w / w.sum()


def cubic(x, a=-0.5):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x <= 1, (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1, np.where(x < 2, a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a, 0.0))


def to_uint8(x):
    """float32 in [-1, 1] -> bytes by the library's rule: round_half_even(clip((x + 1) * 127.5, 0, 255)), fp32 add then multiply."""
    t = (np.asarray(x, dtype=np.float32) + np.float32(1.0)) * np.float32(127.5)
    return np.rint(np.clip(t, 0, 255)).astype(np.uint8)


def rgb2y(u8):
    """uint8 [3, H, W] -> uint8 [H, W], the reference's rgb2y: fp32 u / 255, then fp64 left to right, trunc(y 255 + 0.5)."""
    f = (u8.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    y = f[0] * (65.481 / 255.0) + f[1] * (128.553 / 255.0) + f[2] * (24.966 / 255.0) + 16 / 255.0
    return (y * 255.0 + 0.5).astype(np.uint8)


def plane(img, shave=0):
    """One image [3, H, W] (uint8, or float32 in [-1, 1]) -> the cropped fp64 Y plane."""
    u8 = img if img.dtype == np.uint8 else to_uint8(img)
    y = rgb2y(u8)
    y = y[shave:y.shape[0] - shave, shave:y.shape[1] - shave]
    if min(y.shape) < BLOCK:
        raise ValueError("niqe model: fewer than %d pixels on a side" % BLOCK)
    return y[:y.shape[0] // BLOCK * BLOCK, :y.shape[1] // BLOCK * BLOCK].astype(np.float64)


def correlate_rows(a, w):
    """Along the last axis with replicate borders, the products added left to right, each operation rounded on its own.  (It
    equals ndimage.correlate1d(a, w, mode="nearest") to rounding - the host tests check that - but ndimage adds in another order,
    and the order decides one thing: the window's weights add up to exactly 1 from left to right, so a constant plane whose value
    is a power of two, such as Y = 16 of black, comes out of this filter unchanged and its MSCN is exactly 0, not +-4e-15.)"""
    p = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(3, 3)], mode="edge")
    out = np.zeros_like(a)
    for k in range(7):
        out = out + w[k] * p[..., k:k + a.shape[-1]]
    return out


def mscn(y):
    w = window()
    f = lambda a: correlate_rows(correlate_rows(a, w).T, w).T
    mu = f(y)
    sigma = np.sqrt(np.abs(f(y * y) - mu * mu))
    return (y - mu) / (sigma + 1.0), sigma


def down2(y):
    def one(a):                                          # along the last axis
        n = a.shape[-1]
        idx = 2 * np.arange(n // 2)[:, None] - 3 + np.arange(8)[None, :]
        idx = np.where(idx < 0, -idx - 1, np.where(idx >= n, 2 * n - 1 - idx, idx))
        return (a[..., idx] * TAPS).sum(-1)
    return one(one(y).T).T


def aggd(x):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)             # np.mean of an empty side: NaN is the defined result
        l = np.sqrt(np.mean(x[x < 0] ** 2))
        r = np.sqrt(np.mean(x[x > 0] ** 2))
        g = l / r
        rhat = np.mean(np.abs(x)) ** 2 / np.mean(x ** 2)
        rn = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
        d = (R_GAM - rn) ** 2
        k = int(np.argmin(d))
        alpha = GAM[k]
        two = np.sort(np.abs(R_GAM - rn))[:2]
        gap = (two[1] - two[0]) / rn
        q = np.sqrt(special.gamma(1 / alpha) / special.gamma(3 / alpha))
    return alpha, l * q, r * q, gap


def block_features(m):
    feats, gaps = [], []
    alpha, bl, br, gap = aggd(m)
    feats += [alpha, (bl + br) / 2]
    gaps.append(gap)
    for s in SHIFTS:
        alpha, bl, br, gap = aggd(m * np.roll(m, s, axis=(0, 1)))
        feats += [alpha, (br - bl) * (special.gamma(2 / alpha) / special.gamma(1 / alpha)), bl, br]
        gaps.append(gap)
    return feats, gaps


def features(img, shave=0):
    """One image -> {"feats": [nblk, 36], "sharp": [nblk], "gaps": [nblk, 10], "near_zero": (scale 1, scale 2) - the MSCN elements
    with |m| < 1e-9 -, "exact_zero": (scale 1, scale 2) - those of them that are exactly 0}."""
    y = plane(img, shave)
    m1, sigma = mscn(y)
    m2, _ = mscn(down2(y))
    rows, sharp, gaps = [], [], []
    for by in range(y.shape[0] // BLOCK):
        for bx in range(y.shape[1] // BLOCK):
            f, g = [], []
            for m, n in ((m1, BLOCK), (m2, BLOCK // 2)):
                ff, gg = block_features(m[by * n:(by + 1) * n, bx * n:(bx + 1) * n])
                f += ff
                g += gg
            rows.append(f)
            gaps.append(g)
            sharp.append(sigma[by * BLOCK:(by + 1) * BLOCK, bx * BLOCK:(bx + 1) * BLOCK].mean())
    return {"feats": np.array(rows), "sharp": np.array(sharp), "gaps": np.array(gaps),
            "near_zero": (int((np.abs(m1) < 1e-9).sum()), int((np.abs(m2) < 1e-9).sum())),
            "exact_zero": (int((m1 == 0).sum()), int((m2 == 0).sum()))}


def fit(images, sharpness=0.75):
    """(mu_p, cov_p, the number of blocks kept) over the blocks of `images` (each [3, H, W]) whose sharpness exceeds `sharpness` x
    the image's largest."""
    rows = []
    for img in images:
        r = features(img)
        keep = (r["sharp"] > sharpness * r["sharp"].max()) & np.isfinite(r["feats"]).all(1)
        rows.append(r["feats"][keep])
    rows = np.concatenate(rows)
    return rows.mean(0), np.cov(rows, rowvar=False), rows.shape[0]


def pinv_sym(a):
    w, v = np.linalg.eigh(a)
    keep = np.abs(w) > 36 * 2.0 ** -52 * np.abs(w).max()
    return (v[:, keep] / w[keep]) @ v[:, keep].T


def score(feats, mu_p, cov_p):
    """feats [nblk, 36] of one image -> the NIQE score against (mu_p, cov_p)."""
    finite = ~np.isnan(feats).any(1)
    if finite.sum() < 2:
        return float("nan")
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mu = np.nanmean(feats, 0)
    cov = np.cov(feats[finite], rowvar=False)
    d = mu_p - mu
    return float(np.sqrt(d @ pinv_sym((cov_p + cov) / 2) @ d))
