"""numpy restatement of the metric definitions of tgsr_amd.metrics / tgsr_metrics.hip: what the tests hold
the kernels to.  Images are [..., 3, H, W]."""
import hashlib

import numpy as np

WINDOW, SIGMA, K1, K2, PEAK = 11, 1.5, 0.01, 0.03, 255.0


def quantise(x):
    """tgsr_to_uint8's rule on a float32 array: fp32 add, fp32 multiply, clip, round half to even."""
    x = np.asarray(x, dtype=np.float32)
    t = (x + np.float32(1.0)) * np.float32(127.5)
    assert t.dtype == np.float32
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.round(np.maximum(np.float32(0), np.minimum(np.float32(255), t))).astype(np.uint8)


def loader_normalise(u8):
    """The data loader's ToTensor + Normalize(0.5, 0.5) in fp32: (u / 255 - 0.5) / 0.5."""
    f = np.asarray(u8).astype(np.float32) / np.float32(255)
    return (f - np.float32(0.5)) / np.float32(0.5)


def as_u8(img):
    img = np.asarray(img)
    return img if img.dtype == np.uint8 else quantise(img)


def rgb2y(u8):
    """[..., 3, H, W] uint8 -> [..., H, W] uint8: f = fp32(u) / fp32(255); in fp64, left to right,
    f_r (65.481 / 255) + f_g (128.553 / 255) + f_b (24.966 / 255) + 16 / 255; byte = trunc(y 255 + 0.5)."""
    f = np.asarray(u8).astype(np.float32) / np.float32(255)
    assert f.dtype == np.float32
    c = np.array([65.481, 128.553, 24.966], dtype=np.float64) / 255.0
    r, g, b = (f[..., k, :, :].astype(np.float64) for k in range(3))
    y = r * c[0] + g * c[1] + b * c[2]
    y = y + 16 / 255.0
    return np.uint8(y * 255 + 0.5)


def all_triples():
    """The 4096 x 4096 RGB image whose pixel index i enumerates every triple: (r, g, b) = (i >> 16, (i >> 8) & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)]).reshape(3, 4096, 4096)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def shaved(a, shave):
    return a[..., shave:a.shape[-2] - shave, shave:a.shape[-1] - shave] if shave else a


def sse(a, b):
    """Exact integer sum of squared differences of two uint8 arrays."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def window():
    g = np.exp(-((np.arange(WINDOW) - WINDOW // 2) ** 2) / (2.0 * SIGMA * SIGMA))
    w = np.outer(g, g)
    return w / w.sum()


def ssim_sum(ya, yb):
    """Sum of the SSIM map of two [H, W] uint8 images: the 2-D window applied directly ('valid'), fp64."""
    w = window()
    a, b = ya.astype(np.float64), yb.astype(np.float64)
    view = np.lib.stride_tricks.sliding_window_view

    def filt(m):
        return np.einsum("ijkl,kl->ij", view(m, (WINDOW, WINDOW)), w, optimize=True)
    mu_a, mu_b = filt(a), filt(b)
    va, vb, cab = filt(a * a) - mu_a * mu_a, filt(b * b) - mu_b * mu_b, filt(a * b) - mu_a * mu_b
    c1, c2 = (K1 * PEAK) ** 2, (K2 * PEAK) ** 2
    m = ((2 * mu_a * mu_b + c1) * (2 * cab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (va + vb + c2))
    return float(m.sum()), m.size


def rows(sr, hr, shave=0):
    """What tgsr::sr_metrics returns for [B, 3, H, W] inputs (float32 or uint8 each): ([B] int SSE RGB, [B] int SSE Y,
    [B] float64 SSIM sums) and the counts (pixels, windows) of the crop."""
    a, b = shaved(as_u8(sr), shave), shaved(as_u8(hr), shave)
    ya, yb = rgb2y(a), rgb2y(b)
    s_rgb = [sse(a[i], b[i]) for i in range(a.shape[0])]
    s_y = [sse(ya[i], yb[i]) for i in range(a.shape[0])]
    ss = [ssim_sum(ya[i], yb[i]) for i in range(a.shape[0])]
    return s_rgb, s_y, [s[0] for s in ss], (a.shape[-2] * a.shape[-1], ss[0][1])


def check_rows(got, sr, hr, shave=0, ssim_tol=1e-9):
    """Assert a [B, 3] float64 result of the kernels against the model: the SSEs exact, the MEAN SSIM within `ssim_tol` (a
    window statistic is a sum of 121 terms <= 65 025 in fp64, absolute error <~ 1e-9 against denominators >= C2 = 58.5; both
    sides are fp64 and differ in summation order only).  Returns the largest SSIM deviation seen."""
    got = np.asarray(got)
    s_rgb, s_y, ss, (pixels, windows) = rows(sr, hr, shave)
    assert got.dtype == np.float64 and got.shape == (len(s_rgb), 3)
    worst = 0.0
    for i in range(len(s_rgb)):
        assert got[i, 0] == s_rgb[i] and float(got[i, 0]).is_integer(), (i, got[i, 0], s_rgb[i])
        assert got[i, 1] == s_y[i] and float(got[i, 1]).is_integer(), (i, got[i, 1], s_y[i])
        dev = abs(got[i, 2] / windows - ss[i] / windows)
        worst = max(worst, dev)
        assert dev <= ssim_tol, (i, got[i, 2] / windows, ss[i] / windows)
    return worst
