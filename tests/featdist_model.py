"""A numpy fp64 model of the distribution distances (include/tgsr_hip.h, tgsr_amd/featdist.py): the moments of a feature set, its
mean and covariance, the Frechet distance in its symmetric eigh form and KID from explicit kernel matrices.  Uses no library code;
every expected value of tests/test_featdist_host.py and tests/test_hip_featdist.py comes from here."""
import numpy as np

U = 2.0 ** -53          # the unit roundoff of fp64


def features(n, D, seed, which=0):
    """ReLU-pooled-like float32 features: max(0.5 N(0,1) + 0.3, 0) (which = 0) or max(0.6 N(0,1) + 0.35, 0) (which = 1)."""
    rng = np.random.RandomState(seed)
    s, b = ((0.5, 0.3), (0.6, 0.35))[which]
    return np.maximum(s * rng.standard_normal((n, D)) + b, 0.0).astype(np.float32)


def moments(x):
    """(n, sum [D], outer [D, D]) of float32 rows, accumulated row by row in fp64 (each product of two widened values is exact)."""
    X = np.asarray(x, dtype=np.float64)
    return X.shape[0], X.sum(0), X.T @ X


def moment_bounds(x):
    """Per element, the bound on |got - ref| between two fp64 sums of the same n exact terms in any order: 2 n u sum |term|, for
    `sum` and for `outer`."""
    A = np.abs(np.asarray(x, dtype=np.float64))
    n = A.shape[0]
    return 2 * n * U * A.sum(0), 2 * n * U * (A.T @ A)


def mean_cov(n, s, outer):
    mu = s / n
    return mu, (outer - n * np.outer(mu, mu)) / (n - 1)


def frechet(mc1, mc2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), the last term as the sum of sqrt(max(eigvalsh(sym(A^T S2 A)), 0)) with
    S1 = V diag(w) V^T, A = V diag(sqrt(max(w, 0))).  Not clamped."""
    (m1, c1), (m2, c2) = mc1, mc2
    w, V = np.linalg.eigh(c1)
    A = V * np.sqrt(np.maximum(w, 0.0))
    M = A.T @ c2 @ A
    tr = np.sqrt(np.maximum(np.linalg.eigvalsh((M + M.T) / 2), 0.0)).sum()
    d = m1 - m2
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * tr)


def frechet_of(x, y):
    return frechet(mean_cov(*moments(x)), mean_cov(*moments(y)))


def poly_kernel(a, b):
    A, B = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (A @ B.T / A.shape[1] + 1.0) ** 3


def mmd_sums(x, y, ix, iy):
    """([S, 3] sums, [S, 3] sums of |k| over the same index sets): per subset sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j),
    sum_{i, j} k(x_i, y_j) over POSITIONS i, j of the subset, from the explicit m x m kernel matrices."""
    out, mag = [], []
    for tx, ty in zip(np.asarray(ix), np.asarray(iy)):
        X, Y = x[tx], y[ty]
        off = 1.0 - np.eye(len(tx))
        ks = (poly_kernel(X, X) * off, poly_kernel(Y, Y) * off, poly_kernel(X, Y))
        out.append([k.sum() for k in ks])
        mag.append([np.abs(k).sum() for k in ks])
    return np.array(out), np.array(mag)


def mmd_bound(mag, m, D):
    """|got - ref| <= 4 (D + m^2) u sum |k| per output: a fp64 dot of D terms, a cube and a sum of m^2 terms, on both sides."""
    return 4.0 * (D + m * m) * U * mag


def kid(x, y, ix, iy):
    """{"mean", "std", "per_subset"}: per subset sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2; std in the population form."""
    s, _ = mmd_sums(x, y, ix, iy)
    m = np.asarray(ix).shape[1]
    per = s[:, 0] / (m * (m - 1.0)) + s[:, 1] / (m * (m - 1.0)) - 2.0 * s[:, 2] / (float(m) * m)
    return {"mean": float(per.mean()), "std": float(per.std()), "per_subset": per}
