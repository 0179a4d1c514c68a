#!/usr/bin/env python3
"""Golden results for the image-quality metrics: runs the reference's own `rgb2y` and `psnr` (trainer_objective.py:168-181) on the
image pairs of the committed io_pyramid.npz and on every RGB triple, and stores what they return in tests/golden/sr_metrics.npz.
TEST INFRASTRUCTURE - runs only where the reference exists (TGSR_REFERENCE, default /root/reference).

trainer_objective.py imports cv2 and skimage at module level; neither is installed here and neither takes part in the two
functions.  The file is parsed, the two function definitions alone are compiled (with numpy as `np`, their only global) and
called; nothing of their text is stored.
"""
import ast
import os
import sys

import numpy as np

REF = os.environ.get("TGSR_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import metrics_model as M  # noqa: E402


def reference_functions(names=("rgb2y", "psnr")):
    path = os.path.join(REF, "trainer_objective.py")
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in tree.body) == sorted(names)
    ns = {"np": np}
    exec(compile(tree, path, "exec"), ns)
    return [ns[n] for n in names]


def main():
    rgb2y, psnr = reference_functions()
    z = np.load(os.path.join(OUT, "io_pyramid.npz"))
    out = {}
    for k in (1, 2, 3):
        a, b = z["ret%d_u8" % k], z["bic%d_u8" % k]                       # [3, H, W]
        ya, yb = rgb2y(a.transpose(1, 2, 0)), rgb2y(b.transpose(1, 2, 0))  # the reference works on [H, W, 3]
        out["ret%d_y" % k], out["bic%d_y" % k] = ya, yb
        out["pair%d_rgb" % k] = np.array(psnr(a, b), dtype=np.float64)     # (psnr, rmse)
        out["pair%d_y" % k] = np.array(psnr(ya, yb), dtype=np.float64)
        print("pair %d: RGB %.4f dB, Y %.4f dB" % (k, out["pair%d_rgb" % k][0], out["pair%d_y" % k][0]))
    y = rgb2y(M.all_triples().transpose(1, 2, 0))
    assert y.shape == (4096, 4096) and y.dtype == np.uint8
    out["triples_y_sha256"] = np.array(M.sha256(y))
    out["triples_y_range"] = np.array([int(y.min()), int(y.max())])
    np.savez_compressed(os.path.join(OUT, "sr_metrics.npz"), **out)
    print("sr_metrics.npz", len(out), "arrays; Y range", out["triples_y_range"], out["triples_y_sha256"])


if __name__ == "__main__":
    main()
