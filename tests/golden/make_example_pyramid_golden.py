#!/usr/bin/env python3
"""Golden vectors for the arbitrary-size example path: runs the reference's own `datasets.get_imgsexampletestblur`
(datasets.py:236-278) on one small generated image (83 x 117: neither side a multiple of the scale, so the crop to 80 x 112 is
exercised) and stores the input and the four lists in tests/golden/example_pyramid.npz.
TEST INFRASTRUCTURE - runs only where the reference exists (TGSR_REFERENCE, the build container) and Pillow is installed.

The reference's function opens a file: the image goes through a temporary PNG (lossless).  datasets.py's module-level
imports that are not installed are stubbed exactly as make_io_golden.py does (its `_stubs`): the arithmetic that the
fixture pins is Pillow's.
"""
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_io_golden import _stubs  # noqa: E402


def make_image(h=83, w=117, seed=11):
    """A generated photograph-like image: smooth colour gradients + a few hard edges + noise (so that the resize, the
    blur's borders and the rounding all have something to get wrong)."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 100 * np.sin(x / 9.0 + y / 17.0), 127 + 90 * np.cos(y / 7.0 - x / 23.0), 40 + 1.5 * x + 0.5 * y], -1)
    img[20:45, 30:70] = (250, 10, 128)
    img[60:, :25] = (5, 240, 30)
    img += g.normal(0, 12, img.shape)
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def main():
    tr = _stubs()
    import datasets                                  # the reference's datasets.py
    cfg = types.SimpleNamespace(GAN=types.SimpleNamespace(B_DCGAN=False), TREE=types.SimpleNamespace(BRANCH_NUM=4))
    norm = tr.Compose([tr.ToTensor(), tr.Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])
    hr = make_image()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "example.png")
        Image.fromarray(hr).save(path)
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), hr)
        ret, bic, retb, bicb = datasets.get_imgsexampletestblur(path, scale=8, transform=None, normalize=norm, cfg=cfg)
    out = {"hr_u8": hr.transpose(2, 0, 1).copy(), "scale": np.array(8)}

    def u8(t):
        return np.round((t.numpy() * 0.5 + 0.5) * 255).astype(np.uint8)
    for name, lst in (("ret", ret), ("bic", bic), ("retb", retb), ("bicb", bicb)):
        assert len(lst) == 4
        for i, t in enumerate(lst):
            out["%s%d_u8" % (name, i)] = u8(t)
    out["bic0_f32"] = bic[0].numpy()                 # pins the float normalisation
    out["retb3_f32"] = retb[3].numpy()
    np.savez_compressed(os.path.join(OUT, "example_pyramid.npz"), **out)
    print("example_pyramid.npz", len(out), "arrays", [tuple(t.shape) for t in ret])


if __name__ == "__main__":
    main()
