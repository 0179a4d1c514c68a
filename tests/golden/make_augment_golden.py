#!/usr/bin/env python3
"""Golden vectors for the ragged crop / resize / window / flip launch (tgsr_augment_u8, datasets.DeviceAugment): synthetic
sources put through Pillow itself,

    img.crop((x1, y1, x2, y2)).resize((ow, oh), BILINEAR).crop((left, top, left + S, top + S))   # then mirror if flip

with fixed descriptors, stored with the descriptors and the expected outputs in tests/golden/io_augment.npz.
TEST INFRASTRUCTURE - runs only where Pillow is installed; the tests that read the file need no Pillow.

Sources (H x W, smooth gradients + seeded noise) at S = 32, Resize(int(32 * 76 / 64)) = 38, the smallest shapes at which
the kernel can go wrong:
  0  61 x 83   landscape, down-scale, window at (0, 0)
  1  83 x 61   portrait, down-scale, window at (oh - S, ow - S)
  2  20 x 27   up-scale, flipped
  3  38 x 50   the shorter side already is 38: torchvision's rule keeps BOTH sizes and Pillow skips both passes
  4  37 x 400  -> 38 x 410, window at the far end
  5  400 x 37  -> 410 x 38, window at the far end, flipped
  6  45 x 500  with a CUB-style bounding box whose 0.75-radius square is clamped at three image borders: a 260 x 45 crop
Torchvision's rule keeps the aspect ratio, so it never yields "one axis unchanged" or a reduction on one axis alone; the
kernel takes any (oh, ow), so two more entries with descriptors set by hand cover those paths:
  7  source 3 resized to 38 x 44: the vertical pass is skipped, the horizontal one is not
  8  source 6, columns 4..500, resized to 38 x 32: a 15.5x horizontal reduction, 33 taps
Eval mode (Resize(int(32 * 72 / 64)) = 36 + CenterCrop(32), no flip) for sources 0 and 6 (with its box), and - for the
end-to-end test of SRBatcher((32, 64)) - S = 64 / Resize(76) crops of sources 0, 2, 3 and 6.
The CUB box and the Resize size rule are written out here in the reference's own operations (numpy maximum / minimum on
the bbox, datasets.py:115-123; torchvision's int-size rule as make_io_golden.py has it) and stored as tables for the host
functions crop_box / resized_size.
"""
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
S, SIZE, SIZE_EVAL = 32, int(32 * 76 / 64), int(32 * 72 / 64)
S2, SIZE2 = 64, int(64 * 76 / 64)


def source(g, h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin(x / 5.0 + y / 7.0)]
    a = np.stack(planes, -1) + g.integers(-2, 3, (h, w, 3))
    return np.clip(np.round(a), 0, 255).astype(np.uint8)


def cub_box(bbox, width, height):
    r = int(np.maximum(bbox[2], bbox[3]) * 0.75)
    center_x = int((2 * bbox[0] + bbox[2]) / 2)
    center_y = int((2 * bbox[1] + bbox[3]) / 2)
    y1, y2 = np.maximum(0, center_y - r), np.minimum(height, center_y + r)
    x1, x2 = np.maximum(0, center_x - r), np.minimum(width, center_x + r)
    return int(x1), int(y1), int(x2), int(y2)


def rule(w, h, size):
    return (size, int(size * h / w)) if w <= h else (int(size * w / h), size)          # (ow, oh)


def chain(src, d, s):
    _off, _H, _W, x1, y1, x2, y2, oh, ow, top, left, flip = d
    img = Image.fromarray(src).crop((x1, y1, x2, y2)).resize((ow, oh), Image.BILINEAR).crop((left, top, left + s, top + s))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(img).transpose(2, 0, 1).copy()


def table(srcs, rows):
    """rows: (source index, box, oh, ow, top, left, flip) -> int32 [n, 12] with the offsets of the sources packed in row order."""
    out, off = [], 0
    for i, box, oh, ow, top, left, flip in rows:
        h, w = srcs[i].shape[:2]
        out.append((off, h, w) + tuple(box) + (oh, ow, top, left, flip))
        off += 3 * h * w
    return np.array(out, np.int32)


def main():
    g = np.random.default_rng(20240607)
    shapes = [(61, 83), (83, 61), (20, 27), (38, 50), (37, 400), (400, 37), (45, 500)]
    srcs = [source(g, h, w) for h, w in shapes]
    bbox6 = (300, 5, 240, 30)
    boxes = [(0, 0, w, h) for h, w in shapes]
    boxes[6] = cub_box(bbox6, 500, 45)
    assert boxes[6] == (240, 0, 500, 45)

    def by_rule(i, size, s, where, flip):
        x1, y1, x2, y2 = boxes[i]
        ow, oh = rule(x2 - x1, y2 - y1, size)
        top, left = {"origin": (0, 0), "far": (oh - s, ow - s), "mid": ((oh - s) // 2, (ow - s) // 3),
                     "centre": (int(round((oh - s) / 2.)), int(round((ow - s) / 2.)))}[where]
        return (i, boxes[i], oh, ow, top, left, flip)

    train_rows = [by_rule(0, SIZE, S, "origin", 0), by_rule(1, SIZE, S, "far", 0), by_rule(2, SIZE, S, "mid", 1),
                  by_rule(3, SIZE, S, "mid", 0), by_rule(4, SIZE, S, "far", 0), by_rule(5, SIZE, S, "far", 1),
                  by_rule(6, SIZE, S, "mid", 1),
                  (3, boxes[3], 38, 44, 3, 7, 1),
                  (6, (4, 0, 500, 45), 38, 32, 5, 0, 0)]
    assert train_rows[3][2:4] == (38, 50) and train_rows[4][2:4] == (38, 410) and train_rows[5][2:4] == (410, 38)
    eval_rows = [by_rule(0, SIZE_EVAL, S, "centre", 0), by_rule(6, SIZE_EVAL, S, "centre", 0)]
    e2e_rows = [by_rule(0, SIZE2, S2, "mid", 0), by_rule(2, SIZE2, S2, "far", 1), by_rule(3, SIZE2, S2, "origin", 0),
                by_rule(6, SIZE2, S2, "mid", 1)]
    out = {"pillow_version": np.array(PIL.__version__), "S": np.array(S), "size": np.array(SIZE), "size_eval": np.array(SIZE_EVAL),
           "S_e2e": np.array(S2), "size_e2e": np.array(SIZE2), "n_sources": np.array(len(srcs)), "bbox6": np.array(bbox6)}
    for i, a in enumerate(srcs):
        out["src%d" % i] = a
    for name, rows, s in (("train", train_rows, S), ("eval", eval_rows, S), ("e2e", e2e_rows, S2)):
        t = table(srcs, rows)
        out[name + "_src"] = np.array([r[0] for r in rows])
        out[name + "_table"] = t
        out[name + "_out"] = np.stack([chain(srcs[r[0]], d, s) for r, d in zip(rows, t.tolist())])
    # host-function tables: CUB boxes (x, y, w, h, width, height) -> (x1, y1, x2, y2); (w, h, size) -> (ow, oh)
    bb = [bbox6 + (500, 45), (60, 27, 325, 304, 500, 335), (139, 30, 153, 264, 500, 336), (14, 112, 388, 186, 500, 347),
          (0, 0, 45, 500, 45, 500), (112, 90, 255, 242, 500, 400), (250.5, 100.25, 99.5, 60.0, 375, 500), (3, 2, 1, 1, 8, 8)]
    out["box_cases"] = np.array(bb, np.float64)
    out["box_expected"] = np.array([cub_box(b[:4], b[4], b[5]) for b in bb], np.int32)
    rc = [(w, h, s) for s in (36, 38, 76, 288, 304) for (w, h) in
          ((500, 375), (333, 500), (80, 97), (1999, 1201), (304, 304), (400, 303), (33, 40), (911, 256), (260, 45), (50, 38))]
    out["resize_cases"] = np.array(rc, np.int32)
    out["resize_expected"] = np.array([rule(*c) for c in rc], np.int32)
    path = os.path.join(OUT, "io_augment.npz")
    np.savez_compressed(path, **out)
    print("io_augment.npz", len(out), "arrays,", os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
