#!/usr/bin/env python3
"""us per call of the generators' fp32 conv3x3 layer shapes at batch 16, each on the form ops.conv3x3_form routes it to, through
ops._conv3x3 (validation, plan, launch): ResBlock convolutions, stems, upBlocks at 32^2 / 64^2 / 128^2 and the training forward's
statistics entries.  1000 back-to-back calls between two events: the small layers are bound by the host, the large ones by the kernel.
The working directory decides the tree (and so the library) that is measured: run two checkouts alternately to compare host code.
   python tools/exp_conv_calls.py            (on the GPU box, from the root of the tree to measure)"""
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from tgsr_amd import ops

dev, B = "cuda", 16
torch.manual_seed(0)
LAYERS = [  # name, form, cin, cout, H(=W), glu, residual
    ("GL res c1 64->128 glu", None, 64, 128, 0, 1, 0), ("GL res c2 64->64 +res", None, 64, 64, 0, 0, 1),
    ("GH res c1 32->64 glu", None, 32, 64, 0, 1, 0), ("GH res c2 32->32 +res", None, 32, 32, 0, 0, 1),
    ("stem 3->64 glu", None, 3, 64, 0, 1, 0)]
UPS = [("GL up 64->128 glu", 64, 128), ("GH up 32->64 glu", 32, 64)]


def timeit(f, n=1000):
    for _ in range(10):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


for name, _f, cin, cout, _h, glu, res in LAYERS:
    for r in (32, 64, 128):
        x = torch.randn(B, cin, r, r, device=dev)
        w = torch.randn(cout, cin, 3, 3, device=dev) / (3 * cin ** 0.5)
        co = cout // 2 if glu else cout
        out = torch.empty(B, co, r, r, device=dev)
        resid = torch.randn(B, co, r, r, device=dev) if res else None
        scale, shift = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
        form = ops.conv3x3_form(x, cout, False, bool(glu), out, resid)
        pack = ops.pack_weight(form, w, glu=bool(glu))
        t = timeit(lambda: ops._conv3x3(form, x, pack, cout, scale, shift, bool(glu), False, resid, out))
        print("CALL %-24s %4d^2 %-8s %8.2f us" % (name, r, form, t), flush=True)
for name, cin, cout in UPS:
    for r in (32, 64, 128):
        x = torch.randn(B, cin, r, r, device=dev)
        w = torch.randn(cout, cin, 3, 3, device=dev) / (3 * cin ** 0.5)
        out = torch.empty(B, cout // 2, 2 * r, 2 * r, device=dev)
        scale, shift = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
        form = ops.conv3x3_form(x, cout, True, True, out, None)
        pack = ops.pack_weight(form, w, glu=True) if form != "upconv" else ops.pack_upconv_weight(w)
        t = timeit(lambda: ops._conv3x3(form, x, pack, cout, scale, shift, True, True, None, out))
        print("CALL %-24s %4d^2 %-8s %8.2f us" % (name, r, form, t), flush=True)
# the training forward's statistics entries
for cin, cout, r in ((64, 128, 32), (64, 128, 128), (32, 32, 64)):
    x = torch.randn(B, cin, r, r, device=dev)
    w = torch.randn(cout, cin, 3, 3, device=dev) / (3 * cin ** 0.5)
    out = torch.empty(B, cout, r, r, device=dev)
    form = ops.conv3x3_form(x, cout, False, False, out, None, True, True)
    if ops.FORMS[form].stats is None:
        continue
    pack = ops.pack_weight(form, w, glu=False)
    t = timeit(lambda: ops._conv3x3(form, x, pack, cout, None, None, False, False, None, out, stats=True))
    print("CALL %-24s %4d^2 %-8s %8.2f us" % ("stats %d->%d" % (cin, cout), r, form, t), flush=True)
