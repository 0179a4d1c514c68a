#!/usr/bin/env python3
"""Generate tests/golden/attn_losses.npz: the reference's three attention-guided objectives on seeded inputs (CPU, build
container only).

TEST INFRASTRUCTURE like make_golden.py, whose stubs (`_load_ref`: `.cuda()` an identity, `server = 1`) and plain-torch
discriminators it uses: the reference is imported and its `weight_MSE` (miscc/losses.py:792-804), `words_reweight_loss` (:137-232)
and `generator_re_weight_loss` (:318-350) are called; nothing of the reference is copied.  Stored: inputs, outputs and gradients.

  wmse.*   three scales, B = 2, T = 5, maps 3x5 / 6x10 / 5x7 under images at r = 2 (the third is 10 x 14: no multiple of 4);
  wmse1.*  one scale at r = 1 (map and image 4 x 6);
           images as the uint8 codes k of x = k / 127.5 - 1 (as gan_losses.npz stores them); the maps are softmaxed over T and
           hold no tie (asserted), so the argmax the map gradient goes to is decided by the data;
  wrw.*    words_reweight_loss at B = 3, T = 6, lengths 6 / 5 / 3 (thresholds 2/3, 4/5, 4/3: the 3-word caption's confidences
           are all zero), maps 8 x 8, nef 32 and 17 x 17 regions as in gan_losses.npz, with class ids and without; the region
           features as the int8 codes k of x = k / 4 (a few bits each: the file stays small); gradients are stored sub-sampled.  The script ASSERTS what the product's form relies on: the result equals
           the reference's words_loss on words_emb * conf exactly, in value and in both gradients;
  grw.*    generator_re_weight_loss on the discriminators, stub encoder, fake images, words and sentence codes of
           gan_losses.npz (read from that file, not stored again) and a new [3, 7, 8, 8] attention map.

    python tests/golden/make_attn_losses_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402


def _img(gen, *shape):
    k = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    return k, k.float() / 127.5 - 1.0


def _maps(gen, sharp, *shape):
    a = torch.softmax(sharp * torch.randn(*shape, generator=gen), dim=1)
    top = a.topk(2, dim=1)[0]
    assert float((top[:, 0] - top[:, 1]).min()) > 0, "a tie between two words of one map pixel"
    return a


def _wmse(losses, out, name, gen, B, T, sizes, r):
    fake, label, att = [], [], []
    for i, (h, w) in enumerate(sizes):
        kf, f = _img(gen, B, 3, r * h, r * w)
        kl, l = _img(gen, B, 3, r * h, r * w)
        a = _maps(gen, 2.0, B, T, h, w)
        out["%s.fake%d.u8" % (name, i)], out["%s.label%d.u8" % (name, i)], out["%s.att%d" % (name, i)] = G._np(kf), G._np(kl), G._np(a)
        fake.append(f.requires_grad_(True))
        label.append(l.requires_grad_(True))
        att.append(a.requires_grad_(True))
    loss, wlast = losses.weight_MSE(fake, label, att)
    grads = torch.autograd.grad(loss, fake + label + att)
    n = len(sizes)
    out[name + ".loss"], out[name + ".wlast"] = G._np(loss), G._np(wlast)
    for i in range(n):
        assert torch.equal(grads[n + i], -grads[i])                       # d_label = -d_fake: stored once
        out["%s.g_fake%d" % (name, i)], out["%s.g_att%d" % (name, i)] = G._np(grads[i]), G._np(grads[2 * n + i])
        assert int((grads[2 * n + i] != 0).sum(1).max()) == 1           # one word per map pixel receives the gradient


def _wrw(losses, out, gen):
    B, T, nef, lens = 3, 6, 32, [6, 5, 3]
    k = (torch.randn(B, nef, 17, 17, generator=gen) * 4).round().clamp(-127, 127).to(torch.int8)
    words = torch.randn(B, nef, T, generator=gen)
    att = _maps(gen, 8.0, B, T, 8, 8)
    out["wrw.feats.i8"], out["wrw.words"], out["wrw.attn"] = G._np(k), G._np(words), G._np(att)
    out["wrw.cap_lens"], out["wrw.class_ids"] = np.asarray(lens, np.int64), np.array([0, 1, 1])
    labels, cap_lens = torch.arange(B), torch.tensor(lens)
    conf = torch.zeros(B, T)
    for i, n in enumerate(lens):
        for j in range(n):
            conf[i, j] = (att[i, j] * (att[i, j] > (2. * (2. / float(n)))).float()).sum()
    out["wrw.conf"] = G._np(conf)
    assert float(conf[0].min()) > 0 and float(conf[1, :5].min()) > 0 and float(conf[2].abs().max()) == 0, conf
    for tag, cls in (("cls", out["wrw.class_ids"]), ("nocls", None)):
        feats, w = (k.float() / 4.0).requires_grad_(True), words.clone().requires_grad_(True)
        l0, l1, maps = losses.words_reweight_loss(feats, w, labels, cap_lens, cls, B, att)
        gf, gw = torch.autograd.grad(l0 + l1, [feats, w])
        assert bool(torch.isfinite(l0)) and bool(torch.isfinite(l1)) and float(gw[2].abs().max()) == 0
        # the identity the product's form rests on: words_loss on the scaled words, exactly
        f2, w2 = (k.float() / 4.0).requires_grad_(True), words.clone().requires_grad_(True)
        m0, m1, _ = losses.words_loss(f2, w2 * conf[:, None, :], labels, cap_lens, cls, B)
        gf2, gw2 = torch.autograd.grad(m0 + m1, [f2, w2])
        assert torch.equal(l0, m0) and torch.equal(l1, m1) and torch.equal(gf, gf2) and torch.equal(gw, gw2)
        out["wrw.%s.w0" % tag], out["wrw.%s.w1" % tag], out["wrw.%s.g_words" % tag] = G._np(l0), G._np(l1), G._np(gw)
        out["wrw.%s.g_feats.sub16" % tag] = G._np(gf)[:, ::16]
        if cls is not None:
            for i, m in enumerate(maps):
                out["wrw.att_map%d.sub2" % i] = G._np(m).reshape(1, m.shape[1], -1)[:, :, ::2]
    print("wrw: conf", conf.tolist())


def _grw(cfg, losses, out, gen):
    g = dict(np.load(os.path.join(G.OUT, "gan_losses.npz")))
    cfg.TRAIN.SMOOTH.LAMBDA = float(g["lambda"])
    ndf, nef = int(g["ndf"]), int(g["nef"])
    T = lambda key: torch.from_numpy(np.asarray(g[key]))                                  # noqa: E731
    ds = []
    for k in range(2):
        d = G._plain_d_net(ndf, nef, k, torch.Generator().manual_seed(0))
        d.load_state_dict({n[len("D%d." % k):]: T(n) for n in g if n.startswith("D%d." % k)}, strict=True)
        ds.append(d.train())
    ew, eb, pw, pb = (T("enc." + n) for n in ("f.weight", "f.bias", "p.weight", "p.bias"))
    F = torch.nn.functional
    enc = lambda x: (F.conv2d(F.adaptive_avg_pool2d(x, 17), ew, eb), F.linear(x.mean((2, 3)), pw, pb))   # noqa: E731
    fake = [(T("fake%d.u8" % k).float() / 127.5 - 1.0).requires_grad_(True) for k in range(2)]
    sent, words = T("sent").requires_grad_(True), T("words").requires_grad_(True)
    B = sent.shape[0]
    attn = _maps(gen, 8.0, B, words.shape[2], 8, 8)
    out["grw.attn"] = G._np(attn)
    rl, ml = torch.ones(B), torch.arange(B)
    errG, logs = losses.generator_re_weight_loss(ds, enc, fake, rl, words, sent, ml, T("cap_lens"), g["class_ids"], attn=attn)
    gr = torch.autograd.grad(errG, fake + [sent, words])
    out["grw.errG"], out["grw.logs"] = G._np(errG), np.array(logs)
    out["grw.gG.fake0.sub8"], out["grw.gG.fake1.sub16"] = G._np(gr[0])[:, :, ::8, ::8], G._np(gr[1])[:, :, ::16, ::16]
    out["grw.gG.sent"], out["grw.gG.words"] = G._np(gr[2]), G._np(gr[3])
    errG2, _ = losses.generator_re_weight_loss(ds, enc, [f.detach() for f in fake], rl, words, sent, ml, T("cap_lens"), None,
                                               w=0.5, s=2.0, g=3.0, attn=attn)
    out["grw.errG.nocls.w05.s2.g3"] = G._np(errG2)
    print("grw:", logs)


def main():
    cfg, _GA, _util, _model, losses = G._load_ref(ngf=32, nef=32)
    out = {"gamma": np.array([cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3], np.float32)}
    gen = torch.Generator().manual_seed(2025)
    torch.manual_seed(2025)
    _wmse(losses, out, "wmse", gen, 2, 5, [(3, 5), (6, 10), (5, 7)], 2)
    _wmse(losses, out, "wmse1", gen, 2, 5, [(4, 6)], 1)
    _wrw(losses, out, gen)
    _grw(cfg, losses, out, gen)
    path = os.path.join(G.OUT, "attn_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d KB)" % (path, len(out), os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
