#!/usr/bin/env python3
"""Generate tests/golden/retrieval.npz: the reference's two retrieval similarities on seeded inputs (CPU, build container only).

TEST INFRASTRUCTURE like make_golden.py, whose stubs it uses: the reference is imported and its `sent_similarity`
(miscc/losses.py:234-250) and `words_similarity` (:251-287) are called, in fp32 and again on the same inputs in fp64; nothing of
the reference is copied.  A rectangular case (N images, M captions) is made by calling `words_similarity` on square batches of
max(N, M) - images or captions repeated to fill - and keeping the rows and columns wanted: entry (j, i) depends on image j and
caption i only.

Cases `c0`..`c3` are the gallery kernel's shapes (one region, 33 / 289 / 320 regions, one word, the lengths {1, 16, 17, 32}); the
feature width is 32 where S = 289 so that the file stays at a few hundred KB.  Case `e2e` is a 16-item gallery with class ids and
an R-precision candidate table; for it this script ASSERTS on the fp64 run that every target score is at least 1e-3 away from
every other candidate's in its row (about 14 x the test tolerance at |sim| = 5) - on random data gaps of 2e-4 do occur - and picks
the first seed for which that holds, so that the ranks the tests compare are decided by the data, not by rounding.

    python tests/golden/make_retrieval_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402

GAP = 1e-3


def _similarities(losses, regions, words, lens, codes, sents, dtype):
    """(words_similarity [N, M], sent_similarity [N, M]) of the reference on N images and M captions."""
    N, M = regions.shape[0], words.shape[0]
    b = max(N, M)
    reg = torch.cat([regions, regions[:1].expand(b - N, -1, -1, -1)]).to(dtype).contiguous()
    wrd = torch.cat([words, words[:1].expand(b - M, -1, -1)]).to(dtype).contiguous()
    ln = torch.tensor(list(lens) + [lens[0]] * (b - M), dtype=torch.int64)
    w = losses.words_similarity(reg, wrd, ln, b)[:N, :M]
    s = losses.sent_similarity(codes.to(dtype), sents.to(dtype))
    return G._np(w), G._np(s)


def _case(losses, out, name, gen, N, M, ndf, ih, iw, Tw, lens, scale=1.0):
    regions = torch.randn(N, ndf, ih, iw, generator=gen) * scale
    words = torch.randn(M, ndf, Tw, generator=gen) * scale
    codes, sents = torch.randn(N, ndf, generator=gen), torch.randn(M, ndf, generator=gen)
    w32, s32 = _similarities(losses, regions, words, lens, codes, sents, torch.float32)
    w64, s64 = _similarities(losses, regions, words, lens, codes, sents, torch.float64)
    assert w32.dtype == np.float32 and w64.dtype == np.float64 and w32.shape == (N, M) and s32.shape == (N, M)
    for key, v in (("regions", regions), ("words", words), ("codes", codes), ("sents", sents)):
        out["%s.%s" % (name, key)] = G._np(v)
    out[name + ".lens"] = np.asarray(lens, dtype=np.int32)
    out[name + ".words_sim32"], out[name + ".words_sim64"] = w32, w64
    out[name + ".sent_sim32"], out[name + ".sent_sim64"] = s32, s64
    return w64, s64


def _stable_ranks(sim, target):
    """The rank formula of tgsr_retrieval_ranks, restated: position of column target[n] in a stable descending sort of row n."""
    ranks = np.empty(sim.shape[0], dtype=np.int32)
    for n, t in enumerate(target):
        row = sim[n]
        ranks[n] = np.sum(row > row[t]) + np.sum(row[:t] == row[t])
    return ranks


def _gap(sim, target):
    """Smallest |sim[n][target[n]] - sim[n][k]| over k != target[n] (finite entries)."""
    g = np.inf
    for n, t in enumerate(target):
        d = np.abs(np.delete(sim[n], t) - sim[n][t])
        g = min(g, d[np.isfinite(d)].min())
    return g


def _e2e(losses, out):
    N, ndf, ih, iw, Tw, K = 16, 32, 5, 5, 18, 6
    for seed in range(100, 200):
        gen = torch.Generator().manual_seed(seed)
        lens = torch.randint(1, Tw + 1, (N,), generator=gen).tolist()
        class_ids = torch.randint(1, 5, (N,), generator=gen).tolist()
        class_ids[4:] = [0] * (N - 4)          # a class of twelve: its rows find four captions of other classes, one slot stays empty
        words = torch.randn(N, ndf, Tw, generator=gen)
        sents = torch.randn(N, ndf, generator=gen)
        # an image looks a little like its caption: some of its regions carry the caption's words, its code the sentence
        regions = torch.randn(N, ndf, ih * iw, generator=gen)
        for n in range(N):
            for w in range(lens[n]):
                regions[n, :, (3 * w) % (ih * iw)] += 0.6 * words[n, :, w]
        regions = regions.view(N, ndf, ih, iw).contiguous()
        codes = torch.randn(N, ndf, generator=gen) + 0.5 * sents
        # the candidate table of the R-precision protocol, drawn here with plain numpy (tgsr_amd.retrieval.sample_candidates has
        # its own properties test): column 0 the own caption, then captions of other classes, -1 where there are too few
        rng = np.random.RandomState(seed)
        cand = np.full((N, K), -1, dtype=np.int32)
        for n in range(N):
            pool = [m for m in range(N) if class_ids[m] != class_ids[n]]
            pick = rng.permutation(pool)[:K - 1]
            cand[n, 0] = n
            cand[n, 1:1 + len(pick)] = pick
        w64, s64 = _similarities(losses, regions, words, lens, codes, sents, torch.float64)
        diag, zero = np.arange(N), np.zeros(N, dtype=np.int64)
        gaps = []
        for sim in (w64, s64):
            listed = np.where(cand >= 0, np.take_along_axis(sim, np.maximum(cand, 0).astype(np.int64), 1), -np.inf)
            gaps += [_gap(sim, diag), _gap(sim.T, diag), _gap(listed, zero)]
        if min(gaps) >= GAP:
            break
    else:
        raise SystemExit("no seed separates every target score by %g" % GAP)
    assert min(gaps) >= GAP, gaps
    w32, s32 = _similarities(losses, regions, words, lens, codes, sents, torch.float32)
    for key, v in (("regions", regions), ("words", words), ("codes", codes), ("sents", sents)):
        out["e2e." + key] = G._np(v)
    out["e2e.lens"] = np.asarray(lens, dtype=np.int32)
    out["e2e.class_ids"] = np.asarray(class_ids, dtype=np.int32)
    out["e2e.cand"] = cand
    out["e2e.words_sim32"], out["e2e.words_sim64"], out["e2e.sent_sim32"], out["e2e.sent_sim64"] = w32, w64, s32, s64
    for mode, sim in (("words", w64), ("sent", s64)):
        listed = np.where(cand >= 0, np.take_along_axis(sim, np.maximum(cand, 0).astype(np.int64), 1), -np.inf)
        out["e2e.%s_i2t_ranks" % mode] = _stable_ranks(sim, diag)
        out["e2e.%s_t2i_ranks" % mode] = _stable_ranks(sim.T, diag)
        out["e2e.%s_rp_ranks" % mode] = _stable_ranks(listed, zero)
    out["e2e.seed_gap"] = np.asarray([seed, min(gaps)], dtype=np.float64)
    print("e2e: seed %d, smallest target gap %.3g" % (seed, min(gaps)))


def main():
    cfg, _GA, _util, _model, losses = G._load_ref(nef=32)
    out = {"gammas": np.asarray([cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3], dtype=np.float64)}
    gen = torch.Generator().manual_seed(2024)
    _case(losses, out, "c0", gen, N=3, M=5, ndf=32, ih=3, iw=3, Tw=1, lens=[1] * 5)
    _case(losses, out, "c1", gen, N=4, M=8, ndf=32, ih=17, iw=17, Tw=32, lens=[1, 16, 17, 32, 16, 1, 32, 17], scale=0.5)
    _case(losses, out, "c2", gen, N=3, M=5, ndf=64, ih=3, iw=11, Tw=18, lens=[18, 5, 9, 1, 12], scale=0.5)
    _case(losses, out, "c3", gen, N=2, M=3, ndf=32, ih=16, iw=20, Tw=12, lens=[12, 3, 7], scale=0.5)
    _e2e(losses, out)
    worst = {"words": 0.0, "sent": 0.0}
    for key in out:
        if key.endswith("_sim32"):
            worst[key.split(".")[1].split("_")[0]] = max(worst[key.split(".")[1].split("_")[0]],
                                                         float(np.abs(out[key] - out[key[:-2] + "64"]).max()))
    print("reference fp32 against its fp64 run, largest difference:", worst)
    path = os.path.join(G.OUT, "retrieval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d KB)" % (path, os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
