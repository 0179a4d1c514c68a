"""Text-image retrieval on the device: does an image belong to its caption?

The two similarities are the reference's (`sent_similarity`, `words_similarity`, miscc/losses.py:234-287), scored by the gallery
kernels of csrc/tgsr_retrieval.hip (torch.ops.tgsr.damsm_gallery / sent_gallery) for N images against a candidate list of captions
each; the rank of the true caption comes from tgsr::retrieval_ranks (a count, no sort).  Two protocols:

  r_precision       the AttnGAN family's metric for text-conditioned generators: every image is scored against its own caption and
                    K - 1 mismatched ones (`sample_candidates`); R-precision is the share of images whose own caption ranks first.
  retrieval_scores  the full N x N gallery in both directions (image -> text and text -> image), recall@k and the median rank: what
                    one picks a DAMSM checkpoint by.

Everything stays on the device until one synchronisation at the end of each function.  Ranks are 0-based (0 = the true partner
is on top; ties go to the lower column, as in a stable descending sort); `median_rank` is reported 1-based, as retrieval papers do.
"""
import numpy as np
import torch

from . import custom_ops as C
from .miscc.config import cfg

MODES = ("sent", "words")


def sample_candidates(class_ids, n_candidates=100, generator=None):
    """The R-precision candidate table: int32 [N, K] on the CPU, K = n_candidates.  Row n holds n itself in column 0 (the image's
    own caption), then K - 1 captions drawn without replacement from those whose class id differs from class_ids[n]; where fewer
    exist, the row ends in -1 (empty slots, which the gallery kernels score -inf).  Deterministic under `generator`'s seed."""
    ids = np.asarray(class_ids.cpu() if torch.is_tensor(class_ids) else class_ids).reshape(-1)
    N, K = ids.shape[0], int(n_candidates)
    if N < 1 or K < 1:
        raise ValueError("sample_candidates: %d items, %d candidates" % (N, K))
    table = torch.full((N, K), -1, dtype=torch.int32)
    table[:, 0] = torch.arange(N, dtype=torch.int32)
    for n in range(N):
        pool = torch.from_numpy(np.flatnonzero(ids != ids[n]).astype(np.int32))
        take = min(K - 1, pool.numel())
        if take:
            table[n, 1:1 + take] = pool[torch.randperm(pool.numel(), generator=generator)[:take]]
    return table


class Gallery:
    """The items of many batches for ONE gallery: the batches are kept as they come (no copy, no launch, no synchronisation) and
    concatenated once.  What DAMSMTrainer.evaluate_retrieval and SRTrainer.evaluate(r_precision=) collect."""

    def __init__(self):
        self.regions, self.codes, self.words, self.sents, self.lens, self.class_ids = [], [], [], [], [], []

    def __len__(self):
        return len(self.lens)

    def add(self, regions, codes, words_emb, sent_emb, cap_lens, take=None, class_ids=None):
        """One batch: region features, image codes, word and sentence embeddings, caption lengths (a tensor or a list; kept as
        ints) and - for sample_candidates - class ids.  `take`: only the first `take` items of the batch."""
        for held, t in zip((self.regions, self.codes, self.words, self.sents), (regions, codes, words_emb, sent_emb)):
            held.append(t if take is None else t[:take])
        for held, v in ((self.lens, cap_lens), (self.class_ids, class_ids)):
            if v is not None:
                held += [int(i) for i in (v.tolist() if torch.is_tensor(v) else v)][:take]

    def cat(self):
        """(regions, codes, words_emb, sent_emb, cap_lens): what r_precision and retrieval_scores take.  Batches may differ in
        their longest caption: the word axis is zero-padded to the longest."""
        Tw = max(w.shape[2] for w in self.words)
        words = [w if w.shape[2] == Tw else torch.nn.functional.pad(w, (0, Tw - w.shape[2])) for w in self.words]
        return torch.cat(self.regions), torch.cat(self.codes), torch.cat(words), torch.cat(self.sents), self.lens


def _similarity(mode,regions, codes, words_emb, sent_emb, cap_lens, cand):
    sm = cfg.TRAIN.SMOOTH
    if mode == "sent":
        return C.sent_gallery(codes, sent_emb, 1e-8, float(sm.GAMMA3), cand)
    if mode == "words":
        lens = cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens
        return C.damsm_gallery(regions, words_emb, [int(v) for v in lens], float(sm.GAMMA1), float(sm.GAMMA2), cand)
    raise ValueError("mode must be one of %s, got %r" % (MODES, mode))


def _recalls(ranks, ks):
    """[len(ks) + 1] float64 on the device: the share of ranks below each k, then the median of the 1-based ranks."""
    r = ranks.to(torch.float64)
    return torch.stack([(ranks < int(k)).to(torch.float64).mean() for k in ks] + [r.median() + 1])


@torch.no_grad()
def r_precision(regions, codes, words_emb, sent_emb, cap_lens, cand, mode="sent", ks=(1,)):
    """R-precision of N images against the candidate table `cand` (int [N, K], column 0 = the image's own caption: the table of
    `sample_candidates`; captions are rows of words_emb [M,ndf,Tw] / sent_emb [M,ndf] with lengths cap_lens).  mode "sent" scores
    codes [N,ndf] by the sentence cosine, "words" scores regions [N,ndf,ih,iw] by the word-region attention.
    Returns {"ranks": int32 [N] on the device (0 = the own caption is on top), "r_precision": the share of rank 0,
    "recall": {k: the share of ranks < k}}.  One synchronisation, at the end."""
    sim = _similarity(mode, regions, codes, words_emb, sent_emb, cap_lens, cand)
    ranks = C.retrieval_ranks(sim, torch.zeros(sim.shape[0], dtype=torch.int32, device=sim.device))
    vals = _recalls(ranks, (1,) + tuple(ks)).tolist()                      # the synchronisation
    return {"ranks": ranks, "r_precision": vals[0], "recall": {int(k): v for k, v in zip(ks, vals[1:])}}


@torch.no_grad()
def retrieval_scores(regions, codes, words_emb, sent_emb, cap_lens, ks=(1, 5, 10)):
    """The full N x N gallery (item n = image n and caption n), both similarities, both directions:
    {"sent" | "words": {"i2t" | "t2i": {"ranks": int32 [N] on the device, "recall": {k: float}, "median_rank": float (1-based)}}}.
    Text -> image ranks come from the transposed similarity matrix.  One synchronisation, at the end."""
    N = codes.shape[0]
    if sent_emb.shape[0] != N or words_emb.shape[0] != N or regions.shape[0] != N:
        raise ValueError("retrieval_scores: %d images against %d captions - item n must be image n and caption n"
                         % (N, sent_emb.shape[0]))
    target = torch.arange(N, dtype=torch.int32, device=codes.device)
    ranks, stats = {}, []
    for mode in MODES:
        sim = _similarity(mode, regions, codes, words_emb, sent_emb, cap_lens, None)
        for way, s in (("i2t", sim), ("t2i", sim.t().contiguous())):
            ranks[mode, way] = C.retrieval_ranks(s, target)
            stats.append(_recalls(ranks[mode, way], ks))
    vals = torch.stack(stats).tolist()                                     # the synchronisation
    out = {mode: {} for mode in MODES}
    for (mode, way), row in zip(ranks, vals):
        out[mode][way] = {"ranks": ranks[mode, way], "recall": {int(k): v for k, v in zip(ks, row)}, "median_rank": row[-1]}
    return out
