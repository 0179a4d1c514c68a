"""Drop-in for the hot-path losses of the reference's miscc/losses.py.

`words_loss` / `sent_loss` (DAMSM, losses.py:21-136) keep the reference's signatures and return tuples; the
per-caption Python loop of words_loss is one launch of the batched DAMSM kernel (tgsr_damsm_words_fwd).  The class
mask, the x gamma3 scale and the two cross entropies act on a [B, B] matrix and stay in torch, like sent_loss's
[B,256]x[256,B] product (a plain library GEMM).  `KL_loss` and `MSE` (losses.py:779-810) are scalar reductions.
Both are differentiable: words_loss through the HIP backward of the DAMSM kernel (tgsr_damsm_words_bwd, autograd.DamsmWords),
sent_loss through torch autograd over its [B, B] matrix.
The objectives that read the generator's word-attention maps - `weight_MSE` (:792-804), `words_reweight_loss` (:137-232),
`generator_re_weight_loss` (:318-350) - run on the kernels of tgsr_attn_losses.hip; their torch compositions, for
CPU tensors and for what the kernels do not take, live here and nowhere else.
The cycle-consistency term `CycleMSE` (:785-790) runs on the kernels of tgsr_cycle_mse.hip, one forward and one
backward launch for a whole pyramid; its torch composition lives here as well.
"""
import contextlib

import numpy as np

import torch
import torch.nn.functional as F

from .. import custom_ops as C
from .. import ops
from .config import cfg


def _func_attention(query, context, gamma1):
    return C.func_attention(query, context, float(gamma1))


def cosine_similarity(x1, x2, dim=1, eps=1e-8):
    """losses.py:12-18: <x1, x2> / max(|x1| |x2|, eps) along `dim`."""
    dot = (x1 * x2).sum(dim)
    scale = (x1.norm(p=2, dim=dim) * x2.norm(p=2, dim=dim)).clamp_min(eps)
    return (dot / scale).squeeze()


def _class_masks(class_ids, batch_size, device):
    """losses.py:25-35 / 75-80: masks[i][j] = (class_ids[j] == class_ids[i]) and i != j."""
    if class_ids is None:
        return None
    ids = np.asarray(class_ids)
    m = ids[None, :] == ids[:, None]
    np.fill_diagonal(m, False)
    return torch.from_numpy(m).to(device)


def _ranking_ce(scores, labels):
    """The two cross entropies of a [B, B] matching matrix (rows = images, columns = captions) - losses.py:56-59."""
    if labels is None:
        return None, None
    return F.cross_entropy(scores, labels), F.cross_entropy(scores.t(), labels)


def sent_loss(cnn_code, rnn_code, labels, class_ids, batch_size, eps=1e-8):
    """losses.py:21-62: gamma3-scaled cosine matrix between the image codes and the sentence codes, same-class pairs
    masked out, cross entropy along both axes."""
    img = cnn_code.reshape(-1, cnn_code.shape[-1])                    # the reference's [1, B, D] form is the same matrix
    txt = rnn_code.reshape(-1, rnn_code.shape[-1])
    norms = img.norm(p=2, dim=1, keepdim=True) * txt.norm(p=2, dim=1, keepdim=True).t()
    scores = img @ txt.t() / norms.clamp_min(eps) * cfg.TRAIN.SMOOTH.GAMMA3
    same_class = _class_masks(class_ids, batch_size, scores.device)
    if same_class is not None:
        scores = scores.masked_fill(same_class, float("-inf"))
    return _ranking_ce(scores, labels)


def _damsm_sim(img_features, words_emb, lens):
    """(sim [B, B], att [B, T, 17, 17]) of the batched DAMSM kernel, through autograd.DamsmWords when a gradient is wanted."""
    if torch.is_grad_enabled() and (img_features.requires_grad or words_emb.requires_grad):
        from ..autograd import DamsmWords
        return DamsmWords.apply(img_features, words_emb, lens, cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2)
    return C.damsm_words(img_features, words_emb, [int(v) for v in lens], float(cfg.TRAIN.SMOOTH.GAMMA1),
                         float(cfg.TRAIN.SMOOTH.GAMMA2))


def _words_ranking(sim, att, lens, labels, class_ids, batch_size):
    """losses.py:114-136: the per-caption maps, x gamma3, same-class pairs masked out, cross entropy along both axes."""
    att_maps = [att[i:i + 1, :lens[i]].contiguous() for i in range(batch_size)]
    similarities = sim * cfg.TRAIN.SMOOTH.GAMMA3
    masks = _class_masks(class_ids, batch_size, sim.device)
    if masks is not None:
        similarities = similarities.masked_fill(masks, -float('inf'))
    loss0, loss1 = _ranking_ce(similarities, labels)
    return loss0, loss1, att_maps


def words_loss(img_features, words_emb, labels, cap_lens, class_ids, batch_size):
    """losses.py:65-136.  words_emb(query): batch x nef x seq_len; img_features(context): batch x nef x 17 x 17.
    Returns (loss0, loss1, att_maps) with att_maps[i] = [1, cap_len_i, 17, 17]."""
    lens = cap_lens.data.tolist() if torch.is_tensor(cap_lens) else list(cap_lens)
    sim, att = _damsm_sim(img_features, words_emb, lens)
    return _words_ranking(sim, att, lens, labels, class_ids, batch_size)


def _damsm_sim_torch(img_features, words_emb, lens):
    """`_damsm_sim` as a torch composition (losses.py:73-113 through func_attention, GlobalAttention.py:33-74), all captions at
    once: what words_reweight_loss computes on CPU tensors.  (words_loss itself has no CPU form and refuses them.)"""
    B, nef, T = words_emb.shape
    g1, g2 = float(cfg.TRAIN.SMOOTH.GAMMA1), float(cfg.TRAIN.SMOOTH.GAMMA2)
    ctx = img_features.reshape(img_features.shape[0], nef, -1)                          # [j, d, r]
    valid = torch.arange(T, device=words_emb.device)[None, :] < torch.as_tensor(lens, device=words_emb.device)[:, None]   # [i, l]
    s = torch.einsum("jdr,idl->jirl", ctx, words_emb)
    a1 = torch.softmax(s.masked_fill(~valid[None, :, None, :], -float("inf")), dim=3)   # over the caption's words, per region
    a2 = torch.softmax(a1.transpose(2, 3) * g1, dim=3)                                  # over the regions, per word  [j, i, l, r]
    wc = torch.einsum("jdr,jilr->jild", ctx, a2)
    word = words_emb.transpose(1, 2)[None].expand(wc.shape[0], -1, -1, -1)              # [j, i, l, d]
    cos = (word * wc).sum(3) / (word.norm(p=2, dim=3) * wc.norm(p=2, dim=3)).clamp_min(1e-8)
    sim = torch.log((torch.exp(cos * g2) * valid[None]).sum(2))                         # [j, i]
    att = a2[torch.arange(B), torch.arange(B)] * valid[:, :, None]                      # image i on caption i
    return sim, att.reshape(B, T, *img_features.shape[2:]).detach()


def _attn_maps(attn_map):
    """The generator's maps as one [B, T', Q] tensor: a [B, T', h, w] tensor, or a list of per-image maps [T', h, w] /
    [1, T', h, w] (zero rows are appended where the images' maps differ in words)."""
    if torch.is_tensor(attn_map):
        return attn_map.detach().flatten(2)
    maps = [m.detach().reshape(-1, m.shape[-2] * m.shape[-1]) for m in attn_map]
    width = max(m.shape[0] for m in maps)
    return torch.stack([m if m.shape[0] == width else F.pad(m, (0, 0, 0, width - m.shape[0])) for m in maps])


def _attn_confidence_torch(att, lens):
    """conf [B, T'] of words_reweight_loss as a torch composition (losses.py:150-163 for every caption at once): the map's values
    strictly above float32(2 * (2 / n)), summed, for the caption's n words; zero behind them, and - as the kernel - a zero row for a
    length outside [1, T']."""
    lens = [n if 1 <= n <= att.shape[1] else 0 for n in lens]
    thr = torch.tensor([2. * (2. / float(n)) if n else float("inf") for n in lens], dtype=torch.float32, device=att.device)
    valid = torch.arange(att.shape[1], device=att.device)[None, :] < torch.as_tensor(lens, device=att.device)[:, None]
    return (att * (att > thr[:, None, None]).float()).sum(2) * valid


def attn_confidence(attn_map, cap_lens, fused=None):
    """The per-word weights of words_reweight_loss (losses.py:150-163), detached: conf [B, T'] float32, conf[i, j] = the sum of the
    values of word j's map of image i that lie strictly above 2 * (2 / cap_lens[i]) - compared in float32, as torch compares a
    float32 map with a Python double - for j < cap_lens[i], 0 behind.  One launch of tgsr_attn_confidence on HIP tensors (the
    reference: one `.cpu().numpy()` per word and caption); the torch composition on CPU tensors or with fused=False."""
    lens = [int(v) for v in (cap_lens.data.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    att = _attn_maps(attn_map)
    if att.shape[0] != len(lens):
        raise ValueError("attention maps of %d images against %d caption lengths" % (att.shape[0], len(lens)))
    if fused is None:
        fused = att.is_cuda and att.dtype == torch.float32 and att.shape[1] <= ops.WMSE_MAX_WORDS
    if not fused:
        return _attn_confidence_torch(att, lens)
    return C.attn_confidence(att, ops._lens_on_device(tuple(lens), att.device))


def words_reweight_loss(img_features, words_emb, labels, cap_lens, class_ids, batch_size, attn_map, fused=None):
    """losses.py:137-232: words_loss on the word embeddings scaled by `attn_confidence` of the generator's attention maps
    (`attn_map`: [B, T', h, w] or a list of per-image maps), the factor detached as in the reference (it passes through numpy
    there).  A caption of n <= 4 words has a threshold >= 1: its words enter as zero vectors, the losses stay finite and those
    words receive a zero gradient.  `fused` (not a reference argument): None = the kernels on HIP tensors, the torch compositions
    on CPU tensors; False = the compositions.  Returns (loss0, loss1, att_maps) like words_loss."""
    lens = cap_lens.data.tolist() if torch.is_tensor(cap_lens) else list(cap_lens)
    conf = attn_confidence(attn_map, lens, fused=fused).to(words_emb.dtype)
    T = words_emb.shape[2]
    conf = conf[:, :T] if conf.shape[1] >= T else F.pad(conf, (0, T - conf.shape[1]))
    scaled = words_emb * conf[:, None, :]
    if fused is None:
        fused = scaled.is_cuda
    sim, att = _damsm_sim(img_features, scaled, lens) if fused else _damsm_sim_torch(img_features, scaled, lens)
    return _words_ranking(sim, att, lens, labels, class_ids, batch_size)


def sent_similarity(cnn_code, rnn_code, eps=1e-8):
    """losses.py:234-250: the gamma3-scaled cosine of every image code [N, D] with every sentence code [M, D] -> [N, M] (the
    reference's [1, b, D] form is the same matrix), one launch of the gallery kernel (tgsr_sent_gallery_fwd).  An evaluation
    function: the result carries no grad_fn (`sent_loss` is the differentiable form)."""
    if cnn_code.dim() == 3 and cnn_code.shape[0] == 1:
        cnn_code, rnn_code = cnn_code[0], rnn_code[0]
    if cnn_code.dim() != 2 or rnn_code.dim() != 2:
        raise ValueError("sent_similarity: [b, D] or [1, b, D] codes expected, got %s and %s" % (tuple(cnn_code.shape), tuple(rnn_code.shape)))
    return C.sent_gallery(cnn_code.detach(), rnn_code.detach(), float(eps), float(cfg.TRAIN.SMOOTH.GAMMA3), None)


def words_similarity(img_features, words_emb, cap_lens, batch_size):
    """losses.py:251-287: similarities[j][i] = log sum_w exp(gamma2 * cos(word_w of caption i, its region context in image j)) for the
    first `batch_size` captions -> [b, batch_size], not scaled by gamma3 (the reference's callers do that).  The per-caption Python
    loop is one launch of the gallery kernel (tgsr_damsm_gallery_fwd).  An evaluation function: the result carries no grad_fn
    (`words_loss` is the differentiable form)."""
    lens = cap_lens.data.tolist() if torch.is_tensor(cap_lens) else list(cap_lens)
    batch_size = int(batch_size)
    if batch_size < 1 or batch_size > words_emb.shape[0] or batch_size > len(lens):
        raise ValueError("words_similarity: batch_size %d against %d captions and %d lengths" % (batch_size, words_emb.shape[0], len(lens)))
    return C.damsm_gallery(img_features.detach(), words_emb.detach()[:batch_size], [int(v) for v in lens[:batch_size]],
                           float(cfg.TRAIN.SMOOTH.GAMMA1), float(cfg.TRAIN.SMOOTH.GAMMA2), None)


def MSE(fake, label):
    """losses.py:779-784: sum over the image scales of the mean squared error."""
    return sum(F.mse_loss(f, t) for f, t in zip(fake, label))


def _cycle_mse_torch(fakeSR, Real_LR):
    """CycleMSE as the reference writes it (losses.py:785-790)."""
    mseloss = 0
    for i in range(len(fakeSR)):
        fakeLR = F.interpolate(fakeSR[i], size=[Real_LR.shape[2], Real_LR.shape[3]], mode="bicubic")
        mseloss = mseloss + F.mse_loss(fakeLR, Real_LR)
    return mseloss


def _cycle_mse_fusable(fakeSR, Real_LR):
    """Dense float32 HIP tensors of shapes the kernels take: the shape rule is ops.check_cycle_mse's, asked, not restated."""
    ts = list(fakeSR) + [Real_LR]
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts):
        return False
    try:
        ops.check_cycle_mse([t.shape for t in fakeSR], Real_LR.shape)
    except ops.TgsrError:
        return False
    return True


def CycleMSE(fakeSR, Real_LR, fused=None):
    """losses.py:785-790: sum over the SR images of a pyramid of mean((F.interpolate(fakeSR[i], size=[h, w], mode="bicubic") -
    Real_LR)^2) - every SR image, resized back to the LR size (align_corners=False, no antialiasing), must give the LR input.
    Differentiable w.r.t. every fakeSR[i] and Real_LR.
    `fused` (not a reference argument): None = one forward and one backward launch for the whole pyramid (autograd.CycleMSE,
    tgsr_cycle_mse.hip) where the tensors are dense float32 HIP tensors (any 4-byte aligned base: offset views are taken), at most
    8 scales, with equal B and C; the torch composition of the reference's expression elsewhere (CPU tensors, other dtypes, strided
    views, more scales); False = the composition; True = the kernels or an error.  The kernels' backward gathers - no atomics, the
    same bits on every run, which torch's upsample_bicubic2d_backward does not promise on the device - and nothing in either
    direction waits for the device, so the term can sit inside a captured update."""
    if fused or (fused is None and _cycle_mse_fusable(fakeSR, Real_LR)):
        from ..autograd import CycleMSE as _CycleMSE
        return _CycleMSE.apply(Real_LR, *fakeSR)[0]
    return _cycle_mse_torch(fakeSR, Real_LR)


def _weight_mse_torch(fake, label, att):
    """One scale of weight_MSE as the reference writes it (losses.py:796-800): (term, wups)."""
    w = att.max(dim=1, keepdim=True)[0]
    wups = F.interpolate(w, size=(fake.shape[2], fake.shape[3]))                  # nn.Upsample's default: nearest
    l2 = (att.shape[1] * wups) * (fake - label).pow(2)
    return l2.sum() / (fake.shape[2] * fake.shape[3] * fake.shape[0] * fake.shape[1]), wups


def _weight_mse_fusable(fake, label, att):
    """Float32 HIP tensors of shapes the kernels take: the shape rule is ops.check_weight_mse's, asked, not restated."""
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in (fake, label, att)):
        return False
    try:
        ops.check_weight_mse(fake.shape, label.shape, att.shape)
    except ops.TgsrError:
        return False
    return True


def weight_MSE(fake, label, weight, fused=None):
    """losses.py:792-804: sum over the image scales of sum(T wups (fake - label)^2) / (H W B C) with wups = the per-pixel maximum
    over the T words of the scale's attention map `weight[i]` [B, T, h, w], up-sampled (nearest) to the image.  Returns (mseloss,
    wlast), wlast = the last scale's wups [B, 1, H, W].  Differentiable w.r.t. fake, label and weight; the map's gradient goes to
    the word that held the maximum, the lowest index on a tie (the reference pins none).
    `fused` (not a reference argument): None = one forward and one backward launch per scale (autograd.WeightMSE) where the
    tensors are float32 HIP tensors, H / h = W / w is an integer and T <= 255, the torch composition of the reference's
    expression elsewhere (CPU tensors, any other ratio); False = the composition; True = the kernels or an error.  On the fused
    path `wlast` carries no grad_fn: a caller that differentiates through wlast passes fused=False.  The two forms differ on a NaN
    in a map: the kernels' strict comparison passes it over (the maximum of the other words), torch.max propagates it."""
    mseloss, wlast = 0, None
    for i in range(len(fake)):
        last = i == len(fake) - 1
        if fused or (fused is None and _weight_mse_fusable(fake[i], label[i], weight[i])):
            from ..autograd import WeightMSE
            mse, wups = WeightMSE.apply(fake[i], label[i], weight[i], last)
        else:
            mse, wups = _weight_mse_torch(fake[i], label[i], weight[i])
        if last:
            wlast = wups
        mseloss = mseloss + mse
    return mseloss, wlast


def KL_loss(mu, logvar):
    """losses.py:806-810: -0.5 * mean(1 + logvar - mu^2 - exp(logvar))."""
    return -0.5 * torch.mean(1.0 + logvar - mu * mu - logvar.exp())


def _bce(logits, target):
    return F.binary_cross_entropy_with_logits(logits, target)


_BCE_WEIGHTS = {}


def _bce_weights(device, *runs):
    """The per-logit weights of a sum of mean-reduced BCE terms, `runs` = (count, weight of every element) in order: a device
    tensor built from fill kernels once per distinct argument list (no host copy: also legal inside a hipGraph capture)."""
    key = (str(device),) + runs
    w = _BCE_WEIGHTS.get(key)
    if w is None:
        w = _BCE_WEIGHTS[key] = torch.cat([torch.full((int(n),), float(v), dtype=torch.float32, device=device) for n, v in runs])
    return w


def _fused_bce_ok(*ts):
    return all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in ts)


def discriminator_loss(netD, real_imgs, fake_imgs, conditions, real_labels, fake_labels):
    """losses.py:290-316.  The reference ships no discriminator class; any module exposing `COND_DNET` /
    `UNCOND_DNET` like AttnGAN's D_NET* works: real / fake / wrong-caption terms, the wrong pair being the batch
    shifted by one (:302).
    Under data parallelism (decided here): the shift stays INSIDE the shard - rank r pairs its image i with its
    caption i + 1, so world x (B - 1) wrong pairs are scored instead of world x B - 1 (the pair that would straddle two shards
    is dropped) and each weighs 1 / (world (B - 1)) after the gradient all-reduce's average.  The discriminators normalise with
    per-shard BatchNorm statistics anyway (parallel.py), so this loss is a per-shard quantity by construction; no halo exchange
    of conditions is made for one pair in B."""
    n = real_imgs.size(0)
    if getattr(netD, "supports_groups", False) and n > 1:
        # the build's D_NET*: the real and the fake pass as ONE batch whose two halves keep their own BatchNorm batch
        # statistics (and update the running statistics in the reference's order: real, then fake) - one convolution,
        # data-gradient and weight-gradient launch per layer instead of two, and every parameter receives one gradient;
        # the three conditional heads (real, fake, mismatched) likewise.  Numerically the passes run one by one.
        feats = netD(torch.cat((real_imgs, fake_imgs.detach())), groups=(n, n))
        feat_real, feat_fake = feats[:n], feats[n:]
        lc = netD.COND_DNET(torch.cat((feats, feat_real[:n - 1])), torch.cat((conditions, conditions, conditions[1:n])),
                            groups=(n, n, n - 1))
        lu = netD.UNCOND_DNET(feats) if netD.UNCOND_DNET is not None else None
        if _fused_bce_ok(lc, lu, real_labels, fake_labels):
            # the five mean-reduced BCE terms and their /2, /3 combination as ONE launch (tgsr::weighted_bce; its backward another):
            # ~40 small aten launches per discriminator and step otherwise (BCE, mean, slice backward fills, adds)
            tc = (real_labels, fake_labels, fake_labels[1:n])
            if lu is None:
                return C.weighted_bce(lc, None, torch.cat(tc), _bce_weights(lc.device, (n, 1. / n), (n, .5 / n), (n - 1, .5 / (n - 1))))
            return C.weighted_bce(lc, lu, torch.cat(tc + (real_labels, fake_labels)),
                                  _bce_weights(lc.device, (n, .5 / n), (n, 1. / (3 * n)), (n - 1, 1. / (3 * (n - 1))), (n, .5 / n),
                                               (n, 1. / (3 * n))))
        cond = {"real": _bce(lc[:n], real_labels), "fake": _bce(lc[n:2 * n], fake_labels),
                "wrong": _bce(lc[2 * n:], fake_labels[1:n])}
        if lu is None:
            return cond["real"] + (cond["fake"] + cond["wrong"]) / 2.
        return (_bce(lu[:n], real_labels) + cond["real"]) / 2. + (_bce(lu[n:], fake_labels) + cond["fake"] + cond["wrong"]) / 3.
    feat_real, feat_fake = netD(real_imgs), netD(fake_imgs.detach())
    cond = {"real": _bce(netD.COND_DNET(feat_real, conditions), real_labels),
            "fake": _bce(netD.COND_DNET(feat_fake, conditions), fake_labels),
            "wrong": _bce(netD.COND_DNET(feat_real[:n - 1], conditions[1:n]), fake_labels[1:n])}
    if netD.UNCOND_DNET is None:
        return cond["real"] + (cond["fake"] + cond["wrong"]) / 2.
    unc_real = _bce(netD.UNCOND_DNET(feat_real), real_labels)
    unc_fake = _bce(netD.UNCOND_DNET(feat_fake), fake_labels)
    return (unc_real + cond["real"]) / 2. + (unc_fake + cond["fake"] + cond["wrong"]) / 3.


class _LazyLog:
    """The log string of generator_loss, formatted when somebody looks at it: the reference builds it with `.item()` on
    every term (losses.py:366-390) - three device synchronisations inside the generator step that nothing needs unless
    the string is printed.  Behaves like the str it stands for under str(), format(), +, +=, len, in, slicing and ==; it
    is NOT a str instance (a str subclass cannot fill its character buffer later, so C-level consumers - file.write,
    ''.join - would silently see an empty string).  Only handed out on request: generator_loss(lazy_log=True), which
    train.SRTrainer passes; the default return is the reference's plain str.  The loss tensors are released once the
    text has been formatted."""

    def __init__(self, parts):
        self._parts = parts                      # [(format, tensor, ...), ...]; dropped once formatted
        self._text = None

    def __str__(self):
        if self._text is None:
            self._text = "".join(f % tuple(float(t) for t in ts) for f, *ts in self._parts)
            self._parts = None
        return self._text

    __repr__ = __str__

    def __format__(self, spec):
        return format(str(self), spec)

    def __add__(self, other):
        return str(self) + str(other)

    def __radd__(self, other):
        return str(other) + str(self)

    def __len__(self):
        return len(str(self))

    def __contains__(self, item):
        return item in str(self)

    def __getitem__(self, k):
        return str(self)[k]

    def __eq__(self, other):
        return str(self) == other

    def __hash__(self):
        return hash(str(self))


def damsm_terms(regions, code, words_embs, sent_emb, cap_lens, class_ids, gather=False):
    """(w_loss0, w_loss1, s_loss0, s_loss1, scale, att_maps) of one shard's images and captions.  gather=False: the shard's own
    B x B matching matrices (what the single-process reference computes), scale 1.  gather=True under torch.distributed: the
    matrices of the GLOBAL batch (parallel.gather_damsm_batch; the same four numbers on every rank = the single-process
    losses of the concatenated batch) and scale = world - multiply the term by it before backward, the gradient bucket
    averages over ranks what a replicated loss needs summed."""
    scale = 1
    if gather:
        from .. import parallel
        regions, code, words_embs, sent_emb, cap_lens, class_ids, B, scale = parallel.gather_damsm_batch(
            regions, code, words_embs, sent_emb, cap_lens, class_ids, cfg.TEXT.WORDS_NUM)
    else:
        B = sent_emb.shape[0]
    labels = torch.arange(B, device=sent_emb.device)
    w0, w1, att = words_loss(regions, words_embs, labels, cap_lens, class_ids, B)
    s0, s1 = sent_loss(code, sent_emb, labels, class_ids, B)
    return w0, w1, s0, s1, scale, att


def generator_loss(netsD, image_encoder, fake_imgs, real_labels, words_embs, sent_emb, match_labels, cap_lens,
                   class_ids, w=1, s=1, g=1, streams=None, lazy_log=False, gather_negatives=False, enc_out=None):
    """losses.py:351-391: per-scale adversarial terms + the DAMSM words / sentence ranking loss on the last scale
    (x TRAIN.SMOOTH.LAMBDA).  Returns (total, log) like the reference: `log` is the same str; with `lazy_log=True` (not a
    reference argument) a _LazyLog stands in for it - the same text, formatted (and the device synchronised) only when it
    is looked at.  `image_encoder=None` (the reference
    always has one; its Inception-v3 weights are third-party and not shipped) leaves the ranking term out.  `enc_out` (not a
    reference argument): `image_encoder(fake_imgs[-1])` computed by the caller already - the encoder reads the fake image only, not
    the discriminators, so train.SRTrainer runs it beside the discriminator updates that precede this call."""
    return _generator_loss(words_loss, netsD, image_encoder, fake_imgs, real_labels, words_embs, sent_emb, match_labels, cap_lens,
                           class_ids, w, s, g, streams, lazy_log, gather_negatives, enc_out)


def generator_re_weight_loss(netsD, image_encoder, fake_imgs, real_labels, words_embs, sent_emb, match_labels, cap_lens,
                             class_ids, w=1, s=1, g=1, attn=None, streams=None, lazy_log=False, enc_out=None, fused=None):
    """losses.py:318-350: generator_loss with `words_reweight_loss` on the attention maps `attn` ([B, T, h, w] or a list of
    per-image maps) in place of words_loss - the same terms, order and log text.  streams / lazy_log / enc_out as in
    generator_loss, `fused` as in words_reweight_loss.  There is no gather_negatives form: the confidences would have to be
    gathered with the words."""
    if attn is None and image_encoder is not None and len(netsD) > 0:
        raise ValueError("generator_re_weight_loss: attn (the generator's attention maps) is required for the ranking term")

    def words(regions, words_embs, labels, cap_lens, class_ids, B):
        return words_reweight_loss(regions, words_embs, labels, cap_lens, class_ids, B, attn, fused=fused)
    return _generator_loss(words, netsD, image_encoder, fake_imgs, real_labels, words_embs, sent_emb, match_labels, cap_lens,
                           class_ids, w, s, g, streams, lazy_log, False, enc_out)


def _generator_loss(words_fn, netsD, image_encoder, fake_imgs, real_labels, words_embs, sent_emb, match_labels, cap_lens,
                    class_ids, w, s, g, streams, lazy_log, gather_negatives, enc_out):
    """The body of generator_loss / generator_re_weight_loss; words_fn = words_loss or its re-weighted form."""
    B = real_labels.size(0)
    total, parts = 0, []
    advs = []
    main = torch.cuda.current_stream(real_labels.device) if streams else None
    for k, (netD, img) in enumerate(zip(netsD, fake_imgs)):
        # `streams` (not a reference argument): one stream per discriminator - their forward passes, and through
        # autograd's stream rule their backward passes, run side by side; the terms are added up on the calling stream
        st = streams[k] if streams else None
        if st is not None:
            st.wait_stream(main)
        with torch.cuda.stream(st) if st is not None else contextlib.nullcontext():
            if st is not None:
                for t in (img, sent_emb, real_labels):
                    t.record_stream(st)                    # allocated on the calling stream, read on this one
            feat = netD(img)
            lc = netD.COND_DNET(feat, sent_emb)
            lu = netD.UNCOND_DNET(feat) if netD.UNCOND_DNET is not None else None
            if _fused_bce_ok(lc, lu, real_labels) and lc.dim() == 1:
                # g * (BCE(cond logits, real) + BCE(uncond logits, real)), one launch
                adv = C.weighted_bce(lc, lu, real_labels if lu is None else torch.cat((real_labels, real_labels)),
                                     _bce_weights(lc.device, (lc.numel() + (0 if lu is None else lu.numel()), float(g) / B)))
            else:
                adv = _bce(lc, real_labels)
                if lu is not None:
                    adv = adv + _bce(lu, real_labels)
                adv = g * adv
        advs.append(adv)
    # the ranking term's image encoder (the frozen trunk: ~190 launches forward) is issued BEFORE the calling stream joins the
    # discriminators' streams: it reads the last fake image only, so it runs beside their forward passes (and, through autograd's
    # stream rule, its backward beside theirs)
    if enc_out is None and image_encoder is not None and len(netsD) > 0:
        enc_out = image_encoder(fake_imgs[len(netsD) - 1])
    for k, (netD, img) in enumerate(zip(netsD, fake_imgs)):
        adv = advs[k]
        if streams:
            main.wait_stream(streams[k])
            adv.record_stream(main)
        total = total + adv
        parts.append(("g_loss%d: %%.5f " % k, adv.detach()))
        if k == len(netsD) - 1 and image_encoder is not None:
            regions, code = enc_out
            if gather_negatives:        # (not a reference argument) data parallel: the ranking term of the global batch
                w0, w1, s0, s1, scale, _ = damsm_terms(regions, code, words_embs, sent_emb, cap_lens, class_ids, gather=True)
            else:
                w0, w1, _ = words_fn(regions, words_embs, match_labels, cap_lens, class_ids, B)
                s0, s1 = sent_loss(code, sent_emb, match_labels, class_ids, B)
                scale = 1
            w_term = w * (w0 + w1) * cfg.TRAIN.SMOOTH.LAMBDA
            s_term = s * (s0 + s1) * cfg.TRAIN.SMOOTH.LAMBDA
            total = total + (w_term + s_term) * scale
            parts.append(("w_loss: %.5f s_loss: %.5f ", w_term.detach(), s_term.detach()))
    log = _LazyLog(parts)
    return total, (log if lazy_log else str(log))
