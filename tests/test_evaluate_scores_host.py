"""CPU: the accumulators SRTrainer.evaluate drives - retrieval.Gallery, featdist.RealismScores, niqe.NIQEScores and
ScoreBook.all_gather - each against the lines it replaced, written out here, and over two gloo ranks (no kernel runs)."""
import functools
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from test_niqe_host import _batches


# ----------------------------------------------------------------------------------------- retrieval.Gallery
def _gallery_batches():
    """Three batches of 3, 2 and 4 items whose word axes are 5, 9 and 7 long; the lengths come as a tensor, a list, a tensor."""
    g = torch.Generator().manual_seed(5)
    out = []
    for k, (B, T) in enumerate(((3, 5), (2, 9), (4, 7))):
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[0] = T
        out.append((torch.randn(B, 6, 3, 3, generator=g), torch.randn(B, 6, generator=g), torch.randn(B, 6, T, generator=g),
                    torch.randn(B, 6, generator=g), lens.tolist() if k == 1 else lens))
    return out


def _through_the_gallery(batches, max_items=None):
    """The loop of DAMSMTrainer.evaluate_retrieval around the gallery."""
    from tgsr_amd.retrieval import Gallery
    gallery = Gallery()
    for regions, codes, words, sents, lens in batches:
        if max_items is not None and len(gallery) >= max_items:
            break
        B = codes.shape[0]
        gallery.add(regions, codes, words, sents, lens, take=B if max_items is None else min(B, max_items - len(gallery)))
    return gallery.cat()


def _evaluate_retrieval_as_it_was(batches, max_items=None):
    """What DAMSMTrainer.evaluate_retrieval did with the same features before the gallery existed, line for line."""
    regions, codes, words, sents, lens, n = [], [], [], [], [], 0
    for wf, code, we, se, cap_lens in batches:
        if max_items is not None and n >= max_items:
            break
        B = code.shape[0]
        take = B if max_items is None else min(B, max_items - n)
        regions.append(wf[:take]); codes.append(code[:take]); words.append(we[:take]); sents.append(se[:take])
        lens += [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)][:take]
        n += take
    Tw = max(w.shape[2] for w in words)
    words = [w if w.shape[2] == Tw else torch.nn.functional.pad(w, (0, Tw - w.shape[2])) for w in words]
    return torch.cat(regions), torch.cat(codes), torch.cat(words), torch.cat(sents), lens


def _same(got, want):
    assert len(got) == len(want) == 5
    assert all(torch.equal(a, b) for a, b in zip(got[:4], want[:4]))
    assert got[4] == want[4] and all(type(v) is int for v in got[4])


def test_the_gallery_pads_the_word_axis_to_the_longest_caption_and_truncates():
    from tgsr_amd.retrieval import Gallery
    bs = _gallery_batches()
    gallery = Gallery()
    for k, b in enumerate(bs):
        gallery.add(*b, class_ids=torch.tensor([10 * k + i for i in range(b[1].shape[0])]))
    words = torch.zeros(9, 6, 9)
    words[0:3, :, :5], words[3:5], words[5:9, :, :7] = bs[0][2], bs[1][2], bs[2][2]
    lens = bs[0][4].tolist() + bs[1][4] + bs[2][4].tolist()
    _same(gallery.cat(), (torch.cat([b[0] for b in bs]), torch.cat([b[1] for b in bs]), words, torch.cat([b[3] for b in bs]), lens))
    assert len(gallery) == 9 and gallery.class_ids == [0, 1, 2, 10, 11, 20, 21, 22, 23]
    assert all(type(v) is int for v in gallery.class_ids)
    got = _through_the_gallery(bs, max_items=7)                     # the last batch gives two of its four items
    _same(got, (torch.cat([bs[0][0], bs[1][0], bs[2][0][:2]]), torch.cat([bs[0][1], bs[1][1], bs[2][1][:2]]), words[:7],
                torch.cat([bs[0][3], bs[1][3], bs[2][3][:2]]), lens[:7]))


@pytest.mark.parametrize("max_items", [None, 100, 9, 7, 5, 4, 1])
def test_the_gallery_collects_what_evaluate_retrieval_collected(max_items):
    bs = _gallery_batches()
    _same(_through_the_gallery(bs, max_items), _evaluate_retrieval_as_it_was(bs, max_items))


# ----------------------------------------------------------------------------------------- featdist.RealismScores
N, D, NBATCH = 20, 8, 5
KID = {"subsets": 4, "subset_size": 6}


def _features():
    """(outputs', ground truth's): five batches of four float32 rows of D = 8 each, the two sets distributed differently."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand(N, D, generator=g)
    y = 0.3 + 0.8 * torch.rand(N, D, generator=g) ** 2
    return list(x.split(N // NBATCH)), list(y.split(N // NBATCH))


def _moments(batches):
    from tgsr_amd.featdist import FeatureMoments
    mom = FeatureMoments(D, "cpu")
    for b in batches:
        mom.add(b)
    return mom


def test_realism_scores_are_the_distances_of_moments_and_banks_filled_by_hand(tmp_path):
    from tgsr_amd import featdist
    xs, ys = _features()
    acc = featdist.RealismScores(True, dict(KID), "cpu")
    assert acc.needs_truth
    for x, y in zip(xs, ys):
        acc.add(x, y)
    res = acc.result(torch.Generator().manual_seed(1))
    assert list(res) == ["fid", "kid"]
    mx, my = _moments(xs), _moments(ys)
    fd = featdist.frechet_distance(mx, my)
    assert res["fid"] == {"fine": fd, "n": N} and fd > 0
    bx, by = featdist.FeatureBank(), featdist.FeatureBank()
    for x, y in zip(xs, ys):
        bx.add(x); by.add(y)
    want = featdist.kernel_distance(bx, by, generator=torch.Generator().manual_seed(1), **KID)
    assert res["kid"]["mean"] == want["mean"] and res["kid"]["std"] == want["std"]
    assert res["kid"]["per_subset"].shape == (4,) and torch.equal(res["kid"]["per_subset"], want["per_subset"])

    # one score alone; False is "not asked for", kid=True is kernel_distance's defaults
    only = featdist.RealismScores(True, False, "cpu")
    assert only.kid is None and only.needs_truth
    for x, y in zip(xs, ys):
        only.add(x, y)
    assert only.result() == {"fid": {"fine": fd, "n": N}}
    k = featdist.RealismScores(False, True, "cpu")
    assert k.fid is None and k.kid == {} and k.needs_truth

    # the ground-truth side from saved statistics: nothing of it is asked for, and the distance is the same
    path = my.save(str(tmp_path / "gt.npz"))
    for saved in (path, tmp_path / "gt.npz", featdist.FeatureMoments.load(path, "cpu")):
        acc = featdist.RealismScores(saved, None, "cpu")
        assert not acc.needs_truth
        for x in xs:
            acc.add(x, None)
        assert acc.result() == {"fid": {"fine": fd, "n": N}}
    assert featdist.RealismScores(path, True, "cpu").needs_truth      # the banks of `kid` want both sides


def test_realism_scores_refuse_what_evaluate_refused(tmp_path):
    from tgsr_amd import featdist
    for bad in ({"subset": 3}, {"subsets": 2, "size": 4}, 3, "all", [True]):
        with pytest.raises(ValueError, match="evaluate: kid is True or a dict of subsets / subset_size, got"):
            featdist.RealismScores(None, bad, "cpu")
    with pytest.raises(FileNotFoundError):
        featdist.RealismScores(str(tmp_path / "absent.npz"), None, "cpu")


def test_evaluate_checks_its_arguments_in_order_before_the_first_batch():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import SRTrainer
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    try:
        torch.manual_seed(2)
        tr = SRTrainer(41, device="cpu")                             # no image encoder
        every = dict(r_precision=3, ensemble=4, fid=True, kid={"subset": 3}, niqe=3)
        for first, match in (("r_precision", r"evaluate\(r_precision=3\) needs the trainer's image_encoder"),
                             ("ensemble", "evaluate: ensemble is 1 or 8"),
                             ("fid", r"evaluate\(fid=True, kid=\{'subset': 3\}\) needs the trainer's image_encoder"),
                             ("niqe", "evaluate: niqe is True, a NIQEModel or the path of one, got 3")):
            with pytest.raises(ValueError, match=match):
                tr.evaluate(iter(()), **every)
            del every[first]
            if first == "fid":
                del every["kid"]
        with pytest.raises(ValueError, match=r"evaluate\(fid=None, kid=\{\}\) needs the trainer's image_encoder"):
            tr.evaluate(iter(()), fid=False, kid=True)
        tr.image_encoder = object()                                  # present: the values themselves are looked at, kid's first
        with pytest.raises(ValueError, match="evaluate: kid is True or a dict of subsets / subset_size, got {'subset': 3}"):
            tr.evaluate(iter(()), r_precision=3, fid=True, kid={"subset": 3}, niqe=3)
        with pytest.raises(ValueError, match="evaluate: niqe is True"):
            tr.evaluate(iter(()), r_precision=3, fid=True, kid=True, niqe=3)
    finally:
        cfg_reset()


# ----------------------------------------------------------------------------------------- niqe.NIQEScores
SHAVE = 4


@functools.lru_cache(maxsize=None)
def _pairs():
    """[(sr, hr)] of test_niqe_host's batches: uint8, 384 x 288, two images each; the "output" is the mirrored ground truth."""
    return [(torch.flip(hr, (3,)), hr) for hr in _batches()]


@functools.lru_cache(maxsize=None)
def _block_features():
    """The block features of both sides of every pair at SHAVE, computed once."""
    from tgsr_amd import niqe
    return [(niqe.niqe_features(sr, SHAVE)[0], niqe.niqe_features(hr, SHAVE)[0]) for sr, hr in _pairs()]


def _rows(model, side):
    return torch.cat([model.score_features(f[side]) for f in _block_features()]).numpy()


def _check_niqe(res, model):
    assert sorted(res) == ["fine", "hr", "mean", "n"] and res["n"] == 6
    for side, name in enumerate(("fine", "hr")):
        want = _rows(model, side)
        assert np.isfinite(want).all() and np.array_equal(res[name], want)
        assert res["mean"][name] == float(np.mean(want))


def test_niqe_scores_fit_from_the_ground_truth_seen_then_score():
    from tgsr_amd import niqe
    pairs = _pairs()
    acc = niqe.NIQEScores(True, SHAVE, "cpu")
    for sr, hr in pairs:
        acc.add(sr, hr)
    res = acc.result()
    fitted = niqe.NIQEModel.fit([hr for _sr, hr in pairs], shave=SHAVE, device="cpu")
    _check_niqe(res, fitted)
    assert torch.equal(acc.model.mu, fitted.mu) and torch.equal(acc.model.cov, fitted.cov)
    assert not np.array_equal(res["fine"], res["hr"])


def test_niqe_scores_against_a_given_model_or_its_file(tmp_path):
    from tgsr_amd import niqe
    pairs = _pairs()
    model = niqe.NIQEModel.fit([pairs[0][1]], sharpness=0.0, device="cpu")
    for given in (model, model.save(str(tmp_path / "model.npz")), tmp_path / "model.npz"):
        acc = niqe.NIQEScores(given, SHAVE, "cpu")
        for sr, hr in pairs:
            acc.add(sr, hr)
        res = acc.result()
        _check_niqe(res, model)
        assert np.array_equal(res["fine"], torch.cat([model.score(sr, SHAVE) for sr, _hr in pairs]).numpy())
        assert np.array_equal(res["hr"], torch.cat([model.score(hr, SHAVE) for _sr, hr in pairs]).numpy())
    for bad in (3, 0.5, {"mu": 1}, [True], None, False):
        with pytest.raises(ValueError, match="niqe"):
            niqe.NIQEScores(bad, SHAVE, "cpu")
    with pytest.raises(FileNotFoundError):
        niqe.NIQEScores(str(tmp_path / "absent.npz"), SHAVE, "cpu")


# ----------------------------------------------------------------------------------------- metrics.ScoreBook.all_gather
SIZES = {("fine", 0): (64, 64), ("fine", 1): (128, 96)}


def _book_rows(rank):
    """Rank 0 holds 3 rows per scale, rank 1 holds 5: integer sums of squares and an SSIM sum, as the kernel's rows are."""
    rng = np.random.default_rng(20 + rank)
    n = 3 if rank == 0 else 5
    return {s: np.concatenate([rng.integers(1, 10 ** 7, (n, 2)).astype(np.float64), rng.uniform(100, 2000, (n, 1))], 1) for s in SIZES}


def test_all_gather_without_a_group_is_the_book_itself():
    from tgsr_amd import metrics
    book = metrics.ScoreBook.from_rows(_book_rows(0), SIZES, 2)
    assert book.all_gather() is book
    empty = metrics.ScoreBook(2)
    assert empty.all_gather() is empty and empty.result() == {}


# ----------------------------------------------------------------------------------------- two gloo ranks, uneven shards
def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from tgsr_amd import featdist, metrics, niqe, parallel
    parallel.init_distributed("gloo")
    # the order of the collectives is evaluate's: the book, the moments behind fid, NIQE's fit and rows
    book = metrics.ScoreBook.from_rows(_book_rows(rank), SIZES, 2).all_gather()
    xs, ys = _features()
    mine = slice(0, 2) if rank == 0 else slice(2, NBATCH)
    real = featdist.RealismScores(True, None, "cpu")
    for x, y in zip(xs[mine], ys[mine]):
        real.add(x, y)
    fid = real.result()
    acc = niqe.NIQEScores(True, SHAVE, "cpu")
    for sr, hr in (_pairs()[:1] if rank == 0 else _pairs()[1:]):
        acc.add(sr, hr)
    rows = acc.result()
    q.put({"rank": rank, "book": {s: book.rows(s) for s in book.scales()}, "book_result": book.result(), "fid": fid,
           "moments": [m.state_dict() for m in (real.mom_sr, real.mom_gt)], "niqe": rows,
           "model": (float(acc.model.n), acc.model.mu.numpy(), acc.model.cov.numpy())})
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=120) for _ in ps), key=lambda r: r["rank"])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    return res


def _equal(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_books_come_back_merged_in_rank_order_on_both_ranks(two_ranks):
    from tgsr_amd import metrics
    want = {s: np.concatenate([_book_rows(0)[s], _book_rows(1)[s]]) for s in SIZES}
    whole = metrics.ScoreBook.from_rows(want, SIZES, 2).result()
    for r in two_ranks:
        assert list(r["book"]) == list(SIZES)
        assert all(np.array_equal(r["book"][s], want[s]) for s in SIZES)
        assert _equal(r["book_result"], whole) and r["book_result"]["fine", 1]["n"] == 8


def test_realism_scores_over_two_ranks_are_those_of_the_union(two_ranks):
    """The all-reduce adds two partial sums where one process adds batch by batch, so the moments agree to rounding - 1e-12
    relative to the largest entry, the margin of test_niqe_host's all-reduce test - and "fid" is frechet_distance of exactly the
    moments the ranks ended with; both ranks hold the same bits."""
    from tgsr_amd import featdist
    xs, ys = _features()
    whole = featdist.RealismScores(True, None, "cpu")
    for x, y in zip(xs, ys):
        whole.add(x, y)
    want = whole.result()
    for r in two_ranks:
        ends = []
        for sd, mom in zip(r["moments"], (whole.mom_sr, whole.mom_gt)):
            assert int(sd["n"]) == N
            assert np.allclose(sd["sum"], mom.sum.numpy(), rtol=1e-12, atol=0)
            assert np.allclose(sd["outer"], mom.outer.numpy(), rtol=0, atol=1e-12 * float(mom.outer.abs().max()))
            ends.append(featdist.FeatureMoments(D, "cpu").load_state_dict(sd))
        assert r["fid"] == {"fid": {"fine": featdist.frechet_distance(*ends), "n": N}}
        # D = 8 features of 20 rows: a covariance of full rank, a distance determined to 1e-9 (test_featdist_host.py)
        assert abs(r["fid"]["fid"]["fine"] - want["fid"]["fine"]) <= 1e-9 * abs(want["fid"]["fine"])
    assert _equal(two_ranks[0]["fid"], two_ranks[1]["fid"]) and _equal(two_ranks[0]["moments"], two_ranks[1]["moments"])


def test_niqe_scores_over_two_ranks_are_those_of_the_union_in_rank_order(two_ranks):
    """Both ranks score against the fit of the union (1e-12 on its moments' mu and cov, as test_niqe_host's all-reduce test asks),
    and their rows are exactly the scores of the six images, rank 0's two first, against the model they ended with."""
    from tgsr_amd import niqe
    pairs = _pairs()
    whole = niqe.NIQEModel.fit([hr for _sr, hr in pairs], shave=SHAVE, device="cpu")
    for r in two_ranks:
        n, mu, cov = r["model"]
        assert n == float(whole.n)
        assert np.allclose(mu, whole.mu.numpy(), rtol=1e-12, atol=0)
        assert np.allclose(cov, whole.cov.numpy(), rtol=0, atol=1e-12 * float(whole.cov.abs().max()))
        _check_niqe(r["niqe"], niqe.NIQEModel(mu, cov, "cpu"))
    assert _equal(two_ranks[0]["niqe"], two_ranks[1]["niqe"]) and _equal(two_ranks[0]["model"], two_ranks[1]["model"])
