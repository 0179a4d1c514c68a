"""GPU: text-image retrieval - the gallery kernels and the rank kernel of csrc/tgsr_retrieval.hip through ctypes and through the
`torch.ops.tgsr` operators, then retrieval.py and the two trainers' retrieval evaluation on top of them.

    tgsr_damsm_gallery_fwd    tgsr_sent_gallery_fwd    tgsr_retrieval_ranks

Bound: TOL_SIM = atol 2e-5, rtol 1e-5 (the project's bound for this arithmetic, tests/test_hip_attention_abi.py), every value, against
the reference's fp32 output AND its fp64 run on the same inputs (tests/golden/retrieval.npz; the two are within 1e-6 of each other,
tests/test_retrieval_host.py, so the bound measures the kernel).  Shapes too large for a fixture (ndf 256 / 512 with S 289 / 320)
are held to the same bound against the fp64 restatement of tests/retrieval_cases.py, which test_retrieval_host.py ties to the reference.

The gallery kernel's own promise is checked bit for bit: the score of an (image, caption) pair is the same whether the caption
shared its MFMA tile with a neighbour or ran alone, in an even or an odd column, beside a short caption, a long one or an empty slot.
"""
import ctypes

import numpy as np
import pytest
import torch

import retrieval_cases as R
from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG_INF = float("-inf")


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gallery_abi(regions, words, lens, cand, g1, g2, K=None):
    """tgsr_damsm_gallery_fwd through ctypes, every operand in a guarded arena: sim [N][K] on the host, guards checked."""
    M_, L = _lib()
    N, ndf, ih, iw = regions.shape
    M, _, Tw = words.shape
    K = (M if cand is None else cand.shape[1]) if K is None else K
    a = Arena(DEV)
    w = a.place_input(words)
    c = a.place_input(regions.reshape(N, ndf, ih * iw))
    ln = a.place_input(_i32(lens)) if lens is not None else None
    cd = a.place_input(_i32(cand)) if cand is not None else None
    sim = a.place_output((N, K))
    rc = L.tgsr_damsm_gallery_fwd(w.ptr, ln.ptr if ln else None, c.ptr, cd.ptr if cd else None, N, M, K, ndf, Tw, ih * iw,
                                  g1, g2, sim.ptr, _stream())
    assert rc == M_.OK, rc
    v = [m for m in a.violations() if "non-finite" not in m]          # an empty slot scores -inf: that is the contract
    assert not v, "; ".join(v)
    return sim.read()


def _sent_abi(cnn, rnn, cand, eps, g3):
    M_, L = _lib()
    (N, ndf), M = cnn.shape, rnn.shape[0]
    K = M if cand is None else cand.shape[1]
    a = Arena(DEV)
    x, y = a.place_input(cnn), a.place_input(rnn)
    cd = a.place_input(_i32(cand)) if cand is not None else None
    sim = a.place_output((N, K))
    assert L.tgsr_sent_gallery_fwd(x.ptr, y.ptr, cd.ptr if cd else None, N, M, K, ndf, eps, g3, sim.ptr, _stream()) == M_.OK
    v = [m for m in a.violations() if "non-finite" not in m]
    assert not v, "; ".join(v)
    return sim.read()


def _ranks_abi(sim, target):
    M_, L = _lib()
    N, K = sim.shape
    a = Arena(DEV)
    s, t = a.place_input(torch.as_tensor(sim, dtype=torch.float32)), a.place_input(_i32(target))
    r = a.place_output((N,), dtype=torch.int32)
    assert L.tgsr_retrieval_ranks(s.ptr, t.ptr, N, K, r.ptr, _stream()) == M_.OK
    a.check()
    return r.read().numpy()


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


# ---- gallery kernels against the reference ----
@pytest.mark.parametrize("name", R.CASES)
def test_gallery_matches_the_reference_fp32_and_fp64(name):
    """The fixture's shapes: c0 N = 3, M = 5 (K odd: the last column alone), ndf = 32, S = 9, Tw = 1, cap_lens NULL;  c1 Tw = 32 with
    lengths {1, 16, 17, 32}, S = 289;  c2 ndf = 64, S = 33;  c3 S = 320;  e2e lengths 1..18.  ctypes and operator give the same bits."""
    c = R.case(name)
    g1, g2, g3 = R.gammas()
    lens = c["lens"].tolist()
    sim = _gallery_abi(c["regions"], c["words"], None if name == "c0" else lens, None, g1, g2)
    R.close(sim, c["words_sim32"], what=name + " words vs reference fp32")
    R.close(sim, c["words_sim64"], what=name + " words vs reference fp64")
    op = torch.ops.tgsr.damsm_gallery(c["regions"].to(DEV), c["words"].to(DEV), lens, g1, g2)
    assert torch.equal(_bits(op.cpu()), _bits(sim))
    ssim = _sent_abi(c["codes"], c["sents"], None, 1e-8, g3)
    R.close(ssim, c["sent_sim32"], what=name + " sent vs reference fp32")
    R.close(ssim, c["sent_sim64"], what=name + " sent vs reference fp64")
    op = torch.ops.tgsr.sent_gallery(c["codes"].to(DEV), c["sents"].to(DEV), 1e-8, g3)
    assert torch.equal(_bits(op.cpu()), _bits(ssim))


BIG = [  # N, M, ndf, ih, iw, Tw, lens
    (2, 5, 256, 17, 17, 18, [18, 11, 5, 16, 17]),          # the workload's own shape: packed, long + short, a lone last column
    (2, 4, 512, 16, 20, 32, [1, 16, 17, 32]),              # the limits: 140 KB of LDS, Tw = 32, S = 320
    (1, 3, 96, 3, 11, 7, [7, 3, 1]),                       # ndf no power of two (phase C leaves a wave idle), S = 33
]


@pytest.mark.parametrize("shape", BIG, ids=lambda s: "N%d-M%d-ndf%d-S%d-T%d" % (s[0], s[1], s[2], s[3] * s[4], s[5]))
def test_gallery_at_the_large_shapes_against_fp64(shape):
    N, M, ndf, ih, iw, Tw, lens = shape
    g = torch.Generator().manual_seed(N + 3 * ndf + 5 * Tw + 7 * ih * iw)
    regions, words = torch.randn(N, ndf, ih, iw, generator=g), torch.randn(M, ndf, Tw, generator=g)
    sim = _gallery_abi(regions, words, lens, None, 4.0, 5.0)
    R.close(sim, R.words_sim_ref(regions, words, lens, 4.0, 5.0), what="words vs fp64 restatement")
    cnn, rnn = torch.randn(N, ndf, generator=g), torch.randn(M, ndf, generator=g)
    R.close(_sent_abi(cnn, rnn, None, 1e-8, 10.0), R.sent_sim_ref(cnn, rnn, 1e-8, 10.0), what="sent vs fp64 restatement")


def test_sent_gallery_clamps_the_norm_product_at_eps():
    cnn = torch.tensor([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0]])
    rnn = torch.tensor([[1.0, 2.0, 3.0], [2e-3, 0.0, 0.0]])
    got = _sent_abi(cnn, rnn, None, 1e-4, 10.0)
    R.close(got, R.sent_sim_ref(cnn, rnn, 1e-4, 10.0), what="eps clamp")
    assert got[0].tolist() == [0.0, 0.0] and abs(got[1, 1] - 10.0 * 2e-6 / 1e-4) < 1e-6


# ---- candidate lists ----
def test_candidate_lists_repeats_order_and_empty_slots():
    """cand with repeats, arbitrary order, -1 and (ctypes takes the table as it is) entries outside [0, M): empty slots score -inf
    exactly, everything else carries the bits of the full gallery, nothing outside sim is written."""
    c = R.case("c2")
    g1, g2, g3 = R.gammas()
    lens, M = c["lens"].tolist(), c["words"].shape[0]
    full = _gallery_abi(c["regions"], c["words"], lens, None, g1, g2)
    sfull = _sent_abi(c["codes"], c["sents"], None, 1e-8, g3)
    cand = np.array([[4, 4, 0, -1, 2, 2, 1], [-1, -1, 3, 0, M, 1, -7], [2, 1, 0, 4, 3, 2 ** 31 - 1, -2 ** 31]], dtype=np.int64)
    got = _gallery_abi(c["regions"], c["words"], lens, cand, g1, g2)
    assert torch.equal(_bits(got), _bits(torch.from_numpy(R.listed(full.numpy(), cand).astype(np.float32))))
    assert (got.numpy()[(cand < 0) | (cand >= M)] == NEG_INF).all()
    sgot = _sent_abi(c["codes"], c["sents"], cand, 1e-8, g3)
    assert torch.equal(_bits(sgot), _bits(torch.from_numpy(R.listed(sfull.numpy(), cand).astype(np.float32))))
    # through the operators: a host table is range-checked ([-1, M)), a device table taken as it is
    from tgsr_amd._lib import TgsrError
    reg, wrd = c["regions"].to(DEV), c["words"].to(DEV)
    with pytest.raises(TgsrError):
        torch.ops.tgsr.damsm_gallery(reg, wrd, lens, g1, g2, torch.from_numpy(cand))
    with pytest.raises(TgsrError):
        torch.ops.tgsr.sent_gallery(c["codes"].to(DEV), c["sents"].to(DEV), 1e-8, g3, torch.from_numpy(cand))
    host = np.where((cand < 0) | (cand >= M), -1, cand)
    op = torch.ops.tgsr.damsm_gallery(reg, wrd, lens, g1, g2, torch.from_numpy(host))
    assert torch.equal(_bits(op.cpu()), _bits(got))
    op = torch.ops.tgsr.damsm_gallery(reg, wrd, lens, g1, g2, torch.from_numpy(np.clip(cand, -5, M + 5).astype(np.int32)).to(DEV))
    assert torch.equal(_bits(op.cpu()), _bits(got))


def _pairings(cand, lens, M):
    """Which kinds of column pairs a table makes the workgroups see."""
    seen = set()
    for row in np.asarray(cand):
        for q in range(0, len(row), 2):
            kinds = []
            for k in (q, q + 1):
                if k >= len(row):
                    kinds.append("none")
                elif not 0 <= row[k] < M:
                    kinds.append("empty")
                else:
                    kinds.append("short" if lens[row[k]] <= 16 else "long")
            seen.add("+".join(sorted(kinds)))
    return seen


def test_placement_independence_bitwise():
    """One gallery (Tw = 32, lengths {1, 16, 17, 32}, S = 289) scored with the columns as they are, permuted, shifted by one column
    behind an empty slot, and one pair at a time (K = 1): every (image, caption) score is the same bits in all of them, and between
    them the tables make every pairing occur: short + short (packed), short + long, long + long, short + empty, and a lone column."""
    c = R.case("c1")
    g1, g2, _ = R.gammas()
    lens, (N, M) = c["lens"].tolist(), (c["regions"].shape[0], c["words"].shape[0])
    assert lens == [1, 16, 17, 32, 16, 1, 32, 17]
    base = _gallery_abi(c["regions"], c["words"], lens, None, g1, g2)
    R.close(base, c["words_sim64"], what="placement base vs reference fp64")
    ident = np.tile(np.arange(M), (N, 1))
    tables = {
        "identity": ident,                                          # (0,1) short+short, (2,3) long+long, (4,5) short+short, (6,7)
        "shifted": np.concatenate([np.full((N, 1), -1), ident], 1),  # odd K: empty+short, short+long ..., the last column alone
        "sorted": np.tile(np.array([0, 2, 1, 3, 4, 6, 5, 7]), (N, 1)),    # short+long four times
        "per-row": np.stack([np.random.RandomState(7 + n).permutation(M) for n in range(N)]),
        "reversed-with-holes": np.tile(np.array([7, -1, 6, 5, -1, 4, 3, 2, 1, 0, 0]), (N, 1)),
    }
    seen = set()
    for tag, cand in tables.items():
        got = _gallery_abi(c["regions"], c["words"], lens, cand, g1, g2)
        want = torch.from_numpy(R.listed(base.numpy(), cand).astype(np.float32))
        assert torch.equal(_bits(got), _bits(want)), "%s: %d scores moved" % (tag, int((_bits(got) != _bits(want)).sum()))
        seen |= _pairings(cand, lens, M)
    assert {"short+short", "long+short", "long+long", "empty+short", "empty+long", "none+short"} <= seen, seen
    for m in range(M):                                              # one pair at a time: K = 1, a lone column every time
        got = _gallery_abi(c["regions"], c["words"], lens, np.full((N, 1), m), g1, g2)
        assert torch.equal(_bits(got[:, 0]), _bits(base[:, m])), m


def test_agrees_with_the_pair_kernel_on_a_square_batch():
    """tgsr_damsm_words_fwd is the only way the parent scores a gallery: same problem, within TOL_SIM (bit equality is not asked)."""
    from tgsr_amd import ops
    g = torch.Generator().manual_seed(12)
    B, ndf, Tw = 6, 64, 18
    lens = [18, 3, 16, 17, 9, 1]
    regions, words = torch.randn(B, ndf, 17, 17, generator=g).to(DEV), torch.randn(B, ndf, Tw, generator=g).to(DEV)
    pair, _att = ops.damsm_words_similarity(regions, words, lens, 4.0, 5.0, need_att=False)
    gal = ops.damsm_gallery(regions, words, lens, 4.0, 5.0)
    R.close(gal.cpu(), pair.cpu(), what="gallery vs pair kernel")
    from tgsr_amd.miscc import losses
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2 = 4.0, 5.0
    try:
        ws = losses.words_similarity(regions.requires_grad_(True), words, torch.tensor(lens), B)
        assert ws.grad_fn is None and not ws.requires_grad and torch.equal(ws, gal)
        part = losses.words_similarity(regions, words, torch.tensor(lens), 4)
        assert tuple(part.shape) == (B, 4) and torch.equal(part, gal[:, :4])
        code, sent = torch.randn(B, ndf, generator=g).to(DEV), torch.randn(B, ndf, generator=g).to(DEV)
        ss = losses.sent_similarity(code.requires_grad_(True), sent)
        assert ss.grad_fn is None and tuple(ss.shape) == (B, B)
        assert torch.equal(ss, losses.sent_similarity(code[None], sent[None]))
        R.close(ss.cpu(), R.sent_sim_ref(code.detach().cpu(), sent.cpu(), 1e-8, cfg.TRAIN.SMOOTH.GAMMA3), what="sent_similarity")
    finally:
        cfg_reset()


# ---- the rank kernel ----
def test_ranks_on_hand_made_rows():
    inf = NEG_INF
    rows = [  # (row, target)
        ([3.0, 5.0, 5.0, 5.0, 1.0], 2),            # ties before and after the target: only the one before counts -> 1
        ([2.0, 2.0, 2.0, 2.0, 2.0], 3),            # all equal -> 3
        ([2.0, 2.0, 2.0, 2.0, 2.0], 0),            # ... -> 0
        ([inf, 1.0, inf, 0.5, inf], 3),            # -inf entries (empty slots) rank behind everything -> 1
        ([inf, inf, inf, inf, inf], 4),            # ... and tie among themselves -> 4
        ([inf, 1.0, inf, 0.5, inf], 0),            # a -inf target: two finite ahead, no equal one before -> 2
        ([9.0, 8.0, 7.0, 6.0, 5.0], -1),           # target -1 -> -1
        ([9.0, 8.0, 7.0, 6.0, 5.0], 5),            # target == K -> -1
        ([1.0, 2.0, 3.0, 4.0, 5.0], 0),            # last -> 4
    ]
    sim = np.array([r for r, _ in rows], dtype=np.float32)
    target = np.array([t for _, t in rows])
    got = _ranks_abi(sim, target)
    assert got.tolist() == [1, 3, 0, 1, 4, 2, -1, -1, 4]
    assert (got == R.ranks_ref(sim, target)).all()
    op = torch.ops.tgsr.retrieval_ranks(torch.from_numpy(sim).to(DEV), _i32(target).to(DEV))
    assert op.dtype == torch.int32 and op.cpu().numpy().tolist() == got.tolist()


@pytest.mark.parametrize("K", [1, 63, 64, 65, 1000])
def test_ranks_equal_the_positions_of_a_stable_descending_sort(K):
    g = torch.Generator().manual_seed(K)
    N = 9                                                          # three workgroups, the last with one wave
    sim = torch.randint(0, max(2, K // 3), (N, K), generator=g).float()      # few distinct values: many ties
    sim[1, ::3] = NEG_INF
    target = torch.randint(0, K, (N,), generator=g)
    target[5 % N] = K - 1
    got = _ranks_abi(sim.numpy(), target.numpy())
    assert (got == R.ranks_ref(sim.numpy(), target.numpy())).all()
    order = torch.sort(sim, dim=1, descending=True, stable=True).indices
    pos = (order == target[:, None]).int().argmax(1)
    assert got.tolist() == pos.tolist()


# ---- end to end ----
def _e2e_device():
    c = R.case("e2e")
    feats = [c[k].to(DEV) for k in ("regions", "codes", "words", "sents")]
    return c, feats, c["lens"].tolist()


def test_r_precision_and_retrieval_scores_return_the_reference_ranks():
    from tgsr_amd import retrieval
    from tgsr_amd.miscc.config import cfg, cfg_reset
    c, feats, lens = _e2e_device()
    N = len(lens)
    cfg_reset()
    cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3 = R.gammas()
    try:
        for mode in retrieval.MODES:
            want = c["%s_rp_ranks" % mode].numpy()
            res = retrieval.r_precision(*feats, lens, c["cand"], mode=mode, ks=(1, 3))
            assert res["ranks"].is_cuda and res["ranks"].dtype == torch.int32 and res["ranks"].cpu().numpy().tolist() == want.tolist()
            assert res["r_precision"] == float(np.mean(want == 0)) == res["recall"][1]
            assert res["recall"][3] == float(np.mean(want < 3))
        with pytest.raises(ValueError):
            retrieval.r_precision(*feats, lens, c["cand"], mode="both")
        res = retrieval.retrieval_scores(*feats, lens, ks=(1, 5, 10))
        for mode in retrieval.MODES:
            for way in ("i2t", "t2i"):
                want = c["%s_%s_ranks" % (mode, way)].numpy()
                got = res[mode][way]
                assert got["ranks"].cpu().numpy().tolist() == want.tolist(), (mode, way)
                assert got["recall"] == {k: float(np.mean(want < k)) for k in (1, 5, 10)}
                assert got["median_rank"] == float(np.sort(want)[(N - 1) // 2] + 1)
    finally:
        cfg_reset()


class _Trunk(torch.nn.Module):
    """Stand-in for the frozen Inception trunk (tests/test_hip_train.py): image -> (features [B,768,17,17], pooled [B,2048])."""

    def __init__(self):
        super().__init__()
        self.f = torch.nn.Conv2d(3, 768, 1)
        self.p = torch.nn.Linear(3, 2048)

    def forward(self, x):
        return self.f(torch.nn.functional.adaptive_avg_pool2d(x, 17)), self.p(x.mean((2, 3)))


def test_damsm_trainer_evaluate_retrieval():
    from tgsr_amd.miscc import losses
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.train import DAMSMTrainer
    cfg_reset()
    cfg.TEXT.WORDS_NUM = 10
    cfg.TRAIN.FLAG = True
    try:
        torch.manual_seed(2)
        tr = DAMSMTrainer(40, device=DEV, trunk=_Trunk().to(DEV))
        g = torch.Generator().manual_seed(21)
        lens = [[10, 7, 4], [9, 2, 1]]
        batches = []
        for ln in lens:
            cap = torch.zeros(3, 10, dtype=torch.int64)
            for b, n in enumerate(ln):
                cap[b, :n] = torch.randint(1, 40, (n,), generator=g)
            batches.append((torch.rand(3, 3, 64, 64, generator=g).to(DEV) * 2 - 1, cap.to(DEV), ln, None))
        res = tr.evaluate_retrieval(batches, ks=(1, 2))
        assert not tr.text_encoder.training and not tr.image_encoder.training          # left in eval mode, like evaluate
        # the same six items by hand: features, then the two restored miscc.losses functions and torch's stable sort
        with torch.no_grad():
            enc = [tr.image_encoder.heads(*tr.image_encoder.run_trunk(b[0])) for b in batches]
            txt = [tr.text_encoder(b[1], b[2], tr.text_encoder.init_hidden(3)) for b in batches]
        Tw = max(t[0].shape[2] for t in txt)
        words = torch.cat([torch.nn.functional.pad(t[0], (0, Tw - t[0].shape[2])) for t in txt])
        flat = lens[0] + lens[1]
        sims = {"words": losses.words_similarity(torch.cat([e[0] for e in enc]), words, torch.tensor(flat), 6),
                "sent": losses.sent_similarity(torch.cat([e[1] for e in enc]), torch.cat([t[1] for t in txt]))}
        for mode, sim in sims.items():
            for way, s in (("i2t", sim), ("t2i", sim.t())):
                order = torch.sort(s, dim=1, descending=True, stable=True).indices.cpu()
                pos = (order == torch.arange(6)[:, None]).int().argmax(1)
                got = res[mode][way]
                assert got["ranks"].cpu().tolist() == pos.tolist(), (mode, way)
                assert got["recall"] == {k: float((pos < k).double().mean()) for k in (1, 2)}
                assert got["median_rank"] == float(pos.sort().values[2] + 1)
        few = tr.evaluate_retrieval(batches, ks=(1,), max_items=4)
        assert few["sent"]["i2t"]["ranks"].numel() == 4
        with torch.no_grad():
            five = [(f, p, b[1], b[2], None) for b, (f, p) in zip(batches, [tr.image_encoder.run_trunk(b[0]) for b in batches])]
        again = tr.evaluate_retrieval(five, ks=(1, 2))                    # the batches of evaluate_features: the same result
        assert all(torch.equal(again[m][w]["ranks"], res[m][w]["ranks"]) for m in res for w in res[m])
        with pytest.raises(ValueError):
            tr.evaluate_retrieval([])
    finally:
        cfg_reset()


def test_sr_trainer_evaluate_r_precision():
    """r_precision=None: the dict evaluate returned before, with or without an image encoder on the trainer; r_precision=K: the
    same scores plus the R-precision of the finest output against sampled candidate lists."""
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.synthetic import synthetic_batch
    from tgsr_amd.train import SRTrainer
    from tgsr_amd.util import CNN_ENCODER
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 256
    cfg.TREE.BRANCH_NUM = 4
    cfg.TREE.BASE_SIZE = 32
    try:
        torch.manual_seed(3)
        enc = CNN_ENCODER(256, trunk=_Trunk()).to(DEV).eval()
        for p in enc.parameters():
            p.requires_grad = False

        def batches(with_ids):
            for k in range(2):
                cap, lens, LR, LRb = synthetic_batch(2, seed=70 + k)
                g = torch.Generator().manual_seed(80 + k)
                hr = [(torch.rand(2, 3, s, s, generator=g) * 2 - 1).to(DEV) for s in (64, 128, 256)]
                b = (cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), hr)
                yield b + ([k, 2 + k],) if with_ids else b
        torch.manual_seed(7)
        tr = SRTrainer(41, device=DEV, image_encoder=enc)
        plain = tr.evaluate(batches(False), ema=False)
        assert sorted(plain) == ["fake", "fine"]
        res = tr.evaluate(batches(True), ema=False, r_precision=3, generator=torch.Generator().manual_seed(1))
        assert sorted(res) == ["fake", "fine", "r_precision"] and sorted(res["r_precision"]) == ["sent", "words"]
        for name in ("fine", "fake"):
            for a, b in zip(plain[name], res[name]):
                assert sorted(a) == sorted(b)
                for key in a:
                    if key == "mean":
                        assert a[key] == b[key]
                    else:
                        assert np.array_equal(a[key], b[key]), (name, key)
        for mode in ("sent", "words"):
            r = res["r_precision"][mode]
            ranks = r["ranks"].cpu().numpy()
            assert ranks.shape == (4,) and ranks.min() >= 0 and ranks.max() <= 2
            assert r["r_precision"] == float(np.mean(ranks == 0)) == r["recall"][1]
        again = tr.evaluate(batches(True), ema=False, r_precision=3, generator=torch.Generator().manual_seed(1))
        assert all(torch.equal(again["r_precision"][m]["ranks"], res["r_precision"][m]["ranks"]) for m in ("sent", "words"))
        torch.manual_seed(7)
        with pytest.raises(ValueError):
            SRTrainer(41, device=DEV).evaluate(batches(True), ema=False, r_precision=3)
    finally:
        cfg_reset()


def test_three_launches_replay_from_a_captured_graph():
    from tgsr_amd import ops
    c, feats, lens = _e2e_device()
    regions, codes, words, sents = feats
    cand = c["cand"].to(DEV)
    g1, g2, g3 = R.gammas()
    target = torch.zeros(len(lens), dtype=torch.int32, device=DEV)

    def run():
        w = ops.damsm_gallery(regions, words, lens, g1, g2, cand)
        s = ops.sent_gallery(codes, sents, 1e-8, g3, cand)
        return w, s, ops.retrieval_ranks(w, target), ops.retrieval_ranks(s, target)
    eager = [t.clone() for t in run()]                                # also the warm-up: the LDS opt-in and the cached lengths
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in out:
        t.fill_(0) if t.dtype == torch.int32 else t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(_bits(a.cpu()), _bits(b.cpu()))
    assert eager[2].cpu().numpy().tolist() == c["words_rp_ranks"].numpy().tolist()


def _gallery_call(L, a, **kw):
    p = dict(N=2, M=3, K=3, ndf=32, Tw=4, S=9, words=True, ctx=True, sim=True, cand=False)
    p.update(kw)
    w = a.place_input(torch.zeros(max(p["M"], 1), max(p["ndf"], 1), max(p["Tw"], 1)))
    c = a.place_input(torch.zeros(max(p["N"], 1), max(p["ndf"], 1), max(p["S"], 1)))
    cd = a.place_input(torch.zeros(max(p["N"], 1), max(p["K"], 1), dtype=torch.int32))
    sim = a.place_output((max(p["N"], 1), max(p["K"], 1)), written=False)
    return lambda: L.tgsr_damsm_gallery_fwd(w.ptr if p["words"] else None, None, c.ptr if p["ctx"] else None,
                                            cd.ptr if p["cand"] else None, p["N"], p["M"], p["K"], p["ndf"], p["Tw"], p["S"],
                                            4.0, 5.0, sim.ptr if p["sim"] else None, _stream())


def _sent_call(L, a, **kw):
    p = dict(N=2, M=3, K=3, ndf=8, cnn=True, rnn=True, sim=True, cand=False)
    p.update(kw)
    x, y = a.place_input(torch.zeros(2, 8)), a.place_input(torch.zeros(3, 8))
    cd = a.place_input(torch.zeros(2, 3, dtype=torch.int32))
    sim = a.place_output((2, 3), written=False)
    return lambda: L.tgsr_sent_gallery_fwd(x.ptr if p["cnn"] else None, y.ptr if p["rnn"] else None, cd.ptr if p["cand"] else None,
                                           p["N"], p["M"], p["K"], p["ndf"], 1e-8, 10.0, sim.ptr if p["sim"] else None, _stream())


def _ranks_call(L, a, **kw):
    p = dict(N=2, K=3, sim=True, target=True, rank=True)
    p.update(kw)
    s, t = a.place_input(torch.zeros(2, 3)), a.place_input(torch.zeros(2, dtype=torch.int32))
    r = a.place_output((2,), written=False, dtype=torch.int32)
    return lambda: L.tgsr_retrieval_ranks(s.ptr if p["sim"] else None, t.ptr if p["target"] else None, p["N"], p["K"],
                                          r.ptr if p["rank"] else None, _stream())


REFUSALS = [
    ("gallery ndf = 48", _gallery_call, dict(ndf=48), "EUNSUPPORTED"),
    ("gallery ndf = 544", _gallery_call, dict(ndf=544), "EUNSUPPORTED"),
    ("gallery Tw = 33", _gallery_call, dict(Tw=33), "EUNSUPPORTED"),
    ("gallery S = 321", _gallery_call, dict(S=321), "EUNSUPPORTED"),
    ("gallery K != M without a table", _gallery_call, dict(K=2), "EINVAL"),
    ("gallery words NULL", _gallery_call, dict(words=False), "EINVAL"),
    ("gallery ctx NULL", _gallery_call, dict(ctx=False), "EINVAL"),
    ("gallery sim NULL", _gallery_call, dict(sim=False), "EINVAL"),
    ("gallery N = 0", _gallery_call, dict(N=0, cand=True), "EINVAL"),
    ("gallery M = 0", _gallery_call, dict(M=0, cand=True), "EINVAL"),
    ("gallery K = 0", _gallery_call, dict(K=0, cand=True), "EINVAL"),
    ("gallery ndf = 0", _gallery_call, dict(ndf=0), "EINVAL"),
    ("sent K != M without a table", _sent_call, dict(K=2), "EINVAL"),
    ("sent cnn NULL", _sent_call, dict(cnn=False), "EINVAL"),
    ("sent rnn NULL", _sent_call, dict(rnn=False), "EINVAL"),
    ("sent sim NULL", _sent_call, dict(sim=False), "EINVAL"),
    ("sent N = 0", _sent_call, dict(N=0, cand=True), "EINVAL"),
    ("sent M = 0", _sent_call, dict(M=0, cand=True), "EINVAL"),
    ("sent K = 0", _sent_call, dict(K=0, cand=True), "EINVAL"),
    ("sent ndf = 0", _sent_call, dict(ndf=0), "EINVAL"),
    ("ranks sim NULL", _ranks_call, dict(sim=False), "EINVAL"),
    ("ranks target NULL", _ranks_call, dict(target=False), "EINVAL"),
    ("ranks rank NULL", _ranks_call, dict(rank=False), "EINVAL"),
    ("ranks N = 0", _ranks_call, dict(N=0), "EINVAL"),
    ("ranks K = 0", _ranks_call, dict(K=0), "EINVAL"),
]


def test_refusals_leave_the_output_untouched():
    M_, L = _lib()
    for name, make, kw, code in REFUSALS:
        a = Arena(DEV)
        call = make(L, a, **kw)
        assert call() == getattr(M_, code), name
        a.check()                                                  # every output was placed written=False: untouched


def test_opcheck_of_the_three_operators():
    c, feats, lens = _e2e_device()
    regions, codes, words, sents = feats
    g1, g2, g3 = R.gammas()
    basic = ("test_schema", "test_faketensor")
    chk = torch.library.opcheck
    T = torch.ops.tgsr
    cand = c["cand"].to(DEV)
    chk(T.damsm_gallery.default, (regions, words, lens, g1, g2, None), test_utils=basic)
    chk(T.damsm_gallery.default, (regions, words, lens, g1, g2, cand), test_utils=basic)
    chk(T.sent_gallery.default, (codes, sents, 1e-8, g3, None), test_utils=basic)
    chk(T.sent_gallery.default, (codes, sents, 1e-8, g3, cand), test_utils=basic)
    chk(T.retrieval_ranks.default, (T.sent_gallery(codes, sents, 1e-8, g3, cand), torch.zeros(len(lens), dtype=torch.int32, device=DEV)),
        test_utils=basic)
