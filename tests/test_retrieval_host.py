"""CPU: what text-image retrieval (tgsr_amd/retrieval.py, csrc/tgsr_retrieval.hip) does on the host, and what
tests/test_hip_retrieval.py rests on.

  * `sample_candidates`: own caption first, no candidate of the image's class, no duplicates, -1 fill, deterministic under a seed;
  * the host range check of a CPU candidate table;
  * the three C entry points are declared, bound and exported, and refuse bad arguments before any HIP call;
  * `miscc.losses.sent_similarity` / `words_similarity` exist with the reference's signatures and refuse CPU tensors loudly;
  * the fixture: the reference's own fp32 run is within 1e-6 of its fp64 run (so TOL_SIM measures the kernel), the test-side
    restatements of the formulas equal the reference's fp64 results, every target score of the end-to-end case is >= 1e-3 away
    from every other candidate's, and the recorded ranks are the rank formula's.
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import retrieval_cases as R


def _L():
    from tgsr_amd import _lib
    return _lib, _lib.lib()


# ---- sample_candidates ----
def test_sample_candidates_properties():
    from tgsr_amd.retrieval import sample_candidates
    ids = [0, 1, 2, 0, 1, 2, 3, 3, 4, 0, 1, 5]
    N, K = len(ids), 6
    t = sample_candidates(ids, K, torch.Generator().manual_seed(3))
    assert t.dtype == torch.int32 and tuple(t.shape) == (N, K) and not t.is_cuda
    for n in range(N):
        row = t[n].tolist()
        assert row[0] == n
        assert -1 not in row                                              # every class leaves >= 8 captions of other classes
        assert len(set(row)) == K
        assert all(ids[c] != ids[n] for c in row[1:])
    assert torch.equal(t, sample_candidates(ids, K, torch.Generator().manual_seed(3)))
    assert torch.equal(t, sample_candidates(torch.tensor(ids), K, torch.Generator().manual_seed(3)))
    assert not torch.equal(t, sample_candidates(ids, K, torch.Generator().manual_seed(4)))


def test_sample_candidates_fills_with_minus_one():
    from tgsr_amd.retrieval import sample_candidates
    ids = [7, 7, 7, 8, 9]                                                 # class 7 sees two others, classes 8 and 9 four
    t = sample_candidates(ids, 4, torch.Generator().manual_seed(0))
    for n in range(3):
        assert t[n, 0] == n and sorted(t[n, 1:3].tolist()) == [3, 4] and t[n, 3] == -1
    for n in (3, 4):
        row = t[n].tolist()
        assert row[0] == n and -1 not in row and len(set(row)) == 4 and n not in row[1:]
    one = sample_candidates([1, 1], 3)
    assert one.tolist() == [[0, -1, -1], [1, -1, -1]]
    assert sample_candidates([1, 2, 3], 1).tolist() == [[0], [1], [2]]
    with pytest.raises(ValueError):
        sample_candidates([], 3)
    with pytest.raises(ValueError):
        sample_candidates([1, 2], 0)


# ---- the host check of a CPU candidate table ----
def test_host_candidate_table_is_range_checked():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    good = torch.tensor([[0, 4, -1], [3, 3, 0]], dtype=torch.int64)
    out = ops.check_candidates(good, 2, 5)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.tolist() == good.tolist()
    assert ops.check_candidates(good.to(torch.int32).t().contiguous().t(), 2, 5).is_contiguous()
    for bad in (torch.tensor([[0, 5, 1], [0, 0, 0]]), torch.tensor([[0, -2, 1], [0, 0, 0]])):
        with pytest.raises(TgsrError, match=r"\[-1, 5\)"):
            ops.check_candidates(bad, 2, 5)
    with pytest.raises(TgsrError):
        ops.check_candidates(good, 3, 5)                                  # N rows expected
    with pytest.raises(TgsrError):
        ops.check_candidates(good.float(), 2, 5)
    with pytest.raises(TgsrError):
        ops.check_candidates(torch.zeros(2, 0, dtype=torch.int32), 2, 5)


# ---- the ABI ----
ENTRIES = {"tgsr_damsm_gallery_fwd": 14, "tgsr_sent_gallery_fwd": 11, "tgsr_retrieval_ranks": 6}


def test_abi_bindings_exist():
    M, L = _L()
    for name, nargs in ENTRIES.items():
        assert name in M.SIGNATURES and len(M.SIGNATURES[name][1]) == nargs and M.SIGNATURES[name][0] is ctypes.c_int
        assert hasattr(L, name)
    import tgsr_amd.custom_ops  # noqa: F401
    have = {str(s) for s in torch._C._jit_get_all_schemas() if s.name.startswith("tgsr::")}
    for s in ("tgsr::damsm_gallery(Tensor img_features, Tensor words_emb, int[] cap_lens, float gamma1, float gamma2, "
              "Tensor? cand=None) -> Tensor",
              "tgsr::sent_gallery(Tensor cnn_code, Tensor rnn_code, float eps, float gamma3, Tensor? cand=None) -> Tensor",
              "tgsr::retrieval_ranks(Tensor sim, Tensor target) -> Tensor"):
        assert s in have, s


def test_entry_points_refuse_before_any_hip_call():
    """No device here: every refusal below returns from the argument check, the pointers (host memory) are never followed."""
    M, L = _L()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    g = L.tgsr_damsm_gallery_fwd
    ok = dict(words=p, lens=None, ctx=p, cand=p, N=2, M=3, K=2, ndf=32, Tw=4, S=9)

    def gallery(**kw):
        a = dict(ok, **kw)
        return g(a["words"], a["lens"], a["ctx"], a["cand"], a["N"], a["M"], a["K"], a["ndf"], a["Tw"], a["S"], 4.0, 5.0,
                 kw.get("sim", p), None)
    for kw in (dict(words=None), dict(ctx=None), dict(sim=None), dict(N=0), dict(M=0), dict(K=0), dict(ndf=0), dict(Tw=0), dict(S=0),
               dict(cand=None, K=2)):
        assert gallery(**kw) == M.EINVAL, kw
    for kw in (dict(ndf=48), dict(ndf=544), dict(Tw=33), dict(S=321)):
        assert gallery(**kw) == M.EUNSUPPORTED, kw
    s = L.tgsr_sent_gallery_fwd
    assert s(None, p, p, 2, 3, 2, 8, 1e-8, 10.0, p, None) == M.EINVAL
    assert s(p, None, p, 2, 3, 2, 8, 1e-8, 10.0, p, None) == M.EINVAL
    assert s(p, p, p, 2, 3, 2, 8, 1e-8, 10.0, None, None) == M.EINVAL
    assert s(p, p, None, 2, 3, 2, 8, 1e-8, 10.0, p, None) == M.EINVAL                  # K != M without a table
    for n, m, k, d in ((0, 3, 2, 8), (2, 0, 2, 8), (2, 3, 0, 8), (2, 3, 2, 0)):
        assert s(p, p, p, n, m, k, d, 1e-8, 10.0, p, None) == M.EINVAL
    r = L.tgsr_retrieval_ranks
    assert r(None, p, 2, 3, p, None) == r(p, None, 2, 3, p, None) == r(p, p, 2, 3, None, None) == M.EINVAL
    assert r(p, p, 0, 3, p, None) == r(p, p, 2, 0, p, None) == M.EINVAL
    assert all(v == 0.0 for v in buf)


# ---- the restored miscc.losses names ----
def test_losses_names_exist_and_refuse_cpu_tensors():
    from tgsr_amd._lib import TgsrError
    from tgsr_amd.miscc import losses
    assert list(inspect.signature(losses.sent_similarity).parameters) == ["cnn_code", "rnn_code", "eps"]
    assert inspect.signature(losses.sent_similarity).parameters["eps"].default == 1e-8
    assert list(inspect.signature(losses.words_similarity).parameters) == ["img_features", "words_emb", "cap_lens", "batch_size"]
    with pytest.raises(TgsrError):
        losses.sent_similarity(torch.zeros(3, 8), torch.zeros(3, 8))
    with pytest.raises(TgsrError):
        losses.words_similarity(torch.zeros(2, 32, 3, 3), torch.zeros(2, 32, 4), torch.tensor([4, 2]), 2)
    with pytest.raises(ValueError):
        losses.words_similarity(torch.zeros(2, 32, 3, 3), torch.zeros(2, 32, 4), torch.tensor([4, 2]), 3)
    from tgsr_amd import ops
    with pytest.raises(TgsrError):
        ops.retrieval_ranks(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TgsrError):
        ops.sent_gallery(torch.zeros(2, 3), torch.zeros(2, 3), 1e-8, 10.0)
    with pytest.raises(TgsrError):
        ops.damsm_gallery(torch.zeros(2, 32, 3, 3), torch.zeros(2, 32, 4), [4, 2], 4.0, 5.0)


# ---- the fixture and the restatements ----
@pytest.mark.parametrize("name", R.CASES)
def test_fixture_fp32_is_near_fp64_and_the_restatements_are_the_reference(name):
    c = R.case(name)
    g1, g2, g3 = R.gammas()
    for key in ("words_sim", "sent_sim"):
        assert c[key + "32"].dtype == torch.float32 and c[key + "64"].dtype == torch.float64
        assert float((c[key + "32"].double() - c[key + "64"]).abs().max()) < 1e-6
    w = R.words_sim_ref(c["regions"], c["words"], c["lens"].tolist(), g1, g2)
    s = R.sent_sim_ref(c["codes"], c["sents"], 1e-8, g3)
    assert float((w - c["words_sim64"]).abs().max()) < 1e-10
    assert float((s - c["sent_sim64"]).abs().max()) < 1e-10


def test_fixture_covers_the_kernel_branches():
    shapes = {n: R.case(n) for n in R.CASES}
    assert tuple(shapes["c0"]["regions"].shape) == (3, 32, 3, 3) and tuple(shapes["c0"]["words"].shape) == (5, 32, 1)
    assert sorted(set(shapes["c1"]["lens"].tolist())) == [1, 16, 17, 32] and shapes["c1"]["words"].shape[2] == 32
    S = {n: c["regions"].shape[2] * c["regions"].shape[3] for n, c in shapes.items()}
    assert (S["c0"], S["c1"], S["c2"], S["c3"]) == (9, 289, 33, 320)


def test_fixture_targets_are_separated_and_ranks_follow_the_formula():
    c = R.case("e2e")
    N = c["codes"].shape[0]
    diag, zero = np.arange(N), np.zeros(N, dtype=np.int64)
    cand = c["cand"].numpy()
    assert (cand[:, 0] == diag).all() and (cand == -1).any() and cand.min() == -1 and cand.max() < N
    nontrivial = 0
    for mode in ("words", "sent"):
        sim = c[mode + "_sim64"].numpy()
        for tag, m, t in (("i2t", sim, diag), ("t2i", sim.T, diag), ("rp", R.listed(sim, cand), zero)):
            for n in range(N):
                d = np.abs(np.delete(m[n], t[n]) - m[n][t[n]])
                assert d[np.isfinite(d)].min() >= 1e-3, (mode, tag, n)
            ranks = R.ranks_ref(m, t)
            assert (ranks == c["%s_%s_ranks" % (mode, tag)].numpy()).all()
            nontrivial += int((ranks > 0).sum())
    assert nontrivial > 0                                                 # a gallery in which everything ranks first tests nothing
