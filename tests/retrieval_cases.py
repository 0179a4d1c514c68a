"""Shared by tests/test_hip_retrieval.py (GPU) and tests/test_retrieval_host.py (CPU): the fixture tests/golden/retrieval.npz (the
reference's `words_similarity` / `sent_similarity` in fp32 and fp64, written by tests/golden/make_retrieval_golden.py) and plain
torch restatements of the three formulas of include/tgsr_hip.h for the shapes too large for a fixture.  The restatements are tied
to the reference on the CPU (test_retrieval_host.py: equal to the fixture's fp64 results to 1e-10)."""
import functools

import numpy as np
import torch

from conftest import load_npz

CASES = ("c0", "c1", "c2", "c3", "e2e")
TOL_SIM = (2e-5, 1e-5)        # atol, rtol: the project's bound for this arithmetic (tests/test_hip_attention_abi.py TOL_SIM)


@functools.lru_cache(maxsize=None)
def fixture():
    return load_npz("retrieval.npz")


def case(name):
    """{"regions" [N,ndf,ih,iw], "words" [M,ndf,Tw], "codes", "sents", "lens", "words_sim32" ...} as torch tensors."""
    z = fixture()
    return {k.split(".", 1)[1]: torch.from_numpy(v) for k, v in z.items() if k.startswith(name + ".")}


def gammas():
    return tuple(float(v) for v in fixture()["gammas"])


def words_sim_ref(regions, words, lens, gamma1, gamma2, dtype=torch.float64):
    """[N, M]: log sum_w exp(gamma2 cos(word_w, region context_w)) - losses.py:251-287 / GlobalAttention.py:33-74, per caption."""
    N, ndf = regions.shape[:2]
    ctx = regions.reshape(N, ndf, -1).to(dtype)
    cols = []
    for i, n in enumerate(lens):
        w = words[i, :, :n].to(dtype)                                             # [ndf, n]
        attn = torch.softmax(torch.einsum("nds,dl->nsl", ctx, w), dim=2)            # over the words of each region
        attn = torch.softmax(attn.transpose(1, 2) * gamma1, dim=2)                  # [N, n, S], over the regions of each word
        wc = torch.einsum("nds,nls->ndl", ctx, attn)                                # [N, ndf, n]
        dot = (wc * w[None]).sum(1)
        den = (wc.norm(dim=1) * w.norm(dim=0)[None]).clamp_min(1e-8)
        cols.append(torch.log(torch.exp(gamma2 * dot / den).sum(1)))
    return torch.stack(cols, 1)


def sent_sim_ref(cnn, rnn, eps, gamma3, dtype=torch.float64):
    cnn, rnn = cnn.to(dtype), rnn.to(dtype)
    norm = cnn.norm(dim=1, keepdim=True) * rnn.norm(dim=1, keepdim=True).t()
    return cnn @ rnn.t() / norm.clamp_min(eps) * gamma3


def ranks_ref(sim, target):
    """rank[n] = #{k : sim[n][k] > sim[n][t]} + #{k < t : sim[n][k] == sim[n][t]}, -1 for a target outside [0, K): numpy."""
    sim = np.asarray(sim)
    out = np.full(sim.shape[0], -1, dtype=np.int32)
    for n, t in enumerate(np.asarray(target)):
        if 0 <= t < sim.shape[1]:
            out[n] = np.sum(sim[n] > sim[n][t]) + np.sum(sim[n][:t] == sim[n][t])
    return out


def listed(sim, cand):
    """sim [N, M] gathered through a candidate table [N, K]: -inf where the slot is empty (an entry outside [0, M))."""
    sim, cand = np.asarray(sim), np.asarray(cand)
    ok = (cand >= 0) & (cand < sim.shape[1])
    return np.where(ok, np.take_along_axis(sim, np.where(ok, cand, 0).astype(np.int64), 1), -np.inf)


def close(got, ref, tol=TOL_SIM, what=""):
    atol, rtol = tol
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    err = (got - ref).abs()
    print("CLOSE %s worst |err| %.3g (atol %.3g rtol %.3g)" % (what, float(err.max()), atol, rtol))
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d of %d values beyond atol %.3g rtol %.3g, worst |err| %.3g" % (
        what, int(bad.sum()), bad.numel(), atol, rtol, float(err.max()))
