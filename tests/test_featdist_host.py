"""CPU: the distribution distances of tgsr_amd/featdist.py on host tensors (their torch fp64 form) against the numpy model of
tests/featdist_model.py, and the model itself against scipy.linalg.sqrtm.

Bounds.  The model's Frechet distance against sqrtm: relative 1e-9 on full-rank inputs (the two agree to about 1e-14 there), relative
1e-6 on the rank-deficient case (about 1e-8; there sqrtm is the less accurate side, which is why the eigh form is the definition).
featdist against the model: relative 1e-9 on the full-rank cases, 1e-6 on the rank-deficient one (the same reason).  Moments: 2 n 2^-53 sum |terms| per element (featdist_model.moment_bounds)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import featdist_model as M

FULL_RANK = [(64, 200, 150), (48, 300, 300)]
RANK_DEFICIENT = (64, 37, 41)


def _sets(D, n1, n2, seed=5):
    return M.features(n1, D, seed, 0), M.features(n2, D, seed + 1, 1)


def _sqrtm_frechet(x, y):
    import scipy.linalg
    (m1, c1), (m2, c2) = M.mean_cov(*M.moments(x)), M.mean_cov(*M.moments(y))
    root = scipy.linalg.sqrtm(c1 @ c2)
    d = m1 - m2
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(root).real)


def _moments_of(x, device="cpu", blocks=1):
    from tgsr_amd.featdist import FeatureMoments
    mom = FeatureMoments(x.shape[1], device)
    for part in np.array_split(x, blocks):
        mom.add(torch.from_numpy(part).to(device))
    return mom


@pytest.mark.parametrize("D,n1,n2", FULL_RANK)
def test_model_frechet_equals_sqrtm_on_full_rank_sets(D, n1, n2):
    x, y = _sets(D, n1, n2)
    got, want = M.frechet_of(x, y), _sqrtm_frechet(x, y)
    print("model %.17g sqrtm %.17g rel %.3g" % (got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-9 * abs(want)


def test_model_frechet_equals_sqrtm_on_a_rank_deficient_set():
    x, y = _sets(*RANK_DEFICIENT)
    got, want = M.frechet_of(x, y), _sqrtm_frechet(x, y)
    print("model %.17g sqrtm %.17g rel %.3g" % (got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("D,n1,n2", FULL_RANK + [RANK_DEFICIENT])
def test_frechet_distance_on_cpu_tensors_equals_the_model(D, n1, n2):
    from tgsr_amd.featdist import frechet_distance
    x, y = _sets(D, n1, n2)
    a, b = _moments_of(x), _moments_of(y, blocks=3)
    assert (a.n, b.n) == (n1, n2)
    want = M.frechet_of(x, y)
    got = frechet_distance(a, b)
    # full rank: 1e-9.  Rank deficient (n - 1 < D): the D - n + 1 zero eigenvalues come out of any solver as +-c u |M|, their roots
    # as sqrt(c u) |M|^(1/2) ~ 1e-8 - two correct evaluations (two LAPACK builds, thread counts) differ by that much, so the case
    # is held to the 1e-6 that the model-against-sqrtm test above holds it to
    tol = 1e-9 if min(n1, n2) > D else 1e-6
    assert abs(got - want) <= tol * abs(want), (got, want)
    mu, cov = a.mean_cov()
    assert torch.equal(cov, cov.t())
    wmu, wcov = M.mean_cov(*M.moments(x))
    assert np.allclose(mu.numpy(), wmu, rtol=1e-12, atol=0) and np.allclose(cov.numpy(), wcov, rtol=1e-9, atol=1e-15)
    # a set against itself: rounding size, either sign, not clamped.  An eigenvalue of A^T S A that is exactly 0 comes out of the
    # solver as some c u |A^T S A| <= c u tr(S)^2 (c = 64 allowed), its root as sqrt(c u) tr(S); there are at most D of them, twice.
    self_d = frechet_distance(a, a)
    assert abs(self_d) <= 2 * D * np.sqrt(64 * M.U) * float(torch.trace(cov))


def test_frechet_needs_two_rows_and_equal_width():
    from tgsr_amd.featdist import FeatureMoments, frechet_distance
    one = FeatureMoments(8, "cpu").add(torch.rand(1, 8))
    two = FeatureMoments(8, "cpu").add(torch.rand(5, 8))
    with pytest.raises(ValueError):
        frechet_distance(one, two)
    with pytest.raises(ValueError):
        frechet_distance(two, FeatureMoments(9, "cpu").add(torch.rand(5, 9)))
    with pytest.raises(ValueError):
        two.add(torch.rand(5, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        two.add(torch.rand(5, 7))


def test_merge_of_two_halves_equals_one_add():
    from tgsr_amd.featdist import FeatureMoments
    x = M.features(130, 80, 9)
    whole = _moments_of(x)
    a, b = _moments_of(x[:61]), _moments_of(x[61:])
    merged = FeatureMoments(80, "cpu").merge([a, b])
    also = _moments_of(x[:61]).merge(b)
    n, s, o = M.moments(x)
    bs, bo = M.moment_bounds(x)
    for mom in (whole, merged, also):
        assert mom.n == n
        assert (np.abs(mom.sum.numpy() - s) <= bs).all()
        assert (np.abs(mom.outer_full().numpy() - o) <= bo).all()
    assert torch.equal(merged.outer, also.outer) and torch.equal(merged.sum, also.sum)


def test_save_load_round_trips_the_bits(tmp_path):
    from tgsr_amd.featdist import FeatureMoments, frechet_distance
    mom = _moments_of(M.features(37, 50, 2))
    path = mom.save(os.path.join(tmp_path, "gt_stats.npz"))
    assert os.path.basename(path) == "gt_stats.npz" and os.path.exists(path)
    back = FeatureMoments.load(path, "cpu")
    assert back.n == mom.n and back.D == mom.D
    assert torch.equal(back.sum, mom.sum) and torch.equal(back.outer, mom.outer)
    again = FeatureMoments(50, "cpu").load_state_dict(mom.state_dict())
    assert again.n == 37 and torch.equal(again.outer, mom.outer)
    other = _moments_of(M.features(40, 50, 3, 1))
    assert frechet_distance(back, other) == frechet_distance(mom, other)
    with pytest.raises(ValueError):
        FeatureMoments(49, "cpu").load_state_dict(mom.state_dict())


def test_kernel_distance_on_cpu_tensors_equals_the_model():
    from tgsr_amd.featdist import FeatureBank, kernel_distance, subset_tables
    x, y = _sets(48, 90, 70)
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    got = kernel_distance(tx, ty, subsets=6, subset_size=40, generator=torch.Generator().manual_seed(4))
    ix, iy = subset_tables(90, 70, 6, 40, torch.Generator().manual_seed(4))
    want = M.kid(x, y, ix.numpy(), iy.numpy())
    assert abs(got["mean"] - want["mean"]) <= 1e-9 * abs(want["mean"])
    assert abs(got["std"] - want["std"]) <= 1e-9 * abs(want["std"])
    assert np.allclose(got["per_subset"].numpy(), want["per_subset"], rtol=1e-9, atol=0)
    # subset_size is clipped to the smaller set; a bank of batches is the concatenated set
    bank = FeatureBank().add(tx[:50]).add(tx[50:])
    assert len(bank) == 90
    clipped = kernel_distance(bank, ty, subsets=3, subset_size=1000, generator=torch.Generator().manual_seed(8))
    ix, iy = subset_tables(90, 70, 3, 70, torch.Generator().manual_seed(8))
    want = M.kid(x, y, ix.numpy(), iy.numpy())
    assert np.allclose(clipped["per_subset"].numpy(), want["per_subset"], rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        kernel_distance(tx[:1], ty)
    with pytest.raises(ValueError):
        kernel_distance(tx, torch.zeros(5, 47))


def test_kernel_distance_draws_the_same_tables_from_the_same_generator():
    from tgsr_amd.featdist import kernel_distance, subset_tables
    a = subset_tables(30, 25, 4, 10, torch.Generator().manual_seed(11))
    b = subset_tables(30, 25, 4, 10, torch.Generator().manual_seed(11))
    c = subset_tables(30, 25, 4, 10, torch.Generator().manual_seed(12))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    for t, n in zip(a, (30, 25)):
        assert t.dtype == torch.int32 and tuple(t.shape) == (4, 10) and 0 <= int(t.min()) and int(t.max()) < n
        assert all(len(set(row.tolist())) == 10 for row in t)           # without replacement
    x, y = (torch.from_numpy(v) for v in _sets(16, 30, 25))
    r1 = kernel_distance(x, y, 4, 10, torch.Generator().manual_seed(11))
    r2 = kernel_distance(x, y, 4, 10, torch.Generator().manual_seed(11))
    assert r1["mean"] == r2["mean"] and torch.equal(r1["per_subset"], r2["per_subset"])


def test_check_subset_table_refuses_on_the_host():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    good = ops.check_subset_table(torch.tensor([[0, 4], [3, 1]]), 5)
    assert good.dtype == torch.int32 and good.is_contiguous()
    for bad in (torch.tensor([[0, 5]]), torch.tensor([[-1, 2]]), torch.tensor([[1], [2]]), torch.tensor([0, 1]),
                torch.tensor([[0.0, 1.0]])):
        with pytest.raises(TgsrError):
            ops.check_subset_table(bad, 5)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from tgsr_amd import parallel
    from tgsr_amd.featdist import FeatureMoments
    parallel.init_distributed("gloo")
    x = M.features(75, 40, 6)
    lo, hi = (0, 44) if rank == 0 else (44, 75)                        # uneven shards
    mom = FeatureMoments(40, "cpu").add(torch.from_numpy(x[lo:hi]))
    mom.all_reduce()
    q.put((rank, mom.n, mom.sum.numpy(), mom.outer_full().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_leaves_the_moments_of_the_union_on_both_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=120) for _ in ps), key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    x = M.features(75, 40, 6)
    n, s, o = M.moments(x)
    bs, bo = M.moment_bounds(x)
    for rank, gn, gs, go in res:
        assert gn == n
        assert (np.abs(gs - s) <= bs).all() and (np.abs(go - o) <= bo).all()
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])
