"""GPU: the distribution distances - the two entry points of csrc/tgsr_featdist.hip through ctypes (every operand in a guarded arena)
and through the `torch.ops.tgsr` operators, then featdist.py and SRTrainer.evaluate(fid=, kid=) on top of them.

    tgsr_feat_moments_add    tgsr_poly_mmd_sums (tgsr_poly_mmd_ws_elems)

Every expected value comes from the numpy fp64 model of tests/featdist_model.py.  Bounds, derived (products of widened float32 values
are exact in fp64, both sides add the same terms in fp64):
    moments   |got - ref| <= 2 n 2^-53 sum_r |x_ri x_rj| per element of outer, the same with sum_r |x_ri| for sum;
    mmd sums  |got - ref| <= 4 (D + m^2) 2^-53 sum |k| per output (a dot of D terms, a cube, a sum of m^2 terms, on both sides);
    scores    relative 1e-9 on full-rank sets (two symmetric eigendecompositions of well-conditioned matrices).
What the kernels promise beyond a bound is checked bit for bit: the same call twice, a row stride above D, a subset wherever it
stands in the table, a replay from a captured graph.
"""
import ctypes

import numpy as np
import pytest
import torch

import featdist_model as M
from arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"

MOMENT_SHAPES = [(1, 16), (3, 50), (5, 64), (37, 64), (130, 80), (48, 2048)]
MMD_SHAPES = [(1, 2, 16), (3, 5, 50), (2, 37, 64), (4, 130, 80), (2, 48, 2048)]
FULL_RANK = [(64, 200, 150), (48, 300, 300)]


def _lib():
    from tgsr_amd import _lib as L
    return L, L.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous().view(torch.int32)


def _moments_abi(x, ldx=None, base=None):
    """tgsr_feat_moments_add through ctypes into zeros (or `base` = (sum, outer)): (sum, outer) on the host, guards checked."""
    L_, L = _lib()
    n, D = x.shape
    a = Arena(DEV)
    xs = a.place_input(torch.from_numpy(x), bstride=ldx)             # rows ldx floats apart, NaN in between
    s0, o0 = base if base is not None else (torch.zeros(D, dtype=torch.float64), torch.zeros(D, D, dtype=torch.float64))
    s, o = a.place_inout(s0), a.place_inout(o0)
    rc = L.tgsr_feat_moments_add(xs.ptr, n, D, ldx if ldx is not None else D, s.ptr, o.ptr, _stream())
    assert rc == L_.OK, rc
    a.check()
    return s.read(), o.read()


def _check_moments(x, s, o, outer0=0.0):
    n, D = x.shape
    _n, ws, wo = M.moments(x)
    bs, bo = M.moment_bounds(x)
    s, o = s.numpy(), o.numpy()
    assert (np.abs(s - ws) <= bs).all(), np.abs(s - ws).max()
    blk = np.arange(D) // 64
    upper = blk[:, None] <= blk[None, :]                             # the defined elements: the block-upper part
    assert (np.abs(o - wo)[upper] <= bo[upper]).all(), (np.abs(o - wo) * upper).max()
    assert (o[~upper] == outer0).all()                               # below the block diagonal: neither read nor written


@pytest.mark.parametrize("n,D", MOMENT_SHAPES)
def test_moments_against_the_model(n, D):
    x = M.features(n, D, 100 + n)
    s, o = _moments_abi(x)
    _check_moments(x, s, o)
    if D == 50:                                                      # an asymmetric batch: a swapped row / column map cannot hide
        x = np.zeros((3, 50), dtype=np.float32)
        x[0, 1], x[0, 40], x[1, 7], x[2, 49] = 2.0, 3.0, 5.0, 7.0
        s, o = _moments_abi(x)
        want = x.astype(np.float64).T @ x.astype(np.float64)
        assert np.array_equal(o.numpy(), want) and np.array_equal(s.numpy(), x.sum(0).astype(np.float64))


def test_moments_row_stride_through_the_abi():
    x = M.features(37, 50, 7)
    s, o = _moments_abi(x, ldx=53)
    s2, o2 = _moments_abi(x)
    assert torch.equal(_bits(s), _bits(s2)) and torch.equal(_bits(o), _bits(o2))


def test_three_adds_over_row_blocks_agree_with_one():
    x = M.features(130, 80, 8)
    base = None
    for part in (x[:40], x[40:41], x[41:]):
        base = _moments_abi(part, base=base)
    _check_moments(x, *base)
    one = _moments_abi(x)
    bs, bo = M.moment_bounds(x)
    assert (np.abs(base[1].numpy() - one[1].numpy()) <= bo).all() and (np.abs(base[0].numpy() - one[0].numpy()) <= bs).all()


def _ops_moments(x, sum=None, outer=None):
    from tgsr_amd import ops
    D = x.shape[1]
    s = torch.zeros(D, dtype=torch.float64, device=DEV) if sum is None else sum
    o = torch.zeros(D, D, dtype=torch.float64, device=DEV) if outer is None else outer
    ops.feat_moments_add(x, s, o)
    return s, o


def test_the_same_call_twice_gives_equal_bits_and_a_column_slice_its_copys():
    wide = torch.from_numpy(M.features(48, 2048 + 5, 3)).to(DEV)
    view = wide[:, 3:3 + 2048]                                       # row stride 2053, a base 12 bytes off a 16-byte line
    assert not view.is_contiguous()
    a, b, c = _ops_moments(view), _ops_moments(view), _ops_moments(view.contiguous())
    for k in range(2):
        assert torch.equal(_bits(a[k]), _bits(b[k])) and torch.equal(_bits(a[k]), _bits(c[k]))
    _check_moments(view.cpu().numpy(), a[0].cpu(), a[1].cpu())


def test_mean_cov_is_symmetric_bit_for_bit():
    from tgsr_amd.featdist import FeatureMoments
    x = M.features(130, 80, 12)
    mom = FeatureMoments(80, DEV)
    for part in np.array_split(x, 3):
        mom.add(torch.from_numpy(part).to(DEV))
    mu, cov = mom.mean_cov()
    assert mom.n == 130 and torch.equal(_bits(cov), _bits(cov.t()))
    wmu, wcov = M.mean_cov(*M.moments(x))
    assert np.allclose(mu.cpu().numpy(), wmu, rtol=1e-12, atol=0) and np.allclose(cov.cpu().numpy(), wcov, rtol=1e-9, atol=1e-15)


def _tables(S, m, nx, ny, seed):
    """Row 0 the identity, row 1 the reversed order, the rest drawn without replacement."""
    rng = np.random.RandomState(seed)
    ix = np.stack([rng.permutation(nx)[:m] for _ in range(S)]).astype(np.int32)
    iy = np.stack([rng.permutation(ny)[:m] for _ in range(S)]).astype(np.int32)
    ix[0], iy[0] = np.arange(m), np.arange(m)
    if S > 1:
        ix[1], iy[1] = np.arange(m)[::-1], np.arange(m)[::-1]
    return ix, iy


def _mmd_abi(x, y, ix, iy):
    L_, L = _lib()
    (nx, D), ny, (S, m) = x.shape, y.shape[0], ix.shape
    ws = L.tgsr_poly_mmd_ws_elems(S, m)
    T = (m + 63) // 64
    assert ws == S * 3 * T * T
    a = Arena(DEV)
    xs, ys = a.place_input(torch.from_numpy(x)), a.place_input(torch.from_numpy(y))
    tx, ty = a.place_input(torch.from_numpy(ix)), a.place_input(torch.from_numpy(iy))
    work = a.place_ws(2 * ws)                                        # `ws` doubles
    out = a.place_output((S, 3), dtype=torch.float64)
    rc = L.tgsr_poly_mmd_sums(xs.ptr, nx, D, ys.ptr, ny, D, tx.ptr, ty.ptr, S, m, D, work.ptr, out.ptr, _stream())
    assert rc == L_.OK, rc
    a.check()
    return out.read().numpy()


@pytest.mark.parametrize("S,m,D", MMD_SHAPES)
def test_poly_mmd_sums_against_the_model(S, m, D):
    nx, ny = m + 3, m + 5
    x, y = M.features(nx, D, 200 + m, 0), M.features(ny, D, 300 + m, 1)
    ix, iy = _tables(S, m, nx, ny, m)
    got = _mmd_abi(x, y, ix, iy)
    want, mag = M.mmd_sums(x, y, ix, iy)
    err, bound = np.abs(got - want), M.mmd_bound(mag, m, D)
    assert (err <= bound).all(), (err / bound).max()


def test_a_subset_scores_the_same_bits_wherever_it_stands():
    m, D = 70, 50
    x, y = M.features(80, D, 21, 0), M.features(90, D, 22, 1)
    ix, iy = _tables(4, m, 80, 90, 5)
    ix[3], iy[3] = ix[2], iy[2]                                      # one subset given twice ...
    got = _mmd_abi(x, y, ix, iy)
    assert np.array_equal(got[2].view(np.int64), got[3].view(np.int64))
    alone = _mmd_abi(x, y, ix[2:3].copy(), iy[2:3].copy())           # ... and alone
    assert np.array_equal(got[2].view(np.int64), alone[0].view(np.int64))


def test_a_set_against_itself_differs_by_its_diagonal():
    from tgsr_amd import ops
    m, D = 37, 64
    x = M.features(45, D, 31)
    ix = _tables(2, m, 45, 45, 6)[0]
    xd, t = torch.from_numpy(x).to(DEV), torch.from_numpy(ix)
    got = ops.poly_mmd_sums(xd, xd, t, t).cpu().numpy()
    _want, mag = M.mmd_sums(x, x, ix, ix)
    bound = M.mmd_bound(mag, m, D)
    for s in range(2):
        diag = np.diag(M.poly_kernel(x[ix[s]], x[ix[s]])).sum()
        assert got[s, 0] == got[s, 1]
        assert abs((got[s, 2] - got[s, 0]) - diag) <= bound[s, 0] + bound[s, 2]


@pytest.mark.parametrize("D,n1,n2", FULL_RANK)
def test_scores_on_device_tensors_against_the_model(D, n1, n2):
    from tgsr_amd import featdist
    x, y = M.features(n1, D, 5, 0), M.features(n2, D, 6, 1)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    a = featdist.FeatureMoments(D, DEV).add(xd)
    b = featdist.FeatureMoments(D, DEV).add(yd[:70]).add(yd[70:])
    got, want = featdist.frechet_distance(a, b), M.frechet_of(x, y)
    print("fid %.17g model %.17g rel %.3g, eigh on %s" % (got, want, abs(got - want) / abs(want), featdist.solver_device(DEV)))
    assert abs(got - want) <= 1e-9 * abs(want)
    kd = featdist.kernel_distance(xd, featdist.FeatureBank().add(yd[:33]).add(yd[33:]), subsets=5, subset_size=100,
                                  generator=torch.Generator().manual_seed(9))
    ix, iy = featdist.subset_tables(n1, n2, 5, 100, torch.Generator().manual_seed(9))
    wk = M.kid(x, y, ix.numpy(), iy.numpy())
    print("kid %.17g model %.17g" % (kd["mean"], wk["mean"]))
    assert kd["per_subset"].is_cuda and np.allclose(kd["per_subset"].cpu().numpy(), wk["per_subset"], rtol=1e-9, atol=0)
    assert abs(kd["mean"] - wk["mean"]) <= 1e-9 * abs(wk["mean"]) and abs(kd["std"] - wk["std"]) <= 1e-9 * abs(wk["std"])


def test_fid_ranks_the_same_distribution_below_another():
    from tgsr_amd import featdist
    D = 48
    sets = [M.features(300, D, 41, 0), M.features(300, D, 42, 0), M.features(300, D, 43, 1)]
    moms = [featdist.FeatureMoments(D, DEV).add(torch.from_numpy(v).to(DEV)) for v in sets]
    same, other = featdist.frechet_distance(moms[0], moms[1]), featdist.frechet_distance(moms[0], moms[2])
    assert 0 <= same < other
    kid = [featdist.kernel_distance(torch.from_numpy(sets[0]).to(DEV), torch.from_numpy(v).to(DEV), 4, 200,
                                    torch.Generator().manual_seed(1))["mean"] for v in sets[1:]]
    assert kid[0] < kid[1]


def _moments_call(L, a, **kw):
    p = dict(n=3, D=8, ldx=8, x=True, sum=True, outer=True)
    p.update(kw)
    x = a.place_input(torch.ones(3, 8))
    s = a.place_output((8,), written=False, dtype=torch.float64)
    o = a.place_output((8, 8), written=False, dtype=torch.float64)
    return lambda: L.tgsr_feat_moments_add(x.ptr if p["x"] else None, p["n"], p["D"], p["ldx"], s.ptr if p["sum"] else None,
                                           o.ptr if p["outer"] else None, _stream())


def _mmd_call(L, a, **kw):
    p = dict(S=2, m=3, D=8, ldx=8, ldy=8, nx=4, ny=4, x=True, y=True, ix=True, iy=True, work=True, out=True)
    p.update(kw)
    x, y = a.place_input(torch.ones(4, 8)), a.place_input(torch.ones(4, 8))
    tx, ty = a.place_input(torch.zeros(2, 3, dtype=torch.int32)), a.place_input(torch.zeros(2, 3, dtype=torch.int32))
    work = a.place_output((12,), written=False)
    out = a.place_output((2, 3), written=False, dtype=torch.float64)
    return lambda: L.tgsr_poly_mmd_sums(x.ptr if p["x"] else None, p["nx"], p["ldx"], y.ptr if p["y"] else None, p["ny"], p["ldy"],
                                        tx.ptr if p["ix"] else None, ty.ptr if p["iy"] else None, p["S"], p["m"], p["D"],
                                        work.ptr if p["work"] else None, out.ptr if p["out"] else None, _stream())


REFUSALS = [
    ("moments ldx < D", _moments_call, dict(ldx=7)),
    ("moments n = 0", _moments_call, dict(n=0)),
    ("moments D = 0", _moments_call, dict(D=0, ldx=0)),
    ("moments x NULL", _moments_call, dict(x=False)),
    ("moments sum NULL", _moments_call, dict(sum=False)),
    ("moments outer NULL", _moments_call, dict(outer=False)),
    ("mmd m = 1", _mmd_call, dict(m=1)),
    ("mmd S = 0", _mmd_call, dict(S=0)),
    ("mmd D = 0", _mmd_call, dict(D=0)),
    ("mmd ldx < D", _mmd_call, dict(ldx=7)),
    ("mmd ldy < D", _mmd_call, dict(ldy=7)),
    ("mmd nx = 0", _mmd_call, dict(nx=0)),
    ("mmd x NULL", _mmd_call, dict(x=False)),
    ("mmd y NULL", _mmd_call, dict(y=False)),
    ("mmd ix NULL", _mmd_call, dict(ix=False)),
    ("mmd iy NULL", _mmd_call, dict(iy=False)),
    ("mmd work NULL", _mmd_call, dict(work=False)),
    ("mmd out NULL", _mmd_call, dict(out=False)),
]


def test_refusals_leave_the_outputs_untouched():
    L_, L = _lib()
    assert L.tgsr_poly_mmd_ws_elems(0, 5) == 0 and L.tgsr_poly_mmd_ws_elems(3, 1) == 0
    for name, make, kw in REFUSALS:
        a = Arena(DEV)
        call = make(L, a, **kw)
        assert call() == L_.EINVAL, name
        a.check()                                                    # every output was placed written=False: untouched


def test_ops_refuse_before_any_launch():
    from tgsr_amd import ops
    from tgsr_amd._lib import TgsrError
    x = torch.ones(5, 8, device=DEV)
    s, o = torch.full((8,), 3.0, dtype=torch.float64, device=DEV), torch.full((8, 8), 4.0, dtype=torch.float64, device=DEV)
    t = torch.tensor([[0, 1, 2]])
    cases = [
        lambda: ops.feat_moments_add(x.double(), s, o),                                   # a float64 x
        lambda: ops.feat_moments_add(x, s[:7], o),                                        # a sum of the wrong length
        lambda: ops.feat_moments_add(x, s, o[:, :7]),
        lambda: ops.feat_moments_add(x, s.float(), o),
        lambda: ops.poly_mmd_sums(x, x, torch.tensor([[0, 1, 5]]), t),                    # an index equal to nx
        lambda: ops.poly_mmd_sums(x, x, t, torch.tensor([[0, -1, 2]])),
        lambda: ops.poly_mmd_sums(x, x, torch.tensor([[0]]), torch.tensor([[0]])),       # m = 1
        lambda: ops.poly_mmd_sums(x, x[:, :7], t, t),
        lambda: ops.poly_mmd_sums(x.double(), x, t, t),
        lambda: ops.poly_mmd_sums(x, x, t, torch.tensor([[0, 1, 2, 3]])),
    ]
    for k, case in enumerate(cases):
        with pytest.raises(TgsrError):
            case()
            pytest.fail("case %d ran" % k)
    torch.cuda.synchronize()
    assert bool((s == 3.0).all()) and bool((o == 4.0).all())


def test_the_launches_replay_from_a_captured_graph():
    from tgsr_amd import ops
    x = torch.from_numpy(M.features(48, 200, 51, 0)).to(DEV)
    y = torch.from_numpy(M.features(70, 200, 52, 1)).to(DEV)
    ix, iy = (torch.from_numpy(t).to(DEV) for t in _tables(3, 40, 48, 70, 7))
    s, o = torch.zeros(200, dtype=torch.float64, device=DEV), torch.zeros(200, 200, dtype=torch.float64, device=DEV)

    def run():
        ops.feat_moments_add(x, s, o)
        return ops.poly_mmd_sums(x, y, ix, iy)
    eager = [t.clone() for t in (run(), s, o)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    s.zero_(); o.zero_(); out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (out, s, o)):
        assert torch.equal(_bits(a.cpu()), _bits(b.cpu()))
    _check_moments(x.cpu().numpy(), s.cpu(), o.cpu())


def test_opcheck_of_the_two_operators():
    x = torch.from_numpy(M.features(20, 50, 61, 0)).to(DEV)
    y = torch.from_numpy(M.features(22, 50, 62, 1)).to(DEV)
    ix, iy = (torch.from_numpy(t).to(DEV) for t in _tables(2, 10, 20, 22, 8))
    s, o = torch.zeros(50, dtype=torch.float64, device=DEV), torch.zeros(50, 50, dtype=torch.float64, device=DEV)
    basic = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.tgsr.feat_moments_add.default, (x, s, o), test_utils=basic)
    torch.library.opcheck(torch.ops.tgsr.poly_mmd_sums.default, (x, y, ix, iy), test_utils=basic)


class _Encoder(torch.nn.Module):
    """Stand-in for CNN_ENCODER with a narrow trunk: run_trunk(image) -> (features [B,768,17,17], pooled [B,8]), heads -> (region
    features [B,256,17,17], code [B,256]).  pooled is a ReLU of a full-rank map of the image's 2 x 2 average pool and of its
    absolute value's (noise and a smooth image differ there), so that 20 images give a covariance of full rank - the condition under
    which a Frechet distance is determined to 1e-9 (test_featdist_host.py)."""

    def __init__(self):
        super().__init__()
        self.f, self.p = torch.nn.Conv2d(3, 768, 1), torch.nn.Linear(24, 8)
        self.hf, self.hc = torch.nn.Conv2d(768, 256, 1), torch.nn.Linear(8, 256)
        self.trunk_calls = 0

    def run_trunk(self, x):
        self.trunk_calls += 1
        pool = torch.nn.functional.adaptive_avg_pool2d
        local = torch.cat([8.0 * pool(x, 2), pool(x.abs(), 2)], 1).flatten(1)     # the mean and the contrast of each quadrant
        return self.f(pool(x, 17)), torch.relu(self.p(local) + 1.0)

    def heads(self, features, pooled):
        return self.hf(features), self.hc(pooled)

    def forward(self, x):
        return self.heads(*self.run_trunk(x))


def test_sr_trainer_evaluate_fid_kid(tmp_path):
    from tgsr_amd import featdist
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.synthetic import synthetic_batch
    from tgsr_amd.train import SRTrainer
    from tgsr_amd.trainer import SRPipeline
    cfg_reset()
    cfg.GAN.GF_DIM = 32
    cfg.TEXT.EMBEDDING_DIM = 256
    cfg.TREE.BRANCH_NUM = 4
    cfg.TREE.BASE_SIZE = 32
    NB, B = 5, 4
    try:
        torch.manual_seed(3)
        enc = _Encoder().to(DEV).eval()
        for p in enc.parameters():
            p.requires_grad = False

        def batches(with_ids=False):
            for k in range(NB):
                cap, lens, LR, LRb = synthetic_batch(B, seed=70 + k)
                g = torch.Generator().manual_seed(80 + k)
                hr = [(torch.rand(B, 3, s, s, generator=g) * 2 - 1).to(DEV) for s in (64, 128, 256)]
                b = (cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), hr)
                yield b + ([B * k + i for i in range(B)],) if with_ids else b
        torch.manual_seed(7)
        tr = SRTrainer(41, device=DEV, image_encoder=enc)
        state = [p.detach().clone() for p in tr.params] + [b.detach().clone() for m in (tr.netGL, tr.netGH) for b in m.buffers()]
        plain = tr.evaluate(batches(), ema=False)
        assert sorted(plain) == ["fake", "fine"] and enc.trunk_calls == 0
        kid_arg = {"subsets": 4, "subset_size": 12}
        res = tr.evaluate(batches(), ema=False, fid=True, kid=kid_arg, generator=torch.Generator().manual_seed(1))
        assert sorted(res) == ["fake", "fid", "fine", "kid"] and enc.trunk_calls == 2 * NB
        for name in ("fine", "fake"):                                # the PSNR / SSIM rows: bit for bit those of the plain call
            for a, b in zip(plain[name], res[name]):
                assert sorted(a) == sorted(b)
                for key in a:
                    assert a[key] == b[key] if key in ("mean", "n") else np.array_equal(a[key], b[key]), (name, key)
        after = [p.detach() for p in tr.params] + [b.detach() for m in (tr.netGL, tr.netGH) for b in m.buffers()]
        assert len(state) == len(after) and all(torch.equal(a, b) for a, b in zip(state, after))

        # the same features by hand: the pipeline's outputs through the encoder, then the model
        pipe = SRPipeline.from_modules(tr.text_encoder, tr.netGL, tr.netGH, device=DEV)
        fx, fy, moments = [], [], None
        with torch.no_grad(), tr._eval_weights(False):              # eval mode, the current weights: what evaluate(ema=False) runs
            for cap, lens, LR, LRb, hr in batches():
                out = pipe(cap, lens, LR, LRb)
                fx.append(enc.run_trunk(out["fine"][-1])[1].cpu().numpy())
                fy.append(enc.run_trunk(hr[-1])[1].cpu().numpy())
                moments = pipe.realism(out, hr[-1], enc, moments)
        fx, fy = np.concatenate(fx), np.concatenate(fy)
        want = M.frechet_of(fx, fy)
        print("evaluate fid %.17g model %.17g rel %.3g" % (res["fid"]["fine"], want, abs(res["fid"]["fine"] - want) / abs(want)))
        assert res["fid"]["n"] == NB * B and abs(res["fid"]["fine"] - want) <= 1e-9 * abs(want)
        assert featdist.frechet_distance(*moments) == res["fid"]["fine"]                  # SRPipeline.realism: the same moments
        ix, iy = featdist.subset_tables(NB * B, NB * B, 4, 12, torch.Generator().manual_seed(1))
        wk = M.kid(fx, fy, ix.numpy(), iy.numpy())
        print("evaluate kid %.17g model %.17g" % (res["kid"]["mean"], wk["mean"]))
        assert np.allclose(res["kid"]["per_subset"].cpu().numpy(), wk["per_subset"], rtol=1e-9, atol=0)
        assert abs(res["kid"]["mean"] - wk["mean"]) <= 1e-9 * abs(wk["mean"])

        # the ground-truth side from saved statistics: the same value, and no trunk walk for it
        path = moments[1].save(str(tmp_path / "gt.npz"))
        for saved in (path, featdist.FeatureMoments.load(path, DEV)):
            enc.trunk_calls = 0
            again = tr.evaluate(batches(), ema=False, fid=saved)
            assert again["fid"] == res["fid"] and enc.trunk_calls == NB and "kid" not in again
        # with r_precision as well, the SR image is walked once: NB walks for fid=<saved>, 2 NB with the ground truth's
        enc.trunk_calls = 0
        both = tr.evaluate(batches(True), ema=False, r_precision=3, fid=path, generator=torch.Generator().manual_seed(1))
        assert enc.trunk_calls == NB and both["fid"] == res["fid"]
        enc.trunk_calls = 0
        only = tr.evaluate(batches(True), ema=False, r_precision=3, generator=torch.Generator().manual_seed(1))
        assert enc.trunk_calls == NB and sorted(only) == ["fake", "fine", "r_precision"]
        for mode in ("sent", "words"):
            assert torch.equal(only["r_precision"][mode]["ranks"], both["r_precision"][mode]["ranks"])
        torch.manual_seed(7)
        bare = SRTrainer(41, device=DEV)
        for kw in (dict(fid=True), dict(kid=True), dict(kid={"subsets": 2})):
            with pytest.raises(ValueError):
                bare.evaluate(batches(), ema=False, **kw)
        with pytest.raises(ValueError):
            tr.evaluate(batches(), ema=False, kid={"subset": 3})
    finally:
        cfg_reset()
