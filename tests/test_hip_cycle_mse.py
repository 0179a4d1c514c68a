"""GPU: the cycle-consistency objective on the kernels of csrc/tgsr_cycle_mse.hip - through ctypes (every operand in a guarded
arena), through the `torch.ops.tgsr` operators, through miscc.losses and through SRTrainer.

    tgsr_cycle_mse_ws_elems    tgsr_cycle_mse_fwd    tgsr_cycle_mse_bwd

Bounds, against the fp64 model of tests/cycle_mse_cases.py (F.interpolate on doubles).  torch's own float32 CPU run lies 1e-8 ...
3e-7 (relative) from that model in the loss, <= 1.1e-7 of max|grad| in the gradients at integer ratios - where the weights are exact
constants - and <= 1.1e-6 of max|grad| at non-integer ratios and when up-scaling, where float32 source coordinates move the weights
themselves.  About ten times that for another summation order:
    loss, per-scale terms                         rel. error <= 1e-5
    gradients, integer ratios                     |err| <= 1e-5 |ref| + 1e-6 max|ref|
    gradients, non-integer ratios / up-scaling    |err| <= 1e-5 |ref| + 1e-5 max|ref|
A dropped or doubled corner tap moves a gradient by >= 2 % of its maximum.  Nothing here reads the reference."""
import ctypes

import numpy as np
import pytest
import torch

import cycle_mse_cases as K
from arena import Arena
from conftest import FP32_TOL, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-5
ATOL_INT, ATOL_ANY = 1e-6, 1e-5          # x max|ref|


@pytest.fixture(scope="module")
def golden():
    return load_npz("cycle_mse.npz")


def _lib():
    from tgsr_amd import _lib as M
    return M, M.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tgsr_ops():
    from tgsr_amd import custom_ops  # noqa: F401  (registers torch.ops.tgsr.*)
    return torch.ops.tgsr


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _ptrs(regions):
    return (ctypes.c_void_p * len(regions))(*[None if r is None else r.address for r in regions])


def _grad_close(got, ref, atol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    top = float(ref.abs().max())
    err = (got - ref).abs()
    print("  %s: max err %.3g of max|ref| %.3g (%.3g)" % (what, float(err.max()), top, float(err.max()) / max(top, 1e-300)))
    bad = err > RTOL * ref.abs() + atol * top
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), top)


def _rel_close(got, ref, what):
    got, ref = float(got), float(ref)
    print("  %s: %.9g against %.9g, rel err %.3g" % (what, got, ref, abs(got - ref) / abs(ref)))
    assert abs(got - ref) <= RTOL * abs(ref), (what, got, ref)


# ------------------------------------------------------------------------------------------------ through the C ABI
def _abi(srs, lr, skew=0, grad=0.75):
    """tgsr_cycle_mse_fwd + _bwd through ctypes in a guarded arena (`skew`: every float operand that many words off its 16-byte
    boundary): (loss, terms, diff, [d_sr], d_lr) on the host."""
    M_, L = _lib()
    n, (B, C, h, w) = len(srs), lr.shape
    Hs, Ws = _ints([s.shape[2] for s in srs]), _ints([s.shape[3] for s in srs])
    n_ws = L.tgsr_cycle_mse_ws_elems(Hs, Ws, n, B, C, h, w)
    assert n_ws >= n
    a = Arena(DEV)
    s_in = [a.place_input(s, skew=skew) for s in srs]
    l_in = a.place_input(lr, skew=skew)
    g = a.place_input(torch.tensor([grad], dtype=torch.float32))
    ws = a.place_ws(n_ws)
    diff = a.place_output((n, B, C, h, w), skew=skew)
    loss, terms = a.place_output((1,)), a.place_output((n,))
    d_sr = [a.place_output(tuple(s.shape), skew=skew) for s in srs]
    d_lr = a.place_output((B, C, h, w), skew=skew)
    rc = L.tgsr_cycle_mse_fwd(_ptrs(s_in), Hs, Ws, n, l_in.ptr, B, C, h, w, ws.ptr, diff.ptr, loss.ptr, terms.ptr, _stream())
    assert rc == M_.OK, rc
    rc = L.tgsr_cycle_mse_bwd(g.ptr, diff.ptr, Hs, Ws, n, B, C, h, w, _ptrs(d_sr), d_lr.ptr, _stream())
    assert rc == M_.OK, rc
    a.check()
    return loss.read()[0], terms.read(), diff.read(), [d.read() for d in d_sr], d_lr.read()


def _check(res, ref, grad, atol, what, exact_zeros=False):
    loss, terms, _diff, d_sr, d_lr = res
    l64, t64, g_sr, g_lr = ref
    print(what)
    _rel_close(loss, l64, "loss")
    for i in range(len(d_sr)):
        _rel_close(terms[i], t64[i], "term %d" % i)
        _grad_close(d_sr[i], grad * g_sr[i], atol, "d_sr[%d]" % i)
        if exact_zeros:         # integer ratios: where no tap lands (or only a zero weight) the gradient is 0, not small
            assert torch.equal(d_sr[i] == 0, g_sr[i] == 0), (what, i)
    _grad_close(d_lr, grad * g_lr, atol, "d_lr")


def _same_bits(x, y):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x, y))


def _flat(res):
    loss, terms, diff, d_sr, d_lr = res
    return [loss.reshape(1), terms, diff, d_lr] + d_sr


INTEGER = [
    ((6, 10), (3, 5)),        # ratio 2: the taps -1 and 2h clamp onto the edge pixels, W no multiple of 4
    ((16, 24), (4, 6)),       # ratio 4
    ((32, 48), (4, 6)),       # ratio 8: 3/4 of the SR pixels receive zeros
    ((12, 15), (4, 5)),       # ratio 3: t = 0, a single tap
    ((4, 6), (4, 6)),         # the identity
    ((8, 20), (4, 5)),        # ratio 2 down, 4 across
]
ANY = [
    ((10, 14), (4, 5)),       # 2.5 and 2.8
    ((23, 17), (4, 5)),       # 5.75 and 3.4
    ((3, 4), (7, 9)),         # up-scaling: several LR outputs per SR pixel
    ((1, 1), (3, 3)),         # all sixteen taps collapse onto one pixel
    ((2, 2), (5, 3)),         # a 2-pixel side
]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("sr,lr", INTEGER)
def test_cycle_mse_abi_integer_ratios_against_fp64(sr, lr, skew):
    srs, l, ref = K.seeded_case((sr,), lr)
    res = _abi(srs, l, skew=skew)
    _check(res, ref, 0.75, ATOL_INT, "%dx%d -> %dx%d skew=%d" % (sr + lr + (skew,)), exact_zeros=True)
    assert _same_bits(_flat(res), _flat(_abi(srs, l, skew=skew)))          # two runs, the same bits


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("sr,lr", ANY)
def test_cycle_mse_abi_any_ratio_against_fp64(sr, lr, skew):
    srs, l, ref = K.seeded_case((sr,), lr)
    res = _abi(srs, l, skew=skew)
    _check(res, ref, 0.75, ATOL_ANY, "%dx%d -> %dx%d skew=%d" % (sr + lr + (skew,)))
    assert _same_bits(_flat(res), _flat(_abi(srs, l, skew=skew)))


THREE = (((8, 12), (16, 24), (32, 48)), (4, 6))                                                        # ratios 2 / 4 / 8
EIGHT = (((8, 10), (16, 20), (12, 15), (4, 5), (8, 20), (10, 14), (23, 17), (3, 4)), (4, 5))           # every kind in one call


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("sizes,lr,B,C,atol", [THREE + (2, 3, ATOL_INT), EIGHT + (2, 3, ATOL_ANY), (((6, 10),), (3, 5), 1, 1, ATOL_INT)])
def test_cycle_mse_abi_scale_counts_and_layout(sizes, lr, B, C, atol, skew):
    """Three and eight scales in ONE call (loss[0] = the sum of the terms in scale order), and B = 1, C = 1."""
    srs, l, ref = K.seeded_case(sizes, lr, B, C)
    res = _abi(srs, l, skew=skew)
    _check(res, ref, 0.75, atol, "%d scales -> %dx%d B=%d C=%d skew=%d" % (len(sizes), lr[0], lr[1], B, C, skew))
    total = np.float32(0)
    for t in res[1].numpy():
        total = np.float32(total + t)
    assert float(res[0]) == float(total)                                   # fp32, in scale order
    assert _same_bits(_flat(res), _flat(_abi(srs, l, skew=skew)))


def test_cycle_mse_abi_backward_writes_only_what_is_asked():
    """NULL entries of d_sr and a NULL d_lr: the other outputs hold the same bits as in the full call."""
    M_, L = _lib()
    srs, l, _ref = K.seeded_case(*THREE)
    full = _abi(srs, l)
    n, (B, C, h, w) = 3, l.shape
    Hs, Ws = _ints([s.shape[2] for s in srs]), _ints([s.shape[3] for s in srs])
    a = Arena(DEV)
    diff = a.place_input(full[2])
    g = a.place_input(torch.tensor([0.75]))
    d1 = a.place_output(tuple(srs[1].shape))
    skipped = [a.place_output(tuple(srs[i].shape), written=False) for i in (0, 2)]
    d_lr = a.place_output((B, C, h, w), written=False)
    assert L.tgsr_cycle_mse_bwd(g.ptr, diff.ptr, Hs, Ws, n, B, C, h, w, _ptrs([None, d1, None]), None, _stream()) == M_.OK
    a.check()
    assert torch.equal(d1.read(), full[3][1]) and len(skipped) == 2 and d_lr.kind == "absent"
    b = Arena(DEV)
    diff, g, d_lr = b.place_input(full[2]), b.place_input(torch.tensor([0.75])), b.place_output((B, C, h, w))
    assert L.tgsr_cycle_mse_bwd(g.ptr, diff.ptr, Hs, Ws, n, B, C, h, w, None, d_lr.ptr, _stream()) == M_.OK
    b.check()
    assert torch.equal(d_lr.read(), full[4])


# ------------------------------------------------------------------------------------------------ full size, once each
def test_cycle_mse_abi_at_the_training_shape_once():
    """B = 16, 64^2 / 128^2 / 256^2 -> 32^2: 49 152 LR pixels per scale (192 workgroups each), 3 145 728 SR pixels at the last scale -
    786 432 runs of four against a backward segment capped at 1024 workgroups of 256: three turns of its loop."""
    srs, l, ref = K.seeded_case(((64, 64), (128, 128), (256, 256)), (32, 32), 16, 3)
    _check(_abi(srs, l), ref, 0.75, ATOL_INT, "training shape", exact_zeros=True)


def test_cycle_mse_abi_past_the_grid_caps_once():
    """B = 2, 512^2 -> 128^2: 98 304 LR pixels against a forward capped at 256 workgroups per scale (some take a second turn, the
    finish kernel adds one partial per thread), 393 216 runs against the backward's 262 144 per turn."""
    _M, L = _lib()
    assert L.tgsr_cycle_mse_ws_elems(_ints([512]), _ints([512]), 1, 2, 3, 128, 128) == 256 < 2 * 3 * 128 * 128 // 256
    srs, l, ref = K.seeded_case(((512, 512),), (128, 128))
    _check(_abi(srs, l), ref, 0.75, ATOL_INT, "512x512 -> 128x128", exact_zeros=True)


# ------------------------------------------------------------------------------------------------ refusals
def test_cycle_mse_abi_refusals_leave_the_outputs_alone():
    M_, L = _lib()
    srs, l, _ref = K.seeded_case(((8, 12), (16, 24)), (4, 6))
    n, (B, C, h, w) = 2, l.shape
    a = Arena(DEV)
    s_in = [a.place_input(s) for s in srs]
    l_in = a.place_input(l)
    g = a.place_input(torch.ones(1))
    d_in = a.place_input(torch.zeros(n, B, C, h, w))
    outs = {k: a.place_output(s, written=False) for k, s in (("ws", (64,)), ("diff", (n, B, C, h, w)), ("loss", (1,)), ("terms", (n,)),
                                                               ("d0", tuple(srs[0].shape)), ("d1", tuple(srs[1].shape)),
                                                               ("d_lr", (B, C, h, w)))}
    o = {k: v.ptr for k, v in outs.items()}
    st = _stream()
    H0, W0 = [8, 16], [12, 24]
    nine = dict(sr=_ptrs((s_in * 5)[:9]), H=_ints([8] * 9), W=_ints([12] * 9), n=9)

    def fwd(sr=_ptrs(s_in), H=_ints(H0), W=_ints(W0), n=n, lr=l_in.ptr, B=B, C=C, h=h, w=w, ws=o["ws"], diff=o["diff"], loss=o["loss"],
            terms=o["terms"]):
        return L.tgsr_cycle_mse_fwd(sr, H, W, n, lr, B, C, h, w, ws, diff, loss, terms, st)

    def bwd(grad=g.ptr, diff=d_in.ptr, H=_ints(H0), W=_ints(W0), n=n, B=B, C=C, h=h, w=w, d_sr=_ptrs([outs["d0"], outs["d1"]]),
            d_lr=o["d_lr"], **_):
        return L.tgsr_cycle_mse_bwd(grad, diff, H, W, n, B, C, h, w, d_sr, d_lr, st)

    shapes = [dict(n=0), dict(n=-1), nine, dict(B=0), dict(C=0), dict(h=0), dict(w=0), dict(H=_ints([0, 16])), dict(W=_ints([12, 0])),
              dict(H=_ints([8, -4])), dict(h=65537), dict(W=_ints([12, 65537]))]
    bad = [fwd(**{k: None}) for k in ("sr", "H", "W", "lr", "ws", "diff", "loss", "terms")] + [fwd(**s) for s in shapes]
    bad += [fwd(sr=_ptrs([s_in[0], None]))]
    bad += [bwd(**{k: None}) for k in ("grad", "diff", "H", "W")] + [bwd(**s) for s in shapes]
    bad += [bwd(d_sr=None, d_lr=None), bwd(d_sr=_ptrs([None, None]), d_lr=None)]
    assert all(rc == M_.EINVAL for rc in bad), bad
    for s in shapes:
        kw = dict(dict(H=_ints(H0), W=_ints(W0), n=n, B=B, C=C, h=h, w=w), **{k: v for k, v in s.items() if k != "sr"})
        assert L.tgsr_cycle_mse_ws_elems(kw["H"], kw["W"], kw["n"], kw["B"], kw["C"], kw["h"], kw["w"]) == 0, s
    assert L.tgsr_cycle_mse_ws_elems(None, _ints(W0), n, B, C, h, w) == 0 and L.tgsr_cycle_mse_ws_elems(_ints(H0), None, n, B, C, h, w) == 0
    assert L.tgsr_cycle_mse_ws_elems(_ints(H0), _ints(W0), n, B, C, h, w) == n
    a.check()                                                          # every output still holds its prefill


# ------------------------------------------------------------------------------------------------ operators, autograd, miscc.losses
def test_opcheck_cycle_mse_operators():
    T = _tgsr_ops()
    srs, l, _ref = K.seeded_case(*THREE)
    srs, l = [s.to(DEV) for s in srs], l.to(DEV)
    basic = ("test_schema", "test_faketensor")
    chk = torch.library.opcheck
    chk(T.cycle_mse.default, (srs, l), test_utils=basic)
    chk(T.cycle_mse.default, (srs[:1], l), test_utils=basic)
    _loss, _terms, diff = T.cycle_mse(srs, l)
    g = torch.ones((), device=DEV)
    sizes = [v for s in srs for v in s.shape[2:]]
    chk(T.cycle_mse_bwd.default, (g, diff, sizes, [True, True, True], True), test_utils=basic)
    chk(T.cycle_mse_bwd.default, (g, diff, sizes, [False, True, False], False), test_utils=basic)
    chk(T.cycle_mse_bwd.default, (g, diff, sizes, [False, False, False], True), test_utils=basic)


def _atol(name):
    return ATOL_INT if name == "down" else ATOL_ANY


@pytest.mark.parametrize("name", K.FIXTURE_CASES)
def test_cycle_mse_loss_against_the_fixture_and_fp64(golden, name):
    """miscc.losses.CycleMSE on HIP tensors - the kernels (autograd.CycleMSE) and, with fused=False, the torch composition on the
    device - against the reference's run and the fp64 model; the two forms against each other under an upstream gradient that is
    not 1."""
    from tgsr_amd.miscc import losses
    g, atol = golden, _atol(name)
    l64, t64, g_sr, g_lr = K.cycle_mse_fp64(*K.fixture_inputs(g, name))
    got = {}
    for fused in (None, False):
        srs, lr = K.fixture_inputs(g, name, DEV)
        for t in srs + [lr]:
            t.requires_grad_(True)
        loss = losses.CycleMSE(srs, lr, fused=fused)
        assert loss.grad_fn is not None and (type(loss.grad_fn).__name__ == "CycleMSEBackward") == (fused is None)
        (0.37 * loss).backward()
        print("CycleMSE %s fused=%s: %.9g, reference %.9g, fp64 %.9g" % (name, fused, float(loss.detach()), float(g[name + ".loss"]), float(l64)))
        _rel_close(loss.detach(), l64, "loss against fp64")
        _rel_close(loss.detach(), g[name + ".loss"], "loss against the fixture")
        for i, s in enumerate(srs):
            _grad_close(s.grad, 0.37 * g_sr[i], atol, "d_sr[%d] fp64" % i)
            _grad_close(s.grad, 0.37 * torch.from_numpy(g["%s.g_sr%d" % (name, i)]), atol, "d_sr[%d] fixture" % i)
        _grad_close(lr.grad, 0.37 * g_lr, atol, "d_lr fp64")
        _grad_close(lr.grad, 0.37 * torch.from_numpy(g[name + ".g_lr"]), atol, "d_lr fixture")
        got[fused] = (loss.detach(), [s.grad for s in srs], lr.grad)
    _rel_close(got[None][0], got[False][0], "kernels against the composition")
    for i, (x, y) in enumerate(zip(got[None][1], got[False][1])):
        _grad_close(x, y, atol, "d_sr[%d] kernels against the composition" % i)
    _grad_close(got[None][2], got[False][2], atol, "d_lr kernels against the composition")
    # the per-scale terms, and a second run: the same bits
    from tgsr_amd.autograd import CycleMSE
    srs, lr = K.fixture_inputs(g, name, DEV)
    loss2, terms = CycleMSE.apply(lr, *srs)
    assert torch.equal(loss2, got[None][0]) and terms.grad_fn is None
    np.testing.assert_allclose(terms.cpu().numpy(), t64.numpy(), rtol=RTOL)
    np.testing.assert_allclose(terms.cpu().numpy(), g[name + ".terms"], rtol=RTOL)


def test_cycle_mse_loss_only_the_asked_gradients():
    """A gradient into one SR image only, and into the LR image only: the same bits as in the full backward."""
    from tgsr_amd.miscc import losses
    srs, l, _ref = K.seeded_case(*THREE)
    srs, l = [s.to(DEV) for s in srs], l.to(DEV)
    full = torch.autograd.grad(losses.CycleMSE([s.requires_grad_(True) for s in srs], l.requires_grad_(True)), srs + [l])
    srs, l = [s.detach() for s in srs], l.detach()
    one = srs[1].clone().requires_grad_(True)
    g1, = torch.autograd.grad(losses.CycleMSE([srs[0], one, srs[2]], l), [one])
    ll = l.clone().requires_grad_(True)
    g2, = torch.autograd.grad(losses.CycleMSE(srs, ll), [ll])
    assert torch.equal(g1, full[1]) and torch.equal(g2, full[3])
    assert losses.CycleMSE(srs, l).grad_fn is None


def test_cycle_mse_loss_on_offset_views():
    """Dense tensors whose first element sits one float off a 16-byte boundary are taken by the kernels: the same values."""
    from tgsr_amd.miscc import losses
    srs, l, (l64, _t, g_sr, _g) = K.seeded_case(*THREE)
    off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)]).to(DEV)[1:].view(t.shape)            # noqa: E731
    so = [off(s).requires_grad_(True) for s in srs]
    assert all(s.data_ptr() % 16 == 4 for s in so)
    loss = losses.CycleMSE(so, off(l))
    assert type(loss.grad_fn).__name__ == "CycleMSEBackward"
    loss.backward()
    aligned = losses.CycleMSE([s.to(DEV) for s in srs], l.to(DEV))
    assert torch.equal(loss.detach(), aligned)
    _rel_close(loss.detach(), l64, "loss on offset views")
    for i, s in enumerate(so):
        _grad_close(s.grad, g_sr[i], ATOL_INT, "d_sr[%d] offset" % i)
    # a strided view is not dense: the composition takes it, quietly and correctly
    wide = torch.zeros(2, 3, 8, 16, device=DEV)
    wide[..., :12] = srs[0].to(DEV)
    comp = losses.CycleMSE([wide[..., :12]], l.to(DEV))
    _rel_close(comp, K.cycle_mse_fp64(srs[:1], l)[0], "strided view through the composition")


# ------------------------------------------------------------------------------------------------ SRTrainer
def _trainer_setup():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.synthetic import synthetic_batch
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    cap, lens, LR, LRb = synthetic_batch(2, seed=5)
    g = torch.Generator().manual_seed(1)
    hr = [(torch.rand(2, 3, s, s, generator=g) * 2 - 1).to(DEV) for s in (64, 128, 256)]
    return cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), hr


def test_srtrainer_step_with_the_cycle_term(monkeypatch):
    """One step of SRTrainer(cycle=0.5) against the same step with CycleMSE forced to its torch composition: the loss and the flat
    gradient bucket within FP32_TOL.  The operators are counted: the default trainer's step goes through tgsr::cycle_mse twice (the
    two generators' pyramids, three scales each in one call) and its backward twice, the forced one through neither; and the term is
    there: the loss differs from a trainer's without it."""
    from tgsr_amd import custom_ops
    from tgsr_amd.miscc.config import cfg_reset
    from tgsr_amd.train import SRTrainer
    batch = _trainer_setup()
    calls = {}
    for name in ("cycle_mse", "cycle_mse_bwd"):
        def counted(*a, _op=getattr(custom_ops, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _op(*a)
        monkeypatch.setattr(custom_ops, name, counted)
    try:
        res = []
        for cycle, fused in ((0.5, None), (0.5, False), (0.0, None)):
            torch.manual_seed(7)
            tr = SRTrainer(41, device=DEV, cycle=cycle)
            tr.cycle_fused = fused
            torch.manual_seed(9)
            calls.clear()
            errG = tr.step(*batch)
            assert calls == ({"cycle_mse": 2, "cycle_mse_bwd": 2} if (cycle and fused is None) else {}), (cycle, fused, calls)
            res.append((float(errG), tr.bucket.flat.clone()))
        (la, ga), (lb, gb), (lc, _gc) = res
        print("trainer: errG %.7g fused / %.7g composed / %.7g without the term, bucket max diff %.3g of %.3g"
              % (la, lb, lc, float((ga - gb).abs().max()), float(gb.abs().max())))
        assert np.isfinite(la) and bool(torch.isfinite(ga).all()) and la > lc + 1e-3
        assert abs(la - lb) <= FP32_TOL * max(1.0, abs(lb))
        assert float((ga - gb).abs().max()) <= FP32_TOL * float(gb.abs().max())
    finally:
        cfg_reset()


def test_srtrainer_replayed_cycle_step_equals_the_eager_one(monkeypatch):
    """TGSR_GRAPH_G=1: with cycle=0.5 the generators' update is still captured (`_g_graphs` returns a capture), and after the
    warm-up and two replayed updates the parameters, running statistics and EMA copies equal the eager trainer's bit for bit."""
    from tgsr_amd import train
    from tgsr_amd.miscc.config import cfg_reset
    cap, lens, LR, LRb, hr = _trainer_setup()
    monkeypatch.setenv("TGSR_GRAPH_G", "1")
    try:
        trs = []
        for graphs in (True, False):
            torch.manual_seed(5)
            tr = train.SRTrainer(41, device=DEV, cycle=0.5)
            assert tr._graph_capable
            if not graphs:
                tr._graph_g = False
            trs.append(tr)
        out = [[], []]
        for step in range(train.GRAPH_G_WARMUP + 2):
            g = torch.Generator().manual_seed(step)
            lr_k = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(DEV)          # a new LR input every step: the capture reads its buffer
            for k, tr in enumerate(trs):
                torch.manual_seed(100 + step)
                out[k].append(float(tr.step(cap, lens, lr_k, LRb, hr)))
        torch.cuda.synchronize()
        caps = list(trs[0]._ggraphs.values())
        assert caps and all(isinstance(c, dict) for c in caps), "the update was not captured: %r" % (caps,)
        assert not trs[1]._ggraphs
        assert out[0] == out[1], out
        for a, b in zip((trs[0].netGL, trs[0].netGH), (trs[1].netGL, trs[1].netGH)):
            for (ka, va), (_kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
                assert torch.equal(va, vb), ka
        for a, b in zip(trs[0].avg_param_G, trs[1].avg_param_G):
            assert torch.equal(a, b)
    finally:
        cfg_reset()


def test_srtrainer_cycle_zero_is_the_trainer_without_the_argument():
    """cycle=0.0 (the default): CycleMSE is not called, the LR input is not kept, and loss and gradients equal those of a trainer built
    without the argument bit for bit."""
    from tgsr_amd.miscc import losses
    from tgsr_amd.miscc.config import cfg_reset
    from tgsr_amd.train import SRTrainer
    batch = _trainer_setup()
    try:
        res = []
        for kw in ({}, {"cycle": 0.0}):
            torch.manual_seed(7)
            tr = SRTrainer(41, device=DEV, **kw)
            torch.manual_seed(9)
            errG = tr.step(*batch)
            assert tr._lr_in is None and tr.cycle == 0.0
            res.append((errG.clone(), tr.bucket.flat.clone()))
            with torch.no_grad():
                torch.manual_seed(11)
                fake, fine, mu, logvar, _w, _s = tr.forward_G(*batch[:4])
                assert torch.equal(tr._pixel_kl(fake, fine, mu, logvar, batch[4]),
                                   losses.MSE(fake, batch[4]) + losses.MSE(fine, batch[4]) + losses.KL_loss(mu, logvar))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    finally:
        cfg_reset()
