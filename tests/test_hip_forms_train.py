"""GPU: SRTrainer with NetG_highweight's other forms (weightmap=True: trainable maps a1..a3; use_act=False: heads without
Tanh) - one generator step against fp64 torch autograd through the oracle's training-mode networks (the maps' gradients
and Adam-updated values included), and the graph-replayed update against the eager one."""
import pytest
import torch

from oracle import tgsr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR_G = 1e-3


@pytest.fixture()
def cfg_train():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    yield cfg
    cfg_reset()


def _trainer(weightmap, use_act, seed=5):
    from tgsr_amd.train import SRTrainer
    torch.manual_seed(seed)
    tr = SRTrainer(41, device=DEV, lr=LR_G, weightmap=weightmap, use_act=use_act)
    if weightmap:                                     # non-constant maps (a constant map would not exercise the map)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for m in tr.netGH.maps():
                m.copy_(0.5 + 0.2 * torch.randn(m.shape, generator=g))
    return tr


def _batch(B, step=0):
    cap, lens, _LR, LRb = O.synthetic_batch(B, seed=40 + step % 2)
    g = torch.Generator().manual_seed(step)
    LR = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    hr = [torch.rand(B, 3, s, s, generator=g) * 2 - 1 for s in (64, 128, 256)]
    return cap, lens, LR, LRb, hr


@pytest.mark.parametrize("form", [(True, True), (False, False)], ids=["weightmap", "no-tanh"])
def test_generator_step_against_fp64(form, cfg_train):
    weightmap, use_act = form
    tr = _trainer(weightmap, use_act)
    tr._graph_g = False
    names = [n for n, _ in tr.netGH.named_parameters()]
    if weightmap:
        assert {"a1", "a2", "a3"} <= set(names)
        flat = {id(p) for p in tr.bucket.params}
        assert all(id(m) in flat for m in tr.netGH.maps()), "the maps are not in the flat gradient bucket"
    else:
        assert not any(n.startswith("a") for n in names)
    B = 4
    cap, lens, LR, LRb, hr = _batch(B)
    words, sent, mask = tr._text(cap.to(DEV), lens.tolist())
    sdL0 = {k: v.detach().cpu().clone() for k, v in tr.netGL.state_dict().items()}
    sdH0 = {k: v.detach().cpu().clone() for k, v in tr.netGH.state_dict().items()}
    torch.manual_seed(100)
    loss = float(tr.step(cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), [h.to(DEV) for h in hr]))
    torch.cuda.synchronize()
    # ---- fp64 torch autograd through the oracle's training-mode networks
    dbl = lambda sd: {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k
                          and "num_batches" not in k else (v.double() if v.is_floating_point() else v)) for k, v in sd.items()}
    dL, dH = dbl(sdL0), dbl(sdH0)
    w64, s64, m_ = words.detach().cpu().double(), sent.detach().cpu().double(), mask.cpu()
    i64, _a, mu, lv = O.g_sr_net_low(dL, LR.double(), s64, w64, m_, training=True)
    f64, _a2, _o = O.netg_highweight(dH, LR.double(), i64, LRb.double(), "lr", training=True, use_act=use_act)
    hr64 = [h.double() for h in hr]
    ref = O.mse(i64, hr64) + O.mse(f64, hr64) + O.kl_loss(mu, lv)
    ref.backward()
    assert abs(loss - float(ref)) <= 1e-4 * abs(float(ref)) + 1e-5, (loss, float(ref))
    worst = 0.0
    for net, ref_sd, sd0 in ((tr.netGL, dL, sdL0), (tr.netGH, dH, sdH0)):
        for k, p in net.named_parameters():
            r = ref_sd[k].grad
            assert p.grad is not None and r is not None, k
            denom = float(r.abs().max()) + 1e-12
            err = float((p.grad.detach().cpu().double() - r).abs().max()) / denom
            worst = max(worst, err)
            assert err < 1e-3, (k, err, denom)
            # the first Adam step moves every element by lr * g / (|g| + eps): lr * sign(g) wherever g is not ~0
            upd = (p.detach().cpu().double() - sd0[k].double())
            want = -LR_G * r / (r.abs() + 1e-8)
            big = r.abs() > 1e-2 * denom
            if bool(big.any()):
                assert float((upd - want)[big].abs().max()) < 0.02 * LR_G, k
            assert float((upd - want).abs().max()) < 2.05 * LR_G, k
    print("worst relative gradient error against fp64: %.3g" % worst)


@pytest.mark.parametrize("form", [(True, True), (False, False), (True, False)], ids=["weightmap", "no-tanh", "weightmap-no-tanh"])
def test_replayed_generator_update_equals_eager(form, cfg_train):
    trs = []
    for graphs in (True, False):
        tr = _trainer(*form)
        assert tr._graph_capable
        tr._graph_g = graphs
        trs.append(tr)
    out = [[], []]
    for step in range(8):
        cap, lens, LR, LRb, hr = _batch(4, step)
        for k, tr in enumerate(trs):
            torch.manual_seed(100 + step)
            out[k].append(float(tr.step(cap.to(DEV), lens.tolist(), LR.to(DEV), LRb.to(DEV), [h.to(DEV) for h in hr])))
    torch.cuda.synchronize()
    assert trs[0]._ggraphs and all(isinstance(c, dict) for c in trs[0]._ggraphs.values()), "the update was not captured"
    assert out[0] == out[1], (out[0], out[1])
    for a, b in zip((trs[0].netGL, trs[0].netGH), (trs[1].netGL, trs[1].netGH)):
        for (ka, va), (_kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(va, vb), ka
    for a, b in zip(trs[0].avg_param_G, trs[1].avg_param_G):
        assert torch.equal(a, b)
    if form[0]:
        init = _trainer(*form).netGH.maps()
        for m, m0 in zip(trs[0].netGH.maps(), init):
            assert not torch.equal(m, m0), "the replayed update did not move the maps"
