"""The reduced-precision executor's launch plan, pinned to what it was before the plan was gathered into
`lp.upblock_plan` (tests/golden/lp_plan.json):

* CPU: with the operators replaced by a recorder, `LpExecutor.refresh / high_trunk / low / high_heads` run without a GPU; the
  ordered list of operator calls (name, every scalar, shape / dtype of every tensor, which activation buffer it is) of every
  case of a grid over generators, LR sizes and switches equals the recorded one.
* CPU: `lp.upblock_plan` alone over a grid of shapes and switches against the answers of the predicates it replaced.
* GPU: the `ops.profile` records (name, flops, bytes) of one eager bf16 step equal the recorded ones.

`python tests/test_lp_plan.py --write` regenerates the "cases" of the fixture with the recorder below (it uses only what the
executor keeps: the switches as module attributes, refresh / alloc / high_trunk / low / high_heads), `--write-profile` on an
MI355X its "profile".
"""
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "lp_plan.json")
T_WORDS = 18
# every torch.ops.tgsr.lp_* operator LpExecutor can launch
REACHABLE = {"lp_conv3x3", "lp_resblocks", "lp_upconv_glu", "lp_upconv_glu_head", "lp_upconv_glu_att", "lp_upconv_glu_head_att",
             "lp_stem", "lp_stem_att", "lp_convert", "lp_conv_to3", "lp_conv_to3_map", "lp_word_attention", "lp_head_combine",
             "lp_head_combine_map"}


class _Proj(list):          # trainer._ProjWithPack: the word projections of a step, with or without the attention pack
    pass


class Recorder:
    """Stands in for `lp_pipeline.C`: every operator call becomes one line of text."""

    def __init__(self):
        self.calls, self.named, self.bufs = [], [], None

    def name(self, t, label):
        self.named.append((t, label))
        return t

    def _label(self, t):
        def walk(node, path):
            if torch.is_tensor(node):
                return path if node is t else None
            items = node.items() if isinstance(node, dict) else enumerate(node) if isinstance(node, (list, tuple)) else ()
            for k, v in items:
                hit = walk(v, "%s[%s]" % (path, k) if path else str(k))
                if hit:
                    return hit
        return walk(self.bufs, "") or next((lb for o, lb in self.named if o is t), "-")

    def _show(self, a):
        if torch.is_tensor(a):
            return "%s:%s:%s" % (self._label(a), "x".join(map(str, a.shape)), str(a.dtype)[6:])
        if isinstance(a, (list, tuple)):
            return "[" + ", ".join(self._show(v) for v in a) + "]"
        return "%s%r" % (type(a).__name__[0] if a is not None else "", a)       # b True / i 3 / f 0.5 / None

    def __getattr__(self, op):
        def call(*args):
            self.calls.append("%s(%s)" % (op, ", ".join(self._show(a) for a in args)))
            x = args[0]
            if op == "lp_word_attention":
                return self.name(torch.empty(x.shape[0], args[3], x.shape[1] - 2, x.shape[2] - 2), "r%d" % (len(self.calls) - 1))
            if op in ("lp_conv_to3", "lp_conv_to3_map"):
                return self.name(torch.empty(x.shape[0], 3, x.shape[1] - 2, x.shape[2] - 2), "r%d" % (len(self.calls) - 1))
        return call


def _stub(monkeypatch, rec):
    from tgsr_amd import lp, lp_pipeline, ops
    dt = lp.torch_dtype
    monkeypatch.setattr(lp_pipeline, "C", rec)
    monkeypatch.setattr(lp, "pack_conv3x3_weight", lambda w, d: torch.empty(w.shape[0] * w.shape[1] * 9, dtype=dt(d)))
    monkeypatch.setattr(lp, "pack_upconv_weight", lambda w, d: torch.empty(w.shape[0] * w.shape[1] * 16, dtype=dt(d)))
    monkeypatch.setattr(lp, "pack_to3_weight", lambda w, d: torch.empty(int(w.shape[2]) * 512, dtype=dt(d)))
    monkeypatch.setattr(ops, "bn_fold", lambda g, b, m, v, eps: (torch.empty(g.shape[0]), torch.empty(g.shape[0])))
    monkeypatch.setattr(lp, "head_partial_elems", lambda B, H, W, K: B * (H // 8) * (W // 64 + 1) * 3 * K)
    monkeypatch.setattr(lp, "resblocks_flags", lambda B, H, W, dev: torch.zeros(B * H * W // 256, dtype=torch.int32))


_PIPES = {}


def _pipe(branch, weightmap, use_act):
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.trainer import SRPipeline
    key = (branch, weightmap, use_act)
    if key not in _PIPES:
        cfg_reset()
        cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
        _PIPES[key] = SRPipeline(41, device="cpu", dtype="bf16", branch_num=branch, weightmap=weightmap, use_act=use_act)
        cfg_reset()
    return _PIPES[key]


def grid():
    """(key, branch_num, (B, H, W), fuse_attention, FUSE_HEADS, SUBPIXEL, CHAIN, weightmap, use_act, defer_heads)"""
    sizes = [(2, 32, 32), (1, 16, 16), (1, 32, 48)]
    sw = list(itertools.product((True, False), repeat=3))
    rows = [(br, s, a, h, p, False, False, True, True) for br in (4, 5) for s in sizes for a, h, p in sw]
    rows += [(br, sizes[0], a, h, p, True, False, True, True) for br in (4, 5) for a, h, p in sw]
    rows += [(4, sizes[0], a, h, p, False, wm, act, True) for wm in (False, True) for act in (False, True) for a, h, p in sw]
    rows += [(4, s, True, True, True, False, True, act, True) for s in sizes[1:] for act in (False, True)]
    rows += [(br, s, True, True, True, False, False, True, False) for br in (4, 5) for s in sizes]     # low() finishing its own heads
    out = []
    for r in rows:
        key = "x%d %dx%dx%d att%d heads%d sub%d chain%d map%d act%d defer%d" % ((8 if r[0] == 4 else 16,) + r[1] + tuple(map(int, r[2:])))
        if key not in [k for k, _ in out]:
            out.append((key, r))
    return out


def record_case(monkeypatch, row):
    from tgsr_amd import lp_pipeline
    branch, (B, H, W), att, heads, sub, chain, weightmap, use_act, defer = row
    rec = Recorder()
    _stub(monkeypatch, rec)
    monkeypatch.setattr(lp_pipeline, "FUSE_HEADS", heads)
    monkeypatch.setattr(lp_pipeline, "SUBPIXEL", sub)
    monkeypatch.setattr(lp_pipeline, "CHAIN", chain)
    ex = _pipe(branch, weightmap, use_act)._lp
    ex.fuse_attention = att
    ex.refresh(force=True)
    bufs = rec.bufs = ex.alloc(B, H, W, "cpu")
    LR = rec.name(torch.zeros(B, 3, H, W), "LR")
    proj = _Proj(rec.name(torch.zeros(B, 32, 32), "proj[%d]" % i) for i in range(len(ex.netGL.attention_modules())))
    if att:
        proj.att_pack = rec.name(torch.zeros(4096, dtype=torch.uint8), "att_pack")
    words, mask = torch.zeros(B, 256, T_WORDS), rec.name(torch.zeros(B, T_WORDS, dtype=torch.bool), "mask")
    try:
        feats = ex.high_trunk(bufs, LR, LR)
        res = ex.low(bufs, LR, None, words, mask, ca=(None, 0, 0), proj=proj, defer_heads=defer)
        ex.high_heads(feats, res[0], res[4] if defer else None)
    except ValueError as e:
        rec.calls.append("ValueError: %s" % e)
    return rec.calls


def record_all(monkeypatch):
    return {key: record_case(monkeypatch, row) for key, row in grid()}


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_executor_launch_plan_is_the_recorded_one(monkeypatch):
    """Every case of the grid: the executor makes the recorded operator calls, in the recorded order, with the recorded
    arguments; and the grid reaches every lp_* operator the executor can launch."""
    fx = _fixture()
    table, want = fx["calls"], fx["cases"]
    keys = [k for k, _ in grid()]
    assert sorted(keys) == sorted(want), "the grid and the fixture name different cases"
    seen = set()
    for key, row in grid():
        got, exp = record_case(monkeypatch, row), [table[i] for i in want[key]]
        seen.update(c.split("(")[0] for c in got)
        for n, (g, e) in enumerate(zip(got, exp)):
            assert g == e, "%s: call %d is\n  %s\nwas\n  %s" % (key, n, g, e)
        assert len(got) == len(exp), "%s: %d calls, were %d (first extra: %s)" % (key, len(got), len(exp), (got + exp)[min(len(got), len(exp))])
    assert {s for s in seen if s.startswith("lp_")} == REACHABLE


# lp.upblock_plan against the predicates it replaced (_UpConv.sub / .fusable / .att_fusable, the branches of _UpConv.__call__ and
# the `out if k < last else None` of the executor), recorded before they were folded into it: per shape (cin, cout, Hi, Wi) one hex
# digit per case of _plan_cases(), bits = sub-pixel form 1, head fused 2, image written 4, attention fused 8
_PLAN_SHAPES = [(64, 64, 32, 32), (32, 64, 64, 64), (64, 64, 16, 16), (64, 64, 32, 48), (64, 64, 30, 32), (64, 64, 4, 32),
                (32, 64, 128, 128), (48, 64, 32, 32), (64, 128, 32, 32), (128, 64, 32, 32), (32, 32, 32, 32)]


def _plan_code(sub, head, write, att):
    return "%x" % (int(sub) + 2 * int(head) + 4 * int(write) + 8 * int(att))


def _plan_cases():
    """(K, image read after the head, attention pack, FUSE_HEADS, SUBPIXEL): 32 per shape"""
    return list(itertools.product((3, 5), (True, False), (True, False), (True, False), (True, False)))


def test_upblock_plan_answers_as_the_predicates_it_replaced():
    """lp.upblock_plan is the one launch decision of an upBlock: over the grid above it answers what _UpConv's own conditions and
    the executor's branches answered (the "upblock_plan" table of the fixture, recorded once from them; they are gone, so unlike
    "cases" it cannot be regenerated), and every plan the executor can meet is reached."""
    from tgsr_amd import lp
    want = _fixture()["upblock_plan"]
    seen = set()
    for shape in _PLAN_SHAPES:
        key = "%d,%d,%dx%d" % shape
        got = ""
        for K, read, pack, heads, sub in _plan_cases():
            p = lp.upblock_plan(*shape, K=K, image_read=read, att_pack=pack, fuse_heads=heads, subpixel=sub)
            seen.add(tuple(map(bool, p)))
            got += _plan_code(*p)
        assert len(got) == len(want[key]), key
        bad = [i for i in range(len(got)) if got[i] != want[key][i]]
        assert not bad, "%s: case %d of its grid %r: %s, was %s" % (key, bad[0], _plan_cases()[bad[0]], got[bad[0]], want[key][bad[0]])
    # every plan the executor can meet is in the grid; a head needs the sub-pixel kernel, a fused attention a written image
    assert seen == {(False, False, True, False), (True, False, True, False), (True, True, True, False), (True, True, False, False),
                    (True, False, True, True), (True, True, True, True)}
    # K = 0: no head to fuse, whatever the switch says
    assert lp.upblock_plan(64, 64, 32, 32, K=0, image_read=True, att_pack=True, fuse_heads=True, subpixel=True) == \
        lp.upblock_plan(64, 64, 32, 32, K=3, image_read=True, att_pack=True, fuse_heads=False, subpixel=True)


def _profile_of_one_step(fuse_attention):
    from oracle import tgsr_oracle as O
    from tgsr_amd import ops
    from tgsr_amd.miscc.config import cfg, cfg_reset
    from tgsr_amd.trainer import SRPipeline
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    try:
        p = SRPipeline(41, device="cuda", dtype="bf16", branch_num=4).load_state_dicts(*O.random_state(seed=3))
        p._lp.fuse_attention = fuse_attention
        cap, lens, LR, LRb = O.synthetic_batch(2, lr=32)
        args = (cap.cuda(), lens.tolist(), LR.cuda(), LRb.cuda())
        p(*args)                                    # packs the weights, allocates the buffers
        torch.cuda.synchronize()
        ops.profile = []
        try:
            p(*args)
            torch.cuda.synchronize()
            return [[r[0], float(r[1]), int(r[2])] for r in ops.profile]
        finally:
            ops.profile = None
    finally:
        cfg_reset()


@pytest.mark.gpu
def test_profile_records_of_one_bf16_step_are_the_recorded_ones():
    """bf16, the shipped x8 form, B = 2, LR 32 x 32, one eager step with the attention fused and stand-alone: the list of
    (name, flops, bytes) bench.py's roofline reads is the recorded one."""
    want = _fixture()["profile"]
    for att in (True, False):
        got, exp = _profile_of_one_step(att), want["fuse_attention=%d" % att]
        assert exp, "the fixture holds no profile"
        for n, (g, e) in enumerate(zip(got, exp)):
            assert g == e, "fuse_attention=%s: record %d is %s, was %s" % (att, n, g, e)
        assert len(got) == len(exp)


def _dump(fx, path):
    """One call, one case, one table row per line."""
    compact = lambda v: json.dumps(v, separators=(",", ":"), sort_keys=True)                       # noqa: E731
    parts = []
    for key in sorted(fx):
        v = fx[key]
        rows = [compact(e) for e in v] if isinstance(v, list) else ["%s:%s" % (json.dumps(k), compact(v[k])) for k in sorted(v)]
        parts.append("%s:%s\n%s\n%s" % (json.dumps(key), "[" if isinstance(v, list) else "{", ",\n".join(rows),
                                        "]" if isinstance(v, list) else "}"))
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")


if __name__ == "__main__":
    fx = _fixture() if os.path.exists(FIXTURE) else {}
    if "--write" in sys.argv:
        mp = pytest.MonkeyPatch()
        cases = record_all(mp)
        mp.undo()
        table = sorted({c for calls in cases.values() for c in calls})
        index = {c: i for i, c in enumerate(table)}
        fx["calls"], fx["cases"] = table, {k: [index[c] for c in v] for k, v in cases.items()}
    if "--write-profile" in sys.argv:
        fx["profile"] = {"fuse_attention=%d" % a: _profile_of_one_step(a) for a in (True, False)}
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    _dump(fx, out)
    print("%s: %d cases, %d distinct calls, calls per case %s" % (out, len(fx.get("cases", ())), len(fx.get("calls", ())),
                                                                 sorted({len(v) for v in fx.get("cases", {}).values()})))
