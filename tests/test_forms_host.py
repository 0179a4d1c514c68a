"""CPU: selecting NetG_highweight's form through SRPipeline / SRTrainer's constructors (no kernel runs) and the C ABI of the
map / identity head epilogues."""
import pytest
import torch


@pytest.fixture()
def cfg_small():
    from tgsr_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    cfg.GAN.GF_DIM, cfg.TEXT.EMBEDDING_DIM = 32, 256
    yield cfg
    cfg_reset()


@pytest.mark.parametrize("weightmap,use_act", [(False, True), (True, True), (False, False), (True, False)])
def test_pipeline_builds_every_x8_form(weightmap, use_act, cfg_small):
    from tgsr_amd.trainer import SRPipeline
    p = SRPipeline(41, device="cpu", branch_num=4, weightmap=weightmap, use_act=use_act)
    gh = p.netGH
    assert gh.weightmap == weightmap and gh.useAct == use_act
    assert any(isinstance(m, torch.nn.Tanh) for m in gh.conv_output) == use_act
    keys = set(gh.state_dict())
    assert ({"a1", "a2", "a3"} <= keys) == weightmap and "a" not in keys
    if weightmap:
        assert [tuple(m.shape) for m in gh.maps()] == [(64, 64), (128, 128), (256, 256)]


def test_pipeline_refuses_the_forms_it_cannot_build(cfg_small):
    from tgsr_amd.trainer import SRPipeline
    for dt in ("fp32", "bf16", "f16"):
        with pytest.raises(ValueError, match="tanh-free"):
            SRPipeline(41, device="cpu", dtype=dt, branch_num=5, use_act=False)
    for dt in ("bf16", "f16"):
        with pytest.raises(ValueError, match="16 x 16"):
            SRPipeline(41, device="cpu", dtype=dt, branch_num=5, weightmap=True)
    p = SRPipeline(41, device="cpu", branch_num=5, weightmap=True)          # fp32 builds the x16 weight-map form
    assert [tuple(m.shape) for m in p.netGH.maps()] == [(32, 32), (64, 64), (128, 128), (256, 256)]


def test_map_entry_points_are_in_the_binding():
    import os
    import re
    from conftest import ROOT
    from tgsr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tgsr_hip.h")).read(), flags=re.S)
    for name in ("tgsr_lp_head_combine_map", "tgsr_lp_conv_to3_map_fwd"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SIGNATURES
    assert _lib.ACT_IDENT_AXPY == 2 and re.search(r"#define TGSR_ACT_IDENT_AXPY 2\b", src)
