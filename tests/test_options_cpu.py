"""CPU: launch variants of the Python package are plain attributes of the objects (INTEGRATION.md "Variant fields"): no module
reads the process environment, the defaults hold whatever the environment says, and every option that changes a captured launch
sequence is part of the key its graph is cached under."""
import glob
import os

import torch

from cosyvoice_amd.config import FlowConfig, HiftConfig, LlmConfig

PKG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cosyvoice_amd")

# every variable the package used to read, at the value that used to select the non-default variant
RETIRED = {"CV_DOWN_KSPLIT": "1", "CV_SPLIT_NORM": "0", "CV_LLM_STAGE_ABI": "0", "CV_SPLIT_QKV_NORM": "1", "CV_FLOW_FUSED": "0",
           "CV_FLOW_FUSED_RESNET": "0", "CV_FLOW_FUSE_TAIL_HEAD": "0", "CV_FLOW_STAGE_ABI": "0", "CV_STREAM_ENC_CACHE": "0",
           "CV_HIFT_STAGE_ABI": "0", "CV_HIFT_PRESPLIT": "0", "CV_OVERLAP_HIFT": "1", "CV_PREFILL_ON_FLOW": "0", "CV_LLM_RAMP": "4"}


def _estimator(cfg, dtype=torch.bfloat16):
    """A ConditionalDecoder with the shape of a loaded one (packed resnet weights of the three covered input widths), no device."""
    from cosyvoice_amd.flow import ConditionalDecoder
    est = ConditionalDecoder(cfg, dtype, torch.device("cpu"))
    est.blocks = [dict(res=dict(w1_p=None, wr=torch.empty(256, cin)), tb=[]) for cin in (320, 256, 512)]
    return est


def test_package_reads_no_environment_variable():
    """The one exception is build.py's HIPCC: the path of a build tool, not a run-time switch."""
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) > 10
    for f in files:
        src = open(f).read()
        if os.path.basename(f) == "build.py":
            src = "".join(l for l in src.splitlines(True) if not l.startswith("HIPCC = os.environ.get("))
        assert "os.environ" not in src and "getenv" not in src, f


def test_defaults_ignore_the_retired_variables(monkeypatch):
    from cosyvoice_amd.flow import CausalConditionalCFM
    from cosyvoice_amd.hift import HiFTGenerator
    from cosyvoice_amd.llm import Qwen2LM
    for name, value in RETIRED.items():
        monkeypatch.setenv(name, value)
    lm = Qwen2LM(LlmConfig.tiny())
    assert Qwen2LM.DOWN_KSPLIT == 4 and lm.DOWN_KSPLIT == 4
    assert lm.split_norm is True and lm.use_stage_abi is True and lm.split_qkv_norm is None
    assert [bool(lm._split_qkv(B)) for B in (1, 8, 9, 16, 32)] == [False, False, True, True, True]
    est = _estimator(FlowConfig.tiny())
    assert est.use_fused is True and est.use_fused_resnet is True and est.use_tail_head is True
    assert est.fused is True and est.fused_all is True and est.fuse_tail_head is True
    cfm = CausalConditionalCFM(est.cfg, est, torch.device("cpu"))
    assert cfm.use_stage_abi is True and cfm.stage_abi is True
    hift = HiFTGenerator(HiftConfig.tiny())
    assert hift.use_stage_abi is True and hift.use_presplit is True and hift.presplit is True


def test_every_option_is_in_its_graph_key():
    from cosyvoice_amd.flow import CausalConditionalCFM
    from cosyvoice_amd.llm import Qwen2LM
    lm = Qwen2LM(LlmConfig.tiny())
    base = lm._graph_key(4, True, False)
    assert base == lm._graph_key(4, True, False)
    for name, value in (("split_norm", False), ("use_stage_abi", False), ("split_qkv_norm", True)):
        lm2 = Qwen2LM(LlmConfig.tiny())
        setattr(lm2, name, value)
        assert lm2._graph_key(4, True, False) != base, name
    lm.split_qkv_norm = False   # the key holds the RESOLVED choice: forcing what the row count selects anyway is the same graph
    assert lm._graph_key(4, True, False) == base
    assert lm._graph_key(16, True, False) != Qwen2LM(LlmConfig.tiny())._graph_key(16, True, False)

    cfg = FlowConfig.tiny()
    x, mu, cond, spks = torch.zeros(2, 8, 80), torch.zeros(2, 8, 80), torch.zeros(2, 8, 80), torch.zeros(2, 80)
    key = lambda cfm: cfm._graph_key(x, mu, spks, cond, None, 4)
    base = key(CausalConditionalCFM(cfg, _estimator(cfg), torch.device("cpu")))
    assert base == key(CausalConditionalCFM(cfg, _estimator(cfg), torch.device("cpu")))
    for name in ("use_fused", "use_fused_resnet", "use_tail_head"):
        est = _estimator(cfg)
        setattr(est, name, False)
        assert key(CausalConditionalCFM(cfg, est, torch.device("cpu"))) != base, name
    cfm = CausalConditionalCFM(cfg, _estimator(cfg), torch.device("cpu"))
    cfm.use_stage_abi = False
    assert key(cfm) != base
    # the resnet switch alone, with the stage ABI already off: still another launch sequence, still another key
    cfm.estimator.use_fused_resnet = False
    off = key(cfm)
    cfm.estimator.use_fused_resnet = True
    assert key(cfm) != off
