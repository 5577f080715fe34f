"""CPU: the LoRA entry points (include/cosyvoice_amd_lora.h, cosyvoice_amd._lib.LORA_EXPORTS) — declarations, exports and the Python list
agree and arguments are validated before anything is launched; LoraBank's checkpoint parsing; the plain-torch restatement
(tests/lora_ref.py) against the golden minted from the reference's own loralib-wrapped inference loop; and the way the batch pipeline
carries per-utterance adapters through a merged decode job."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lora_ref  # noqa: E402

from cosyvoice_amd.config import LlmConfig  # noqa: E402
from cosyvoice_amd.weights import llm_lora_modules, llm_lora_state_dict, llm_state_dict  # noqa: E402

HEADER = os.path.join(HERE, "..", "include", "cosyvoice_amd_lora.h")


# ----------------------------------------------------------------------------- ABI
def test_lora_exports_match_header_and_library():
    from cosyvoice_amd import build, _lib
    lib = ctypes.CDLL(build.build(verbose=False))
    declared = set(re.findall(r"\b(cv_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    assert declared == set(_lib.LORA_EXPORTS), (sorted(declared - set(_lib.LORA_EXPORTS)), sorted(set(_lib.LORA_EXPORTS) - declared))
    assert len(set(_lib.LORA_EXPORTS)) == len(_lib.LORA_EXPORTS)
    assert not set(_lib.LORA_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.STYLE_EXPORTS))
    for name in _lib.LORA_EXPORTS:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    _lib.lora_lib()   # the size handshake of the two parameter blocks


def test_main_header_does_not_declare_lora_entry_points():
    from cosyvoice_amd import _lib
    main = open(os.path.join(HERE, "..", "include", "cosyvoice_amd.h")).read()
    for name in _lib.LORA_EXPORTS:
        assert name not in main
    assert "lora" not in main.lower()


def _shrink_block(L):
    p = L.LoraShrinkParams()
    p.dtype, p.rows, p.rows_per_seq, p.K, p.R_tot, p.n_slots = L.CV_F16, 4, 1, 64, 16, 2
    p.x = p.A = p.row_adapter = p.u = 64
    p.ldx, p.ldu = 64, 16
    return p


def _expand_block(L):
    p = L.LoraExpandParams()
    p.dtype, p.rows, p.rows_per_seq, p.N, p.r, p.n_slots, p.mode, p.n_seg = L.CV_F16, 4, 1, 96, 16, 2, L.LORA_ADD, 3
    for i in range(3):
        p.seg[i].n_begin, p.seg[i].n_end, p.seg[i].u_off = 32 * i, 32 * (i + 1), 16 * i
    p.u = p.B = p.s = p.row_adapter = p.y = p.h = 64
    p.ldu, p.ldy, p.ldh = 48, 96, 48
    return p


def test_lora_argument_validation_without_a_gpu():
    """Bad arguments come back as a negative cv_status before anything is launched: dummy pointers are never dereferenced.  Each block
    passes every check until one field is broken."""
    from cosyvoice_amd import _lib as L
    lib = L.lora_lib()
    null = ctypes.c_void_p(None)
    ARG, UNSUPPORTED = -1, -3
    assert lib.cv_lora_shrink(None, null) == ARG and lib.cv_lora_expand(None, null) == ARG
    for field, bad, want in (("K", 48, UNSUPPORTED), ("K", 0, ARG), ("rows", 0, ARG), ("rows_per_seq", 0, ARG), ("R_tot", 12, UNSUPPORTED),
                             ("R_tot", 104, UNSUPPORTED), ("A", None, ARG), ("x", None, ARG), ("u", None, ARG), ("row_adapter", None, ARG),
                             ("x", 72, ARG), ("A", 8, ARG), ("u", 66, ARG), ("ldx", 60, ARG), ("ldx", 68, ARG), ("ldu", 8, ARG),
                             ("n_slots", 0, ARG), ("dtype", L.CV_F32, UNSUPPORTED)):
        p = _shrink_block(L)
        setattr(p, field, bad)
        assert lib.cv_lora_shrink(ctypes.byref(p), null) == want, (field, bad)
    for field, bad, want in (("r", 12, UNSUPPORTED), ("r", 64, UNSUPPORTED), ("rows", 0, ARG), ("N", 0, ARG), ("B", None, ARG), ("s", None, ARG),
                             ("u", None, ARG), ("y", None, ARG), ("row_adapter", None, ARG), ("n_seg", 4, ARG), ("n_seg", 0, ARG),
                             ("n_seg", 2, ARG),            # two segments no longer cover [0, N)
                             ("B", 72, ARG), ("y", 66, ARG), ("ldy", 64, ARG), ("ldu", 40, ARG), ("mode", 3, ARG), ("n_slots", 0, ARG),
                             ("dtype", L.CV_F32, UNSUPPORTED)):
        p = _expand_block(L)
        setattr(p, field, bad)
        assert lib.cv_lora_expand(ctypes.byref(p), null) == want, (field, bad)
    p = _expand_block(L)
    p.seg[1].n_begin = 40                                   # a gap between two segments
    assert lib.cv_lora_expand(ctypes.byref(p), null) == ARG
    p = _expand_block(L)
    p.mode = L.LORA_SWIGLU                                  # SWIGLU takes exactly the gate and the up segment
    assert lib.cv_lora_expand(ctypes.byref(p), null) == UNSUPPORTED
    p.n_seg, p.N = 2, 64
    p.h = None
    assert lib.cv_lora_expand(ctypes.byref(p), null) == ARG


def test_lora_source_has_no_environment_switch_or_inline_assembly():
    src = open(os.path.join(HERE, "..", "cosyvoice_amd", "csrc", "lora.hip")).read()
    assert "getenv" not in src and "asm" not in src and "atomic" not in src.replace("<atomic>", "")


# ----------------------------------------------------------------------------- LoraBank
class _CpuLM:
    """What LoraBank reads of a Qwen2LM."""
    def __init__(self, dtype=torch.float16):
        self.cfg, self.dtype, self.device = LlmConfig.tiny(), dtype, torch.device("cpu")


def test_lora_state_dict_names_what_the_bank_parses():
    from cosyvoice_amd.lora import LoraBank
    cfg = LlmConfig.tiny()
    sd = llm_lora_state_dict(cfg, r=16)
    assert len(sd) == 2 * len(llm_lora_modules(cfg)) == 2 * (7 * cfg.num_layers + 5)
    assert all(bool(v.abs().max() > 0) for v in sd.values())            # non-zero B: a trained adapter
    bank = LoraBank(_CpuLM(), max_adapters=3, r=16)
    assert bank.add("a", sd) == 0 and bank.add("b", sd, alpha=32) == 1 and bank.add("c", sd, alpha=32, noscale=True) == 2
    assert bank.slot("b") == 1 and bank.s.tolist() == [1.0, 2.0, 1.0]      # s = alpha / r, or 1 with noscale
    with pytest.raises(RuntimeError):
        bank.add("d", sd)                                                   # the bank is full
    assert bank.add("a", sd, alpha=8) == 0 and bank.s[0].item() == 0.5      # the same name re-loads its own slot
    r, q, kv, I = 16, cfg.q_dim, cfg.kv_dim, cfg.intermediate_size
    h16 = lambda t: t.to(torch.float16)
    for i, lay in enumerate(bank.layers):
        p = f"llm.model.model.layers.{i}."
        A_qkv = torch.cat([sd[p + f"self_attn.{n}_proj.lora_A"] for n in "qkv"], 0)
        B_qkv = torch.cat([sd[p + f"self_attn.{n}_proj.lora_B"] for n in "qkv"], 0)
        assert torch.equal(lay["A_qkv"][1], h16(A_qkv)) and torch.equal(lay["B_qkv"][1], h16(B_qkv))
        assert torch.equal(lay["A_o"][1], h16(sd[p + "self_attn.o_proj.lora_A"])) and torch.equal(lay["B_o"][1], h16(sd[p + "self_attn.o_proj.lora_B"]))
        assert torch.equal(lay["A_gu"][1], h16(torch.cat([sd[p + "mlp.gate_proj.lora_A"], sd[p + "mlp.up_proj.lora_A"]], 0)))
        assert torch.equal(lay["B_gate"][1], h16(sd[p + "mlp.gate_proj.lora_B"])) and torch.equal(lay["B_up"][1], h16(sd[p + "mlp.up_proj.lora_B"]))
        assert lay["B_gu"].shape == (3, 2 * I, r) and torch.equal(lay["B_gu"][1, I:], lay["B_up"][1])
        assert torch.equal(lay["A_down"][1], h16(sd[p + "mlp.down_proj.lora_A"])) and torch.equal(lay["B_down"][1], h16(sd[p + "mlp.down_proj.lora_B"]))
    assert torch.equal(bank.A_dec[1], h16(sd["llm_decoder.lora_A"])) and torch.equal(bank.B_dec[1], h16(sd["llm_decoder.lora_B"]))
    assert torch.equal(bank.AT_embed[1], h16(sd["llm.model.model.embed_tokens.lora_A"].t()))       # A^T (vocab, r) for the gather
    assert torch.equal(bank.AT_speech[1], h16(sd["speech_embedding.lora_A"].t())) and torch.equal(bank.B_speech[1], h16(sd["speech_embedding.lora_B"]))
    assert bank.qkv_segments == [(0, q, 0), (q, q + kv, r), (q + kv, q + 2 * kv, 2 * r)] and bank.gu_segments == [(0, I, 0), (I, 2 * I, r)]
    ptrs = [bank.A_dec.data_ptr(), bank.layers[0]["B_gu"].data_ptr(), bank.s.data_ptr()]
    bank.remove("b")
    with pytest.raises(KeyError):
        bank.slot("b")
    assert bank.s[1].item() == 0.0 and not bool(bank.B_dec[1].any()) and not bool(bank.layers[0]["B_qkv"][1].any())
    assert bank.add("e", sd) == 1                                           # the freed slot is reused; no buffer moved
    assert ptrs == [bank.A_dec.data_ptr(), bank.layers[0]["B_gu"].data_ptr(), bank.s.data_ptr()]
    assert bank.resolve("e") == 1 and bank.resolve(-1) == -1 and bank.resolve(2) == 2
    with pytest.raises(ValueError):
        bank.resolve(3)


def test_lora_bank_skipped_modules_ignored_modules_and_refusals():
    from cosyvoice_amd.lora import LoraBank
    cfg = LlmConfig.tiny()
    sd = llm_lora_state_dict(cfg, r=16)
    bank = LoraBank(_CpuLM(torch.bfloat16), max_adapters=2, r=16)
    # lora_skip_modules = ["llm_decoder", "llm.model.model.layers.1.mlp"]: the checkpoint has no keys of them -> zero B
    skipped = {k: v for k, v in sd.items() if not (k.startswith("llm_decoder.") or k.startswith("llm.model.model.layers.1.mlp."))}
    bank.add("skip", skipped)
    assert not bool(bank.B_dec[0].any()) and not bool(bank.layers[1]["B_gu"][0].any()) and not bool(bank.layers[1]["B_down"][0].any())
    assert bool(bank.layers[0]["B_gu"][0].any()) and bool(bank.layers[1]["B_qkv"][0].any())
    # llm_embedding and lm_head are wrapped by loralib but never called as modules by Qwen2LM.inference (llm.py:846-847): accepted, ignored;
    # speech_embedding is kept for the prompt rows only (the decode-step input is the raw .weight row, llm.py:874)
    for k in ("llm_embedding.lora_A", "llm_embedding.lora_B", "llm.model.lm_head.lora_A", "llm.model.lm_head.lora_B", "speech_embedding.lora_A"):
        assert k in sd
    only_ignored = {k: v for k, v in sd.items() if k.startswith("llm_embedding.") or k.startswith("llm.model.lm_head.")}
    bank.add("ignored", only_ignored)
    assert not bool(bank.B_dec[1].any()) and not bool(bank.B_embed[1].any()) and not bool(bank.AT_speech[1].any())
    bank.remove("ignored")
    # keys without lora_ (a `bias = all` save) are not read
    bank.add("with_bias", {**sd, "llm_decoder.bias": torch.zeros(cfg.out_vocab)})
    bank.remove("with_bias")
    with pytest.raises(ValueError, match="text_encoder"):                   # a module of the phoneme front end
        bank.add("foreign", {**sd, "text_encoder.encoders.0.feed_forward.w_1.lora_A": torch.zeros(16, 8)})
    with pytest.raises(ValueError, match="rank"):
        bank.add("rank8", llm_lora_state_dict(cfg, r=8))
    with pytest.raises(ValueError, match="weight_cache"):
        bank.add("cachewnorm", {**sd, "llm_decoder.weight_cache": torch.zeros(cfg.out_vocab, cfg.hidden_size)})
    assert bank.names() == {"skip": 0}                                      # a refused checkpoint takes no slot
    with pytest.raises(ValueError):
        LoraBank(_CpuLM(), max_adapters=1, r=12)


# ----------------------------------------------------------------------------- restatement vs the reference golden
def test_lora_ref_vs_reference_golden(golden_dir):
    """tests/lora_ref.py against the reference's own loralib-wrapped Qwen2LM.inference loop: lm_input bit-equal, log-probs within the 1e-4
    test_oracle_golden.py uses for the tiny LM.  Adapting the decode-step embedding (llm.py:874 reads the base .weight row) fails this."""
    cfg = LlmConfig.tiny()
    sd = llm_state_dict(cfg)
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "llm_lora_tiny.npz")).items()}
    r = int(g["lora_r"])
    sets = [("a0", llm_lora_state_dict(cfg, r=r, seed=int(g["seeds"][0])), float(g["alphas"][0]) / r),
            ("a1", llm_lora_state_dict(cfg, r=r, seed=int(g["seeds"][1])), float(g["alphas"][1]) / r), ("base", None, 0.0)]
    out = {}
    for tag, lsd, s in sets:
        lm_in, lp = lora_ref.forced_logps(sd, lsd, s, cfg, g["text"], g["prompt_text"], g["prompt_speech"], g["forced"].tolist())
        assert torch.equal(lm_in[0], g["lm_input_" + tag]), tag
        err = (lp - g["logps_" + tag]).abs().max().item()
        print(f"lora_ref {tag}: Linf {err:.3e}")
        assert err < 1e-4
        out[tag] = lp
    # the sos / task rows are base rows in every set; the text and prompt-speech rows differ
    L = g["lm_input_base"].shape[0]
    n_text = g["text"].shape[1] + g["prompt_text"].shape[1]
    for tag in ("a0", "a1"):
        d = (g["lm_input_" + tag] - g["lm_input_base"]).abs().amax(-1)
        assert d[0] == 0 and d[1 + n_text] == 0 and bool((d[1:1 + n_text] > 0).all()) and bool((d[2 + n_text:L] > 0).all())
    sep = [float((out[a] - out[b]).abs().max()) for a, b in (("a0", "a1"), ("a0", "base"), ("a1", "base"))]
    assert np.allclose(sep, g["separation"].numpy(), atol=1e-3) and all(0.3 <= v <= 3.0 for v in sep)


# ----------------------------------------------------------------------------- pipeline
class _FakeLLM:
    def __init__(self):
        self.calls = []

    def generate_batch(self, texts, prompt_texts, prompt_speech, forced=None, **kw):
        self.calls.append(dict(texts=list(texts), forced=forced, **kw))
        return [[int(t)] for t in texts]


def _batch(ids, adapters=None):
    b = dict(texts=list(ids), prompt_texts=[None] * len(ids), llm_prompt_speech_tokens=[None] * len(ids))
    if adapters is not None:
        b["llm_adapters"] = list(adapters)
    return b


def test_pipeline_carries_adapters_through_a_merged_decode_job():
    from cosyvoice_amd.pipeline import decode_job, merged_adapters
    llm = _FakeLLM()
    bs = [_batch([0, 1], ["alice", -1]), _batch([2], [1]), _batch([3, 4, 5], [0, "bob", -1])]
    out = decode_job(llm, bs, steps_per_poll=64)
    assert out == [[[0], [1]], [[2]], [[3], [4], [5]]]
    assert llm.calls[0]["texts"] == [0, 1, 2, 3, 4, 5] and llm.calls[0]["adapters"] == ["alice", -1, 1, 0, "bob", -1]
    assert llm.calls[0]["steps_per_poll"] == 64
    decode_job(llm, [_batch([0, 1]), _batch([2])])
    assert "adapters" not in llm.calls[1]                       # no batch carries the key: the call is today's call
    assert merged_adapters([_batch([0])]) is None
    with pytest.raises(ValueError, match="1 of the 3 batches"):
        decode_job(llm, [_batch([0, 1]), _batch([2], [0]), _batch([3])])
    with pytest.raises(ValueError, match="2 entries"):
        decode_job(llm, [_batch([0], [0, 1])])
    assert len(llm.calls) == 2
