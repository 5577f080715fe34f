"""GPU: per-sequence LoRA adapters in Qwen2LM (cosyvoice_amd/lora.py, attach_lora / adapters=) against the golden minted from the
reference's own loralib-wrapped Qwen2LM.inference loop (tests/golden/make_golden_lora.py -> llm_lora_tiny.npz), and the batch
properties: mixed adapters per row, generation equal to each sequence alone, one captured graph for every assignment, and a base
path that attaching a bank does not touch."""
import os

import numpy as np
import pytest
import torch

from cosyvoice_amd.config import LlmConfig
from cosyvoice_amd.weights import llm_lora_state_dict, llm_state_dict

pytestmark = pytest.mark.gpu

TOL = {torch.float16: 2e-2, torch.bfloat16: 1.5e-1}      # the tiny-LM tolerances of test_llm_gpu.py::test_teacher_forced_logp_vs_golden
TAGS = {0: "a0", 1: "a1", -1: "base"}


def _golden(golden_dir):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "llm_lora_tiny.npz")).items()}


def _lm_with_bank(g, dt, max_batch=4, round_to=None):
    """Tiny LM + a 4-slot bank holding the golden's two adapters in slots 0 and 1."""
    from cosyvoice_amd.llm import Qwen2LM
    from cosyvoice_amd.lora import LoraBank
    cfg = LlmConfig.tiny()
    lm = Qwen2LM(cfg, dtype=dt, max_batch=max_batch, ctx_max=256, max_out=256).load_state_dict(llm_state_dict(cfg, round_to=round_to))
    bank = LoraBank(lm, max_adapters=4, r=int(g["lora_r"]))
    for i in range(2):
        slot = bank.add(f"voice{i}", llm_lora_state_dict(cfg, r=int(g["lora_r"]), seed=int(g["seeds"][i])), alpha=float(g["alphas"][i]))
        assert slot == i
    lm.attach_lora(bank)
    return lm, bank, cfg


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_lora_teacher_forced_logp_vs_reference_golden(golden_dir, dt):
    g = _golden(golden_dir)
    lm, bank, cfg = _lm_with_bank(g, dt)
    sep = {(0, 1): float(g["separation"][0]), (0, -1): float(g["separation"][1]), (1, -1): float(g["separation"][2])}
    assert TOL[dt] < 0.25 * min(sep.values())      # a result within TOL of its own golden is farther than 3 TOL from the other two
    forced = g["forced"].tolist()
    for use_graph in (False, True):
        lm.use_graph = use_graph
        for k in (0, 1, -1):
            lp = lm.forced_logits(g["text"], g["prompt_text"], g["prompt_speech"], forced, adapters=[k]).cpu()
            err = (lp - g["logps_" + TAGS[k]]).abs().max().item()
            print(f"lora logp[{dt}, graph={use_graph}, adapter {k}] Linf {err:.3e}")
            assert err < TOL[dt]
            for other in (0, 1):
                if other != k and k >= 0:
                    far = (lp - g["logps_" + TAGS[other]]).abs().max().item()
                    assert far > 0.5 * sep[(min(k, other), max(k, other))], (k, other, far)
    by_name = lm.forced_logits(g["text"], g["prompt_text"], g["prompt_speech"], forced, adapters=["voice1"]).cpu()
    assert torch.equal(by_name, lm.forced_logits(g["text"], g["prompt_text"], g["prompt_speech"], forced, adapters=[1]).cpu())


def test_lora_mixed_batch_rows_use_their_own_adapter(golden_dir):
    g = _golden(golden_dir)
    dt = torch.float16
    lm, bank, cfg = _lm_with_bank(g, dt)
    forced = g["forced"].tolist()
    assign = [0, 1, -1, 0]
    lp = lm.forced_logits(g["text"], g["prompt_text"], g["prompt_speech"], forced, rows=4, adapters=assign).cpu()     # (13, 4, V)
    assert torch.equal(lp[:, 0], lp[:, 3])
    for row, k in enumerate(assign):
        err = (lp[:, row] - g["logps_" + TAGS[k]]).abs().max().item()
        print(f"mixed batch row {row} adapter {k}: Linf {err:.3e}")
        assert err < TOL[dt]
    # an adapter whose B is all zero (a checkpoint that skipped every module) computes the base model
    assert bank.add("zero", {}) == 2
    z = lm.forced_logits(g["text"], g["prompt_text"], g["prompt_speech"], forced, rows=2, adapters=["zero", -1]).cpu()
    assert bool((z[:, 0] == z[:, 1]).all())
    # a removed adapter frees its slot and leaves the base model behind
    bank.remove("voice1")
    gone = lm.forced_logits(g["text"], g["prompt_text"], g["prompt_speech"], forced, rows=2, adapters=[1, -1]).cpu()
    assert bool((gone[:, 0] == gone[:, 1]).all())
    with pytest.raises(KeyError):
        lm.forced_logits(g["text"], g["prompt_text"], g["prompt_speech"], forced, adapters=["voice1"])


def _ragged_inputs(cfg):
    """The four ragged shapes and the uniforms of test_llm_gpu.py::test_ragged_batch_equals_single_sequences."""
    g = torch.Generator().manual_seed(21)
    shapes = [(5, 3, 7), (2, 0, 0), (9, 4, 12), (1, 1, 3)]
    texts = [torch.randint(0, cfg.vocab_size, (1, a), generator=g, dtype=torch.int32) for a, _, _ in shapes]
    ptexts = [torch.randint(0, cfg.vocab_size, (1, b), generator=g, dtype=torch.int32) for _, b, _ in shapes]
    pspeech = [torch.randint(0, cfg.speech_token_size, (1, c), generator=g, dtype=torch.int32) for _, _, c in shapes]
    uni = torch.zeros(16, 101, 2)
    uni[:, :, 0] = torch.rand(16, 101, generator=g) * 0.6
    uni[:, :, 1] = torch.rand(16, 101, generator=g)
    return texts, ptexts, pspeech, uni


def test_lora_generation_batch_equals_each_sequence_alone(golden_dir):
    g = _golden(golden_dir)
    lm, bank, cfg = _lm_with_bank(g, torch.bfloat16, round_to=torch.bfloat16)
    texts, ptexts, pspeech, uni = _ragged_inputs(cfg)
    assign = [0, -1, 1, 0]
    got = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=assign)
    n_graphs = len(lm._graphs)
    assert n_graphs >= 1
    for b in range(4):
        u1 = uni.clone()
        u1[0] = uni[b]
        alone = lm.generate_batch([texts[b]], [ptexts[b]], [pspeech[b]], uniforms=u1, adapters=[assign[b]])[0]
        assert alone == got[b], (b, alone[:8], got[b][:8])
    base = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni)
    # adapters change tokens.  (The -1 row computes the base model through the LoRA step's un-fused composition, which rounds differently
    # from the base step: its tokens agree with ``base`` only up to 16-bit near-ties, which the golden test bounds instead.)
    assert base[0] != got[0] or base[2] != got[2]
    # one captured graph serves every assignment: another assignment of the same batch shape adds no entry
    n_graphs = len(lm._graphs)
    other = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=[1, 0, -1, "voice1"])
    assert len(lm._graphs) == n_graphs
    assert other != got
    again = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=assign)
    assert again == got and len(lm._graphs) == n_graphs
    lm.use_graph = False
    eager = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=assign)
    assert eager == got


def test_lora_attach_leaves_the_base_path_untouched(golden_dir):
    from cosyvoice_amd.llm import Qwen2LM
    from cosyvoice_amd.lora import LoraBank
    g = _golden(golden_dir)
    cfg = LlmConfig.tiny()
    lm = Qwen2LM(cfg, dtype=torch.bfloat16, max_batch=4, ctx_max=256, max_out=256).load_state_dict(llm_state_dict(cfg, round_to=torch.bfloat16))
    texts, ptexts, pspeech, uni = _ragged_inputs(cfg)
    before = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni)
    keys_before = set(lm._graphs)
    with pytest.raises(RuntimeError):
        lm.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=[0, 0, 0, 0])      # no bank attached
    bank = LoraBank(lm, max_adapters=2, r=16)
    bank.add("voice0", llm_lora_state_dict(cfg, seed=int(g["seeds"][0])))
    lm.attach_lora(bank)
    attached = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni)
    assert attached == before and set(lm._graphs) == keys_before
    with_lora = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=["voice0"] * 4)
    assert with_lora != before and len(lm._graphs) == len(keys_before) + 1
    ctx = lm.new_context()                      # shares the bank, owns its step buffers
    assert ctx._lora["bank"] is bank and ctx._lora["u"].data_ptr() != lm._lora["u"].data_ptr()
    assert ctx.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=["voice0"] * 4) == with_lora
    lm.detach_lora()
    after = lm.generate_batch(texts, ptexts, pspeech, uniforms=uni)
    assert after == before and set(lm._graphs) == keys_before
    assert all(len(k) == len(lm._graph_key(4, False, True)) for k in lm._graphs)       # only keys of the base shape


def test_lora_two_row_groups_equal_one(golden_dir):
    """20 rows with mixed adapters on a max_batch = 32 object (two 16-row groups per step) emit the tokens the same rows emit on a
    max_batch = 16 object."""
    g = _golden(golden_dir)
    lm32, _, cfg = _lm_with_bank(g, torch.bfloat16, max_batch=32, round_to=torch.bfloat16)
    lm16, _, _ = _lm_with_bank(g, torch.bfloat16, max_batch=16, round_to=torch.bfloat16)
    gen = torch.Generator().manual_seed(77)
    n = 20
    texts = [torch.randint(0, cfg.vocab_size, (1, 2 + b % 3), generator=gen, dtype=torch.int32) for b in range(n)]
    ptexts = [torch.randint(0, cfg.vocab_size, (1, b % 2), generator=gen, dtype=torch.int32) for b in range(n)]
    pspeech = [torch.randint(0, cfg.speech_token_size, (1, 3 + b % 4), generator=gen, dtype=torch.int32) for b in range(n)]
    uni = torch.zeros(32, 101, 2)
    uni[:, :, 0] = torch.rand(32, 101, generator=gen) * 0.6
    uni[:, :, 1] = torch.rand(32, 101, generator=gen)
    assign = [(0, 1, -1, 1, 0)[b % 5] for b in range(n)]
    got = lm32.generate_batch(texts, ptexts, pspeech, uniforms=uni, adapters=assign)
    for lo, hi in ((0, 16), (16, 20)):
        u16 = torch.zeros(16, 101, 2)
        u16[:hi - lo] = uni[lo:hi]
        part = lm16.generate_batch(texts[lo:hi], ptexts[lo:hi], pspeech[lo:hi], uniforms=u16, adapters=assign[lo:hi])
        assert part == got[lo:hi], (lo, hi)


# ----------------------------------------------------------------------------- orchestrators
def _tiny_stack(g, max_batch=4):
    """The tiny LLM -> flow -> HiFT stack of test_model_gpu.py with the golden's two adapters attached to its LLM."""
    from cosyvoice_amd.config import FlowConfig, HiftConfig
    from cosyvoice_amd.flow import CausalMaskedDiffWithXvec
    from cosyvoice_amd.hift import HiFTGenerator
    from cosyvoice_amd.llm import Qwen2LM
    from cosyvoice_amd.lora import LoraBank
    from cosyvoice_amd.model import CosyVoice2Model
    from cosyvoice_amd.weights import flow_state_dict, hift_state_dict
    lc, fc, hc = LlmConfig.tiny(), FlowConfig.tiny(), HiftConfig.tiny()
    llm = Qwen2LM(lc, dtype=torch.bfloat16, max_batch=max_batch, ctx_max=256, max_out=256)
    m = CosyVoice2Model(llm, CausalMaskedDiffWithXvec(fc, dtype=torch.float16), HiFTGenerator(hc, dtype=torch.float32), fp16=False)
    m.load_state_dicts(llm_state_dict(lc), flow_state_dict(fc), hift_state_dict(hc))
    bank = LoraBank(llm, max_adapters=4, r=int(g["lora_r"]))
    for i in range(2):
        bank.add(f"voice{i}", llm_lora_state_dict(lc, r=int(g["lora_r"]), seed=int(g["seeds"][i])), alpha=float(g["alphas"][i]))
    llm.attach_lora(bank)
    return m, lc, fc, hc


def _stack_inputs(lc, fc, seed=0, n_text=6, n_p=10):
    g = torch.Generator().manual_seed(seed)
    return dict(text=torch.randint(0, lc.vocab_size, (1, n_text), generator=g, dtype=torch.int32),
                prompt_text=torch.randint(0, lc.vocab_size, (1, 4), generator=g, dtype=torch.int32),
                llm_prompt_speech_token=torch.randint(0, lc.speech_token_size, (1, n_p), generator=g, dtype=torch.int32),
                flow_prompt_speech_token=torch.randint(0, lc.speech_token_size, (1, n_p), generator=g, dtype=torch.int32),
                prompt_speech_feat=torch.clamp(torch.randn(1, 2 * n_p, 80, generator=g) * 2 - 6, -11.5, 2.0),
                flow_embedding=torch.randn(1, fc.spk_embed_dim, generator=g))


def test_lora_tts_batch_and_tts_pass_adapters_to_the_llm(golden_dir):
    """tts_batch(adapters=[0, 1]) with forced tokens: the waveforms of the two single-adapter runs (forced tokens fix the audio), and row b
    of the LLM's last logits is the row the run with adapter b alone in every row leaves — the adapters reached the decode loop."""
    g = _golden(golden_dir)
    m, lc, fc, hc = _tiny_stack(g)
    B = 2
    ins = [_stack_inputs(lc, fc, seed=s) for s in range(B)]
    sh = ins[0]
    forced = [torch.randint(0, lc.speech_token_size, (14,), generator=torch.Generator().manual_seed(9 + b)).tolist() for b in range(B)]
    out = {}
    for name, ad in (("mixed", [0, 1]), ("a0", [0, 0]), ("a1", ["voice1", "voice1"]), ("base", None)):
        torch.manual_seed(0)
        wav = m.tts_batch([i["text"] for i in ins], [sh["prompt_text"]] * B, [sh["llm_prompt_speech_token"]] * B,
                          sh["flow_prompt_speech_token"].expand(B, -1), sh["prompt_speech_feat"].expand(B, -1, -1),
                          sh["flow_embedding"].expand(B, -1), forced=forced, adapters=ad)
        out[name] = (wav.clone(), m.llm.st["logits"][:B, :lc.out_vocab].cpu().clone())
    assert out["mixed"][0].shape == (B, 14 * 2 * hc.total_upsample) and torch.isfinite(out["mixed"][0]).all()
    assert torch.equal(out["mixed"][0], out["a0"][0]) and torch.equal(out["mixed"][0], out["a1"][0])
    assert torch.equal(out["mixed"][1][0], out["a0"][1][0]) and torch.equal(out["mixed"][1][1], out["a1"][1][1])
    assert not torch.equal(out["a0"][1], out["a1"][1]) and not torch.equal(out["mixed"][1], out["base"][1])
    # tts(): the request's adapter goes through llm_job to the decode context (made before or after attach_lora)
    toks = {}
    for lora in ("voice0", 1, -1, None):
        wavs = [o["tts_speech"] for o in m.tts(**ins[1], stream=False, seed=5, lora=lora)]
        assert len(wavs) == 1 and torch.isfinite(wavs[0]).all()
        toks[lora] = wavs[0].shape[1] // (2 * hc.total_upsample)
        assert 2 * 6 <= toks[lora] <= 20 * 6
    with pytest.raises(KeyError):
        list(m.tts(**ins[1], stream=False, lora="nobody"))


def test_lora_tts_batches_merges_adapters_in_row_order(golden_dir, monkeypatch):
    """tts_batches with ``llm_adapters`` in every batch dict: the CU-partitioned pipeline (two decode contexts made on demand, two batches
    per token loop) hands generate_batch the concatenated adapters and returns the waveforms of the plain two-stream pipeline."""
    from cosyvoice_amd.llm import Qwen2LM
    g = _golden(golden_dir)
    m, lc, fc, hc = _tiny_stack(g)
    B, nb = 2, 4
    sh = _stack_inputs(lc, fc, seed=0)
    per_batch = [[0, 1], [-1, "voice0"], [1, 1], ["voice1", -1]]

    def batches():
        out = []
        for i in range(nb):
            ins = [_stack_inputs(lc, fc, seed=10 * i + s) for s in range(B)]
            forced = [torch.randint(0, lc.speech_token_size, (14,), generator=torch.Generator().manual_seed(100 + i)).tolist()] * B
            out.append(dict(texts=[x["text"].cuda() for x in ins], prompt_texts=[sh["prompt_text"].cuda()] * B,
                            llm_prompt_speech_tokens=[sh["llm_prompt_speech_token"].cuda()] * B,
                            flow_prompt_speech_tokens=sh["flow_prompt_speech_token"].cuda().expand(B, -1),
                            prompt_speech_feats=sh["prompt_speech_feat"].cuda().expand(B, -1, -1),
                            flow_embeddings=sh["flow_embedding"].cuda().expand(B, -1), forced=forced, llm_adapters=per_batch[i]))
        return out

    seen = []
    real = Qwen2LM.generate_batch

    def spy(self, *a, **k):
        seen.append(k.get("adapters"))
        return real(self, *a, **k)
    monkeypatch.setattr(Qwen2LM, "generate_batch", spy)
    torch.manual_seed(0)
    ref = [w.clone() for w in m.tts_batches(batches(), llm_cu_slots=0)]
    assert seen == per_batch
    del seen[:]
    torch.manual_seed(0)
    m.llm_merge = 2
    got = [w.cpu().clone() for w in m.tts_batches(batches(), llm_cu_slots=8, llm_loops=2)]
    m.llm_merge = 1
    # the decode jobs run on two threads, in any order: each call carries the adapters of CONSECUTIVE batches, concatenated in row order,
    # and the calls cover every batch once
    spans = {tuple(map(str, sum(per_batch[i:j], []))): (i, j) for i in range(nb) for j in range(i + 1, nb + 1)}
    covered = sorted(spans[tuple(map(str, ads))] for ads in seen)
    assert [i for i, _ in covered] == [0] + [j for _, j in covered[:-1]] and covered[-1][1] == nb
    assert any(j - i == 2 for i, j in covered)
    assert len(got) == nb and all(torch.equal(a, b) for a, b in zip(ref, got))
    mixed = batches()
    del mixed[1]["llm_adapters"]
    m.llm_merge = 2                             # jobs of 1, 2, ... batches: the second job merges a batch without the key and one with it
    with pytest.raises(ValueError, match="llm_adapters"):
        list(m.tts_batches(mixed, llm_cu_slots=8, llm_loops=1))
    m.llm_merge = 1
    m.close()
