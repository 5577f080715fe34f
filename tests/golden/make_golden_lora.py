#!/usr/bin/env python3
"""Mint tests/golden/llm_lora_tiny.npz by running the REFERENCE's own Qwen2LM (cosyvoice/llm/llm.py:743-874) wrapped by its own
loralib.replace_specific_layer_4lora (cosyvoice/loralib/utils.py:102-214) on the key-seeded weights of
cosyvoice_amd.weights.llm_state_dict + llm_lora_state_dict.

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_lora.py

The tiny reference LM is built and driven exactly as make_golden.golden_llm_loop does for llm_tiny_loop.npz: the reference's own
``inference`` loop, teacher-forced (make_golden._ref_lm_inference_capture).  That pins which tensors take part at inference
(llm.py:824-874): embed_tokens and speech_embedding are CALLED in the prefill assembly (adapted), llm_embedding.weight[...] and the
decode-step input speech_embedding.weight[top_ids] are raw ``.weight`` reads (base rows), lm_head is never called.

Three sets over the same inputs: adapter 0 (seed, lora_alpha 16), adapter 1 (seed + 1, lora_alpha 32) and the base model through
loralib.mark_only_infer_base_model.  Stored: the inputs, the prefill sequence lm_input and the 13 log-prob rows of each set; no weights
(they are regenerated from cosyvoice_amd.weights).

The script asserts the SEPARATION the adapters' gain is chosen for: the L-infinity distance between any two of the three log-prob sets
lies in [0.3, 3] — far above the 16-bit parity tolerances of the GPU tests, small enough that the adapted model is still the same
model."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

LORA_R = 16
SEED = 1986
ADAPTERS = ((SEED, 16), (SEED + 1, 32))      # (seed, lora_alpha) of adapter 0 and adapter 1
SEPARATION = (0.3, 3.0)


def build_wrapped(cfg, base_sd, lora_sd, alpha):
    from cosyvoice import loralib
    from cosyvoice.loralib.utils import replace_specific_layer_4lora
    lm = mg.build_ref_llm(cfg, base_sd)
    lm = replace_specific_layer_4lora(lm, {"lora_r": LORA_R, "lora_alpha": alpha})
    n_lora = sum(1 for k in lm.state_dict() if "lora_" in k)
    assert set(k for k in lm.state_dict() if "lora_" in k) == set(lora_sd), "llm_lora_state_dict does not name what loralib wraps"
    res = lm.load_state_dict({**base_sd, **lora_sd}, strict=False)   # the wrap re-initialised every base weight: load both
    assert not res.unexpected_keys, res.unexpected_keys
    assert all("rotary" in k or "inv_freq" in k for k in res.missing_keys), res.missing_keys
    return lm.eval(), n_lora


def main():
    mg.install_stubs()
    from cosyvoice.loralib.utils import mark_only_infer_base_model
    from cosyvoice_amd.config import LlmConfig
    from cosyvoice_amd.weights import llm_lora_state_dict, llm_state_dict
    cfg = LlmConfig.tiny()
    base_sd = llm_state_dict(cfg)
    g = torch.Generator().manual_seed(31)    # the inputs of llm_tiny_loop.npz
    text = torch.randint(0, cfg.vocab_size, (1, 6), generator=g, dtype=torch.int32)
    prompt_text = torch.randint(0, cfg.vocab_size, (1, 4), generator=g, dtype=torch.int32)
    prompt_speech = torch.randint(0, cfg.speech_token_size, (1, 9), generator=g, dtype=torch.int32)
    forced = torch.randint(0, cfg.speech_token_size, (12,), generator=g).tolist()
    out = {}
    for tag, (seed, alpha), base_only in (("a0", ADAPTERS[0], False), ("a1", ADAPTERS[1], False), ("base", ADAPTERS[0], True)):
        lm, n_lora = build_wrapped(cfg, base_sd, llm_lora_state_dict(cfg, r=LORA_R, seed=seed), alpha)
        if base_only:
            mark_only_infer_base_model(lm)
        lm_input, logps = mg._ref_lm_inference_capture(lm, text, prompt_text, prompt_speech, forced, cfg.speech_token_size)
        out[tag] = (lm_input[0], logps)
        print(tag, "lora tensors", n_lora, "logps", tuple(logps.shape))
    ref = np.load(os.path.join(HERE, "llm_tiny_loop.npz"))
    assert np.abs(out["base"][1].numpy() - ref["logps"]).max() < 1e-5, "infer_base_model does not reproduce llm_tiny_loop.npz"
    sep = {}
    for a, b in (("a0", "a1"), ("a0", "base"), ("a1", "base")):
        sep[a + "_" + b] = float((out[a][1] - out[b][1]).abs().max())
    print("separation", sep)
    assert all(SEPARATION[0] <= v <= SEPARATION[1] for v in sep.values()), sep
    mg.save("llm_lora_tiny", text=text, prompt_text=prompt_text, prompt_speech=prompt_speech, forced=np.array(forced),
            lora_r=np.array(LORA_R), seeds=np.array([a[0] for a in ADAPTERS]), alphas=np.array([a[1] for a in ADAPTERS]),
            separation=np.array([sep["a0_a1"], sep["a0_base"], sep["a1_base"]]),
            lm_input_a0=out["a0"][0], lm_input_a1=out["a1"][0], lm_input_base=out["base"][0],
            logps_a0=out["a0"][1], logps_a1=out["a1"][1], logps_base=out["base"][1])


if __name__ == "__main__":
    main()
