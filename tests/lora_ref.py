"""Plain-torch restatement of the reference's LoRA inference semantics for the speech LM, built on oracle.llm (tests only).

loralib/layers.py:222-235 (Linear, unmerged) and :115-123 (Embedding), as Qwen2LM.inference (llm/llm.py:824-874) uses them:
  * the 7 Linears of every decoder layer and llm_decoder: y = x W^T + b + s (x A^T) B^T — restated with MERGED weights W + s B A;
  * embed_tokens(text) and speech_embedding(prompt_speech_token) in the prefill assembly: e = W[idx] + s (A^T[idx]) B^T, evaluated in
    exactly that form so that lm_input is bit-equal to the reference's;
  * llm_embedding.weight[...] (:846-847) and the decode-step input speech_embedding.weight[top_ids] (:874): raw base rows.
"""
import torch
import torch.nn.functional as F

from oracle import llm as ol

P = "llm.model.model."
LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def merged_state_dict(sd, lora_sd, s):
    """Base state dict with s B A added to the weights of the decoder layers' Linears and of llm_decoder (None: the base model)."""
    if lora_sd is None:
        return sd
    out = dict(sd)
    mods = [k[:-len(".lora_A")] for k in lora_sd if k.endswith(".lora_A")]
    for m in mods:
        if m == "llm_decoder" or (m.startswith(P + "layers.") and m.split(".", 5)[-1] in LINEARS):
            out[m + ".weight"] = sd[m + ".weight"] + s * (lora_sd[m + ".lora_B"] @ lora_sd[m + ".lora_A"])
    return out


def lora_embedding(idx, W, A, B, s):
    """loralib Embedding.forward (layers.py:115-123)."""
    e = F.embedding(idx, W)
    e += (F.embedding(idx, A.transpose(0, 1)) @ B.transpose(0, 1)) * s
    return e


def build_lm_input(sd, lora_sd, s, cfg, text, prompt_text, prompt_speech_token):
    """llm.py:837-852 with the two module calls adapted and the two llm_embedding rows read raw."""
    if lora_sd is None:
        return ol.build_lm_input(sd, cfg, text, prompt_text, prompt_speech_token)
    t = torch.cat([prompt_text, text], dim=1).long()
    te = lora_embedding(t, sd[f"{P}embed_tokens.weight"], lora_sd[f"{P}embed_tokens.lora_A"], lora_sd[f"{P}embed_tokens.lora_B"], s)
    sos = sd["llm_embedding.weight"][0].reshape(1, 1, -1)
    task = sd["llm_embedding.weight"][1].reshape(1, 1, -1)
    if prompt_speech_token.shape[1] != 0:
        pe = lora_embedding(prompt_speech_token.long(), sd["speech_embedding.weight"], lora_sd["speech_embedding.lora_A"],
                            lora_sd["speech_embedding.lora_B"], s)
    else:
        pe = torch.zeros(1, 0, cfg.hidden_size)
    return torch.cat([sos, te, task, pe], dim=1)


def forced_logps(sd, lora_sd, s, cfg, text, prompt_text, prompt_speech_token, forced):
    """Teacher-forced log-probs of Qwen2LM.inference: returns lm_input (1, L, H) and (len(forced) + 1, V) rows."""
    msd = merged_state_dict(sd, lora_sd, s)
    lm_input = build_lm_input(sd, lora_sd, s, cfg, text, prompt_text, prompt_speech_token)
    cache = ol.KVCache(cfg.num_layers)
    x, rows = lm_input, []
    for i in range(len(forced) + 1):
        y = ol.qwen2_forward(msd, cfg, x, cache)
        rows.append(ol.logits_to_logp(msd, y[:, -1]).squeeze(0))
        if i < len(forced):
            x = sd["speech_embedding.weight"][forced[i]].reshape(1, 1, -1)      # llm.py:874: the BASE row, whatever the adapter
    return lm_input, torch.stack(rows)
