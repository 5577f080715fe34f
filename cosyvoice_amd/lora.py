"""Per-speaker LoRA adapters of the speech LM: the fork ships voices as one base model plus LoRA-only checkpoints
(bin/ckpt_resave.py:441-461,605-663 -> llm_v2_lora_*.pt; cosyvoice/loralib wraps every Linear / Embedding, r = 16, alpha = 16 in
examples/tts_vc/cosyvoice2/conf/cosyvoice_pho_lora.yaml).  ``LoraBank`` holds up to ``max_adapters`` of them on the device in the layout
the kernels of include/cosyvoice_amd_lora.h read, so every row of a decode batch can use its own voice over ONE base weight stream:

    bank = LoraBank(lm, max_adapters=8, r=16)
    bank.add("alice", torch.load("llm_v2_lora_0.pt"), alpha=16)
    lm.attach_lora(bank)
    lm.generate_batch(texts, prompt_texts, prompt_speech, adapters=["alice", -1, "alice"])     # -1: base model only

Which tensors take part at inference is decided by the reference's Qwen2LM.inference (llm/llm.py:824-874):
  * adapted: the 7 Linears of every decoder layer, llm_decoder, and — in the prefill assembly only — embed_tokens(text) (:840) and
    speech_embedding(prompt_speech_token) (:849), which are module CALLS;
  * not adapted: llm_embedding.weight[...] (:846-847) and the decode-step input speech_embedding.weight[top_ids] (:874), raw ``.weight``
    reads that see the base rows, and llm.model.lm_head, which is never called.  The ``lora_*`` keys of llm_embedding and lm_head are
    therefore accepted and ignored, and the speech_embedding adapter is used for the prompt rows alone.
"""
from typing import Dict, Optional

import torch

_IGNORED = ("llm_embedding", "llm.model.lm_head")      # llm.py:846-847 raw .weight reads; lm_head is never called


class LoraBank:
    """Device banks for ``max_adapters`` rank-``r`` adapters of ``lm`` (a Qwen2LM: its cfg, 16-bit dtype and device), all allocated
    here; ``add`` / ``remove`` only write into them, so captured decode graphs (which hold the banks' addresses) stay valid.  Values are
    rounded to the LM's 16-bit type once, at ``add``."""

    def __init__(self, lm, max_adapters: int, r: int = 16):
        if r not in (8, 16, 32):
            raise ValueError("LoRA rank must be 8, 16 or 32")
        cfg, dt, dev = lm.cfg, lm.dtype, lm.device
        if dt not in (torch.float16, torch.bfloat16):
            raise ValueError("LoraBank needs the LM's 16-bit dtype")
        self.cfg, self.dtype, self.device, self.r, self.max_adapters = cfg, dt, dev, r, int(max_adapters)
        assert self.max_adapters >= 1
        S, H, I = self.max_adapters, cfg.hidden_size, cfg.intermediate_size
        self.qkv_dim = cfg.q_dim + 2 * cfg.kv_dim
        z = lambda *s, dtype=dt: torch.zeros(*s, device=dev, dtype=dtype)
        self.layers = []
        for _ in range(cfg.num_layers):
            lay = dict(A_qkv=z(S, 3 * r, H), B_qkv=z(S, self.qkv_dim, r), A_o=z(S, r, cfg.q_dim), B_o=z(S, H, r),
                       A_gu=z(S, 2 * r, H), B_gu=z(S, 2 * I, r), A_down=z(S, r, I), B_down=z(S, H, r))
            lay["B_gate"], lay["B_up"] = lay["B_gu"][:, :I], lay["B_gu"][:, I:]      # views: gate rows, then up rows (CV_LORA_SWIGLU)
            self.layers.append(lay)
        self.A_dec, self.B_dec = z(S, r, H), z(S, cfg.out_vocab, r)
        # embeddings: A^T (vocab, r) so that a token gathers one contiguous row (loralib/layers.py:118-122)
        self.AT_embed, self.B_embed = z(S, cfg.vocab_size, r), z(S, H, r)
        self.AT_speech, self.B_speech = z(S, cfg.out_vocab, r), z(S, H, r)
        self.s = z(S, dtype=torch.float32)
        self._slots: Dict[str, int] = {}
        # q | k | v column segments of the stacked B_qkv, each reading its own r columns of u (cv_lora_segment)
        self.qkv_segments = [(0, cfg.q_dim, 0), (cfg.q_dim, cfg.q_dim + cfg.kv_dim, r), (cfg.q_dim + cfg.kv_dim, self.qkv_dim, 2 * r)]
        self.gu_segments = [(0, I, 0), (I, 2 * I, r)]

    # ------------------------------------------------------------------ slots
    def slot(self, name: str) -> int:
        if name not in self._slots:
            raise KeyError(f"no LoRA adapter named {name!r} in this bank")
        return self._slots[name]

    def names(self):
        return dict(self._slots)

    def resolve(self, a) -> int:
        """An entry of ``adapters=``: a name, a slot index, or -1 (base model only)."""
        if isinstance(a, str):
            return self.slot(a)
        a = int(a)
        if a < -1 or a >= self.max_adapters:
            raise ValueError(f"adapter slot {a} outside [-1, {self.max_adapters})")
        return a

    def _targets(self, slot):
        """reference module name -> (destination of lora_A, transposed?, destination of lora_B) for one slot."""
        r, cfg = self.r, self.cfg
        q, kv = cfg.q_dim, cfg.kv_dim
        out = {}
        for i, lay in enumerate(self.layers):
            p = f"llm.model.model.layers.{i}."
            out[p + "self_attn.q_proj"] = (lay["A_qkv"][slot, 0:r], False, lay["B_qkv"][slot, 0:q])
            out[p + "self_attn.k_proj"] = (lay["A_qkv"][slot, r:2 * r], False, lay["B_qkv"][slot, q:q + kv])
            out[p + "self_attn.v_proj"] = (lay["A_qkv"][slot, 2 * r:3 * r], False, lay["B_qkv"][slot, q + kv:q + 2 * kv])
            out[p + "self_attn.o_proj"] = (lay["A_o"][slot], False, lay["B_o"][slot])
            out[p + "mlp.gate_proj"] = (lay["A_gu"][slot, 0:r], False, lay["B_gate"][slot])
            out[p + "mlp.up_proj"] = (lay["A_gu"][slot, r:2 * r], False, lay["B_up"][slot])
            out[p + "mlp.down_proj"] = (lay["A_down"][slot], False, lay["B_down"][slot])
        out["llm_decoder"] = (self.A_dec[slot], False, self.B_dec[slot])
        out["llm.model.model.embed_tokens"] = (self.AT_embed[slot], True, self.B_embed[slot])
        out["speech_embedding"] = (self.AT_speech[slot], True, self.B_speech[slot])
        return out

    def add(self, name: str, state_dict, alpha: Optional[float] = None, noscale: bool = False) -> int:
        """Load one LoRA-only checkpoint (the reference's key names, as loralib.replace_specific_layer_4lora produces them on its
        Qwen2LM) into a free slot, or over the slot ``name`` already has.  ``alpha``: the run's lora_alpha (default r, the fork's
        configs); the scale is alpha / r, or 1 with ``noscale`` (an init string containing "noscale", loralib/layers.py:152).  Modules
        the checkpoint leaves out (lora_skip_modules) keep a zero B.  Keys without ``lora_`` (a ``bias = all`` save) are not read."""
        keys = [k for k in state_dict if "lora_" in k or "weight_cache" in k]
        cache = [k for k in keys if "weight_cache" in k]
        if cache:
            raise ValueError(f"the cachewnorm LoRA variant is not supported (weight_cache keys): {cache[:4]}")
        slot = self._slots.get(name)
        if slot is None:
            used = set(self._slots.values())
            free = [i for i in range(self.max_adapters) if i not in used]
            if not free:
                raise RuntimeError(f"LoraBank is full ({self.max_adapters} adapters)")
            slot = free[0]
        tg = self._targets(slot)
        foreign, bad_rank, todo = [], [], []
        for k in keys:
            mod, _, ab = k.rpartition(".lora_")
            if ab not in ("A", "B") or not (mod in tg or mod in _IGNORED):
                foreign.append(k)
                continue
            if mod in _IGNORED:
                continue    # llm.py:846-847: llm_embedding is read through .weight; lm_head is never called
            t = state_dict[k]
            a_dst, transposed, b_dst = tg[mod]
            want = (tuple(a_dst.shape[::-1]) if transposed else tuple(a_dst.shape)) if ab == "A" else tuple(b_dst.shape)
            if t.dim() != 2 or (t.shape[0] if ab == "A" else t.shape[1]) != self.r:
                bad_rank.append(k)
            elif tuple(t.shape) != want:
                foreign.append(k)
            else:
                todo.append((a_dst if ab == "A" else b_dst, t.t() if (ab == "A" and transposed) else t))
        if foreign:
            raise ValueError(f"LoRA keys of modules the speech LM does not have (or of another shape): {foreign[:6]}")
        if bad_rank:
            raise ValueError(f"LoRA rank differs from the bank's r = {self.r}: {bad_rank[:6]}")
        self._clear(slot)
        for dst, t in todo:
            dst.copy_(t.detach().to(torch.float32).to(self.dtype))
        self.s[slot] = 1.0 if noscale else float(self.r if alpha is None else alpha) / self.r
        self._slots[name] = slot
        return slot

    def _clear(self, slot):
        for lay in self.layers:
            for k in ("A_qkv", "B_qkv", "A_o", "B_o", "A_gu", "B_gu", "A_down", "B_down"):
                lay[k][slot].zero_()
        for t in (self.A_dec, self.B_dec, self.AT_embed, self.B_embed, self.AT_speech, self.B_speech):
            t[slot].zero_()
        self.s[slot] = 0.0

    def remove(self, name: str) -> None:
        """Free the adapter's slot.  Its banks are zeroed: a row that still names the slot gets the base model."""
        self._clear(self._slots.pop(name))

