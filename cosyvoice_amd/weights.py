"""Deterministic, key-name-seeded synthetic state dicts with the reference's key names.

No checkpoint exists in the build environment, so parity and the
benchmark run on synthetic weights.  Every tensor is drawn from a CPU
``torch.Generator`` seeded by a hash of its state-dict key, so the same bytes are
regenerated on any machine (here to mint goldens through the reference's own
``load_state_dict``; on the GPU box to feed the HIP path and the oracle).

Key names follow the reference module tree (SURVEY.md §8b "State-dict contract"):
  hift : /root/reference/cosyvoice/hifigan/generator.py:268-316, f0_predictor.py:27-50
  flow : /root/reference/cosyvoice/flow/flow.py:195-201, flow/decoder.py:110-206,
         transformer/upsample_encoder.py:177-235, transformer/attention.py:44-48,216-221
  llm  : /root/reference/cosyvoice/llm/llm.py:786-801 + HF Qwen2 module names
"""
import hashlib
import math
from typing import Dict, List, Tuple

import torch

from .config import FlowConfig, HiftConfig, LlmConfig

Spec = Tuple[str, Tuple[int, ...], str, float]  # key, shape, kind, param


def _seed(key: str, base: int) -> int:
    h = hashlib.sha256(f"{base}:{key}".encode()).digest()
    return int.from_bytes(h[:8], "little") & 0x7FFFFFFFFFFFFFFF


def _draw(key: str, shape, kind: str, param: float, base: int) -> torch.Tensor:
    g = torch.Generator(device="cpu")
    g.manual_seed(_seed(key, base))
    if kind == "normal":
        return torch.randn(shape, generator=g, dtype=torch.float32) * param
    if kind == "uniform":  # U(-param, param)
        return (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * param
    if kind == "norm_w":  # LayerNorm / RMSNorm gain
        return 1.0 + torch.randn(shape, generator=g, dtype=torch.float32) * param
    if kind == "alpha":  # snake alpha in (0.5, 1.5)
        return 0.5 + torch.rand(shape, generator=g, dtype=torch.float32)
    if kind == "const":
        return torch.full(shape, param, dtype=torch.float32)
    raise ValueError(kind)


def materialize(specs: List[Spec], base_seed: int = 1986, round_to: torch.dtype = None) -> Dict[str, torch.Tensor]:
    """Draw every tensor of ``specs``.  ``weight_g`` entries (kind 'wn_g') are derived
    from the already-drawn ``weight_v`` so that g = ||v|| * U(0.7, 1.3) exercises the
    legacy weight-norm fold."""
    sd: Dict[str, torch.Tensor] = {}
    for key, shape, kind, param in specs:
        if kind == "wn_g":
            continue
        sd[key] = _draw(key, shape, kind, param, base_seed)
    for key, shape, kind, param in specs:
        if kind != "wn_g":
            continue
        v = sd[key[:-1] + "v"]
        nrm = v.reshape(v.shape[0], -1).norm(dim=1).reshape(shape)
        g = torch.Generator(device="cpu")
        g.manual_seed(_seed(key, base_seed))
        sd[key] = nrm * (0.7 + 0.6 * torch.rand(shape, generator=g, dtype=torch.float32))
    if round_to is not None:
        for k in sd:
            sd[k] = sd[k].to(round_to).to(torch.float32)
    return sd


# --------------------------------------------------------------------------- HiFT
def _wn_conv(specs, name, cout, cin, k, std, transpose=False, bias_std=0.02):
    shape = (cin, cout, k) if transpose else (cout, cin, k)
    d0 = shape[0]
    specs.append((f"{name}.weight_v", shape, "normal", std))
    specs.append((f"{name}.weight_g", (d0, 1, 1), "wn_g", 0.0))
    specs.append((f"{name}.bias", (cout,), "normal", bias_std))


def _resblock(specs, name, ch, k, dils):
    for j in range(len(dils)):
        _wn_conv(specs, f"{name}.convs1.{j}", ch, ch, k, 0.01)
        _wn_conv(specs, f"{name}.convs2.{j}", ch, ch, k, 0.01)
    for j in range(len(dils)):
        specs.append((f"{name}.activations1.{j}.alpha", (ch,), "alpha", 0.0))
        specs.append((f"{name}.activations2.{j}.alpha", (ch,), "alpha", 0.0))


def hift_downsample_plan(cfg: HiftConfig):
    """(stride u, kernel, padding) of each source_downs conv — generator.py:289-300."""
    ups = list(cfg.upsample_rates)
    down = [1] + ups[::-1][:-1]
    cum = []
    c = 1
    for d in down:
        c *= d
        cum.append(c)
    plan = []
    for u in cum[::-1]:
        if u == 1:
            plan.append((1, 1, 0))
        else:
            plan.append((u, u * 2, u // 2))
    return plan


def hift_specs(cfg: HiftConfig) -> List[Spec]:
    s: List[Spec] = []
    nh = cfg.nb_harmonics + 1
    s.append(("m_source.l_linear.weight", (1, nh), "uniform", 1.0 / math.sqrt(nh)))
    s.append(("m_source.l_linear.bias", (1,), "uniform", 1.0 / math.sqrt(nh)))
    bc = cfg.base_channels
    _wn_conv(s, "conv_pre", bc, cfg.in_channels, 7, 1.0 / math.sqrt(cfg.in_channels * 7 * 3))
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        _wn_conv(s, f"ups.{i}", bc // 2 ** (i + 1), bc // 2 ** i, k, 0.01, transpose=True)
    nfft2 = cfg.n_fft + 2
    for i, (stride, k, pad) in enumerate(hift_downsample_plan(cfg)):
        ch = bc // 2 ** (i + 1)
        bound = 1.0 / math.sqrt(nfft2 * k)
        s.append((f"source_downs.{i}.weight", (ch, nfft2, k), "uniform", bound))
        s.append((f"source_downs.{i}.bias", (ch,), "uniform", bound))
        _resblock(s, f"source_resblocks.{i}", ch, cfg.source_resblock_kernel_sizes[i],
                  cfg.source_resblock_dilation_sizes[i])
    nk = len(cfg.resblock_kernel_sizes)
    ch = bc
    for i in range(len(cfg.upsample_rates)):
        ch = bc // 2 ** (i + 1)
        for j, (k, d) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
            _resblock(s, f"resblocks.{i * nk + j}", ch, k, d)
    # conv_post: magnitude-channel bias pulled negative so exp() keeps the synthetic waveform unclipped
    s.append(("conv_post.weight_v", (nfft2, ch, 7), "normal", 0.01))
    s.append(("conv_post.weight_g", (nfft2, 1, 1), "wn_g", 0.0))
    s.append(("conv_post.bias", (nfft2,), "normal", 0.3))
    fc = cfg.f0_cond_channels
    cin = cfg.in_channels
    for idx in (0, 2, 4, 6, 8):
        _wn_conv(s, f"f0_predictor.condnet.{idx}", fc, cin, 3, 1.0 / math.sqrt(cin * 3))
        cin = fc
    # classifier scaled so the synthetic F0 spans voiced/unvoiced around the 10 Hz threshold
    s.append(("f0_predictor.classifier.weight", (1, fc), "normal", 40.0 / math.sqrt(fc)))
    s.append(("f0_predictor.classifier.bias", (1,), "const", 60.0))
    return s


# --------------------------------------------------------------------------- flow
def _linear(specs, name, out_f, in_f, bias=True, gain=1.0, bias_std=0.02):
    specs.append((f"{name}.weight", (out_f, in_f), "normal", gain / math.sqrt(in_f)))
    if bias:
        specs.append((f"{name}.bias", (out_f,), "normal", bias_std))


def _conv(specs, name, cout, cin, k, gain=1.0, bias_std=0.02):
    specs.append((f"{name}.weight", (cout, cin, k), "normal", gain / math.sqrt(cin * k)))
    specs.append((f"{name}.bias", (cout,), "normal", bias_std))


def _ln(specs, name, dim):
    specs.append((f"{name}.weight", (dim,), "norm_w", 0.1))
    specs.append((f"{name}.bias", (dim,), "normal", 0.05))


def _conformer_layer(specs, name, dim, heads, units):
    dk = dim // heads
    for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
        _linear(specs, f"{name}.self_attn.{n}", dim, dim)
    _linear(specs, f"{name}.self_attn.linear_pos", dim, dim, bias=False)
    bound = math.sqrt(6.0 / (heads + dk))
    specs.append((f"{name}.self_attn.pos_bias_u", (heads, dk), "uniform", bound))
    specs.append((f"{name}.self_attn.pos_bias_v", (heads, dk), "uniform", bound))
    _linear(specs, f"{name}.feed_forward.w_1", units, dim)
    _linear(specs, f"{name}.feed_forward.w_2", dim, units)
    _ln(specs, f"{name}.norm_ff", dim)
    _ln(specs, f"{name}.norm_mha", dim)


def _est_resnet(specs, name, cin, cout, tdim, norm_idx=2):
    for b, ci in (("block1", cin), ("block2", cout)):
        _conv(specs, f"{name}.{b}.block.0", cout, ci, 3)
        _ln(specs, f"{name}.{b}.block.{norm_idx}", cout)
    _linear(specs, f"{name}.mlp.1", cout, tdim)
    _conv(specs, f"{name}.res_conv", cout, cin, 1)


def _est_tblock(specs, name, dim, inner, ff):
    _ln(specs, f"{name}.norm1", dim)
    for n in ("to_q", "to_k", "to_v"):
        _linear(specs, f"{name}.attn1.{n}", inner, dim, bias=False)
    _linear(specs, f"{name}.attn1.to_out.0", dim, inner, gain=0.5)
    _ln(specs, f"{name}.norm3", dim)
    _linear(specs, f"{name}.ff.net.0.proj", ff, dim)
    _linear(specs, f"{name}.ff.net.2", dim, ff, gain=0.5)


def estimator_specs(cfg: FlowConfig, prefix: str = "decoder.estimator.") -> List[Spec]:
    s: List[Spec] = []
    C, tdim = cfg.est_channels, cfg.est_time_dim
    inner, ff = cfg.est_inner, cfg.est_channels * cfg.est_ff_mult
    _linear(s, f"{prefix}time_mlp.linear_1", tdim, cfg.est_in_channels)
    _linear(s, f"{prefix}time_mlp.linear_2", tdim, tdim)
    _est_resnet(s, f"{prefix}down_blocks.0.0", cfg.est_in_channels, C, tdim)
    for j in range(cfg.est_n_blocks):
        _est_tblock(s, f"{prefix}down_blocks.0.1.{j}", C, inner, ff)
    _conv(s, f"{prefix}down_blocks.0.2", C, C, 3)
    for i in range(cfg.est_mid_blocks):
        _est_resnet(s, f"{prefix}mid_blocks.{i}.0", C, C, tdim)
        for j in range(cfg.est_n_blocks):
            _est_tblock(s, f"{prefix}mid_blocks.{i}.1.{j}", C, inner, ff)
    _est_resnet(s, f"{prefix}up_blocks.0.0", 2 * C, C, tdim)
    for j in range(cfg.est_n_blocks):
        _est_tblock(s, f"{prefix}up_blocks.0.1.{j}", C, inner, ff)
    _conv(s, f"{prefix}up_blocks.0.2", C, C, 3)
    _conv(s, f"{prefix}final_block.block.0", C, C, 3)
    _ln(s, f"{prefix}final_block.block.2", C)
    _conv(s, f"{prefix}final_proj", cfg.output_size, C, 1)
    return s


def encoder_specs(cfg: FlowConfig, prefix: str = "encoder.") -> List[Spec]:
    s: List[Spec] = []
    D = cfg.enc_dim
    _linear(s, f"{prefix}embed.out.0", D, cfg.input_size)
    _ln(s, f"{prefix}embed.out.1", D)
    _ln(s, f"{prefix}after_norm", D)
    _conv(s, f"{prefix}pre_lookahead_layer.conv1", D, D, cfg.pre_lookahead_len + 1)
    _conv(s, f"{prefix}pre_lookahead_layer.conv2", D, D, 3)
    for i in range(cfg.enc_blocks):
        _conformer_layer(s, f"{prefix}encoders.{i}", D, cfg.enc_heads, cfg.enc_linear_units)
    _conv(s, f"{prefix}up_layer.conv", D, D, 5)
    _linear(s, f"{prefix}up_embed.out.0", D, cfg.input_size)
    _ln(s, f"{prefix}up_embed.out.1", D)
    for i in range(cfg.enc_up_blocks):
        _conformer_layer(s, f"{prefix}up_encoders.{i}", D, cfg.enc_heads, cfg.enc_linear_units)
    return s


def flow_specs(cfg: FlowConfig) -> List[Spec]:
    s: List[Spec] = []
    s.append(("input_embedding.weight", (cfg.vocab_size, cfg.input_size), "normal", 1.0))
    _linear(s, "spk_embed_affine_layer", cfg.output_size, cfg.spk_embed_dim, gain=3.0)
    s += encoder_specs(cfg)
    _linear(s, "encoder_proj", cfg.output_size, cfg.enc_dim)
    s += estimator_specs(cfg)
    return s


# --------------------------------------------------------------------------- llm
def llm_specs(cfg: LlmConfig) -> List[Spec]:
    s: List[Spec] = []
    H, I = cfg.hidden_size, cfg.intermediate_size
    p = "llm.model.model."
    s.append((f"{p}embed_tokens.weight", (cfg.vocab_size, H), "normal", 0.02))
    for i in range(cfg.num_layers):
        lp = f"{p}layers.{i}."
        s.append((f"{lp}self_attn.q_proj.weight", (cfg.q_dim, H), "normal", 1.0 / math.sqrt(H)))
        s.append((f"{lp}self_attn.q_proj.bias", (cfg.q_dim,), "normal", 0.1))
        s.append((f"{lp}self_attn.k_proj.weight", (cfg.kv_dim, H), "normal", 1.0 / math.sqrt(H)))
        s.append((f"{lp}self_attn.k_proj.bias", (cfg.kv_dim,), "normal", 0.1))
        s.append((f"{lp}self_attn.v_proj.weight", (cfg.kv_dim, H), "normal", 1.0 / math.sqrt(H)))
        s.append((f"{lp}self_attn.v_proj.bias", (cfg.kv_dim,), "normal", 0.1))
        s.append((f"{lp}self_attn.o_proj.weight", (H, cfg.q_dim), "normal", 0.5 / math.sqrt(cfg.q_dim)))
        s.append((f"{lp}mlp.gate_proj.weight", (I, H), "normal", 1.0 / math.sqrt(H)))
        s.append((f"{lp}mlp.up_proj.weight", (I, H), "normal", 1.0 / math.sqrt(H)))
        s.append((f"{lp}mlp.down_proj.weight", (H, I), "normal", 0.5 / math.sqrt(I)))
        s.append((f"{lp}input_layernorm.weight", (H,), "norm_w", 0.1))
        s.append((f"{lp}post_attention_layernorm.weight", (H,), "norm_w", 0.1))
    s.append((f"{p}norm.weight", (H,), "norm_w", 0.1))
    if not cfg.tie_word_embeddings:
        s.append(("llm.model.lm_head.weight", (cfg.vocab_size, H), "normal", 0.02))
    s.append(("llm_embedding.weight", (2, H), "normal", 0.02))
    s.append(("llm_decoder.weight", (cfg.out_vocab, H), "normal", 2.0 / math.sqrt(H)))
    s.append(("llm_decoder.bias", (cfg.out_vocab,), "normal", 0.1))
    s.append(("speech_embedding.weight", (cfg.out_vocab, H), "normal", 0.02))
    return s


def hift_state_dict(cfg: HiftConfig, seed: int = 1986):
    return materialize(hift_specs(cfg), seed)


def flow_state_dict(cfg: FlowConfig, seed: int = 1986, round_to=None):
    return materialize(flow_specs(cfg), seed, round_to)


def llm_state_dict(cfg: LlmConfig, seed: int = 1986, round_to=None):
    sd = materialize(llm_specs(cfg), seed, round_to)
    if cfg.tie_word_embeddings:
        sd["llm.model.lm_head.weight"] = sd["llm.model.model.embed_tokens.weight"]
    return sd


LLM_LORA_LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                    "mlp.down_proj")


def llm_lora_modules(cfg: LlmConfig):
    """(module name, kind, in_features / vocab, out_features / dim) of every module of the reference Qwen2LM that
    loralib.replace_specific_layer_4lora wraps (loralib/utils.py:102-214): the seven Linears of each decoder layer, llm_decoder, and
    the Embeddings / Linear that Qwen2LM.inference never calls as modules (llm_embedding, lm_head) or calls in the prefill assembly only
    (embed_tokens, speech_embedding)."""
    H, I = cfg.hidden_size, cfg.intermediate_size
    dims = {"self_attn.q_proj": (H, cfg.q_dim), "self_attn.k_proj": (H, cfg.kv_dim), "self_attn.v_proj": (H, cfg.kv_dim),
            "self_attn.o_proj": (cfg.q_dim, H), "mlp.gate_proj": (H, I), "mlp.up_proj": (H, I), "mlp.down_proj": (I, H)}
    mods = [("llm.model.model.embed_tokens", "embedding", cfg.vocab_size, H)]
    for i in range(cfg.num_layers):
        mods += [(f"llm.model.model.layers.{i}.{n}", "linear", *dims[n]) for n in LLM_LORA_LINEARS]
    mods += [("llm.model.lm_head", "linear", H, cfg.vocab_size), ("llm_embedding", "embedding", 2, H),
             ("llm_decoder", "linear", H, cfg.out_vocab), ("speech_embedding", "embedding", cfg.out_vocab, H)]
    return mods


def llm_lora_state_dict(cfg: LlmConfig, r: int = 16, seed: int = 1986, gain: float = 0.02, round_to=None):
    """A synthetic LoRA-only checkpoint of the speech LM with the reference's key names (``<module>.lora_A`` (r, in) and
    ``<module>.lora_B`` (out, r), loralib/layers.py:49-50,150-151), key-seeded like every other fixture, with NON-ZERO B (a trained
    adapter; the reference initialises B = 0).  Linear: A ~ N(0, 1 / in), B ~ N(0, gain^2 / r), so the low-rank term of a unit-rms input
    has standard deviation about ``gain`` per output.  Embedding: A ~ N(0, 1) (the reference's init), B ~ N(0, (0.02 gain)^2 / r)
    against base rows of N(0, 0.02^2)."""
    specs: List[Spec] = []
    for name, kind, n_in, n_out in llm_lora_modules(cfg):
        if kind == "linear":
            specs.append((f"{name}.lora_A", (r, n_in), "normal", 1.0 / math.sqrt(n_in)))
            specs.append((f"{name}.lora_B", (n_out, r), "normal", gain / math.sqrt(r)))
        else:
            specs.append((f"{name}.lora_A", (r, n_in), "normal", 1.0))
            specs.append((f"{name}.lora_B", (n_out, r), "normal", 0.02 * gain / math.sqrt(r)))
    return materialize(specs, seed, round_to)


def fold_weight_norm(sd: Dict[str, torch.Tensor], name: str) -> torch.Tensor:
    """w = g * v / ||v||, norm over dims (1,2) per index of dim 0 (legacy torch weight_norm, dim=0);
    for ConvTranspose1d that is per *input* channel."""
    if f"{name}.weight" in sd:
        return sd[f"{name}.weight"]
    v, g = sd[f"{name}.weight_v"], sd[f"{name}.weight_g"]
    nrm = v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)
    return v * (g / nrm)


# --------------------------------------------------------------------------- BigVGAN
def bigvgan_specs(cfg) -> List[Spec]:
    """Keys of the reference's BigVGAN module tree (BigVGAN/bigvgan.py:257-382) for encoder1 = encoder2 = None."""
    s: List[Spec] = []
    s.append(("input_embedding.weight", (cfg.vocab_size, cfg.input_size), "normal", 1.0))
    _linear(s, "encoder_proj", cfg.output_size, cfg.input_size)
    c0 = cfg.upsample_initial_channel
    _linear(s, "mel_proj", cfg.mel_bin, c0)
    _wn_conv(s, "conv_pre", c0, cfg.output_size, 7, 1.0 / math.sqrt(cfg.output_size * 7))
    sd = cfg.speaker_embedding_dim
    s.append(("cond_layer.weight", (c0, sd, 1), "normal", 0.5 / math.sqrt(sd)))
    s.append(("cond_layer.bias", (c0,), "normal", 0.02))
    nk = len(cfg.resblock_kernel_sizes)
    ch = c0
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        ch = c0 // 2 ** (i + 1)
        _wn_conv(s, f"ups.{i}.0", ch, c0 // 2 ** i, k, 1.0 / math.sqrt(c0 // 2 ** i * k / u), transpose=True)
        if cfg.cond_in_each_up_layer:
            s.append((f"conds.{i}.weight", (ch, sd, 1), "normal", 0.5 / math.sqrt(sd)))
            s.append((f"conds.{i}.bias", (ch,), "normal", 0.02))
        for j, (k2, dils) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
            name = f"resblocks.{i * nk + j}"
            for d in range(len(dils)):
                _wn_conv(s, f"{name}.convs1.{d}", ch, ch, k2, 0.5 / math.sqrt(ch * k2))
                _wn_conv(s, f"{name}.convs2.{d}", ch, ch, k2, 0.5 / math.sqrt(ch * k2))
            for m in range(2 * len(dils)):
                s.append((f"{name}.activations.{m}.act.alpha", (ch,), "normal", 0.3))   # log-scale parameters
                s.append((f"{name}.activations.{m}.act.beta", (ch,), "normal", 0.3))
    s.append(("activation_post.act.alpha", (ch,), "normal", 0.3))
    s.append(("activation_post.act.beta", (ch,), "normal", 0.3))
    _wn_conv(s, "conv_post", 1, ch, 7, 0.3 / math.sqrt(ch * 7))   # keeps tanh out of saturation on synthetic weights
    return s


def bigvgan_state_dict(cfg, seed: int = 0, round_to=None) -> Dict[str, torch.Tensor]:
    return materialize(bigvgan_specs(cfg), seed, round_to)


# --------------------------------------------------------------------------- Qwen2LM_Phoneme_Src2
def phoneme_lm_specs(pcfg, lcfg: LlmConfig) -> List[Spec]:
    """llm.py:1482-1531 module tree: text_embedding.{0..3}, text_encoder (ConformerEncoder), text_encoder_affine_layer,
    src_attention.0 (DecoderLayer), spk_embed_affine_layer + the Qwen2 stack / llm_embedding / llm_decoder / speech_embedding."""
    s: List[Spec] = llm_specs(lcfg)
    H, D = lcfg.hidden_size, pcfg.enc_dim
    for i, (n, d) in enumerate(((pcfg.text_token_size, pcfg.text_token_dim), (pcfg.text_tone_size, pcfg.text_tone_dim),
                                (pcfg.text_lang_size, pcfg.text_lang_dim), (pcfg.text_prsd_size, pcfg.text_prsd_dim))):
        s.append((f"text_embedding.{i}.weight", (n, d), "normal", 1.0))
    _linear(s, "text_encoder.embed.out.0", D, pcfg.input_size)
    _ln(s, "text_encoder.embed.out.1", D)
    _ln(s, "text_encoder.after_norm", D)
    for i in range(pcfg.enc_blocks):
        _conformer_layer(s, f"text_encoder.encoders.{i}", D, pcfg.enc_heads, pcfg.enc_linear_units)
    _linear(s, "text_encoder_affine_layer", H, D)
    for att in ("self_attn", "src_attn"):
        for lin in ("linear_q", "linear_k", "linear_v", "linear_out"):
            _linear(s, f"src_attention.0.{att}.{lin}", H, H, gain=(0.5 if lin == "linear_out" else 1.0))
    _linear(s, "src_attention.0.feed_forward.w_1", pcfg.src_linear_units, H)
    _linear(s, "src_attention.0.feed_forward.w_2", H, pcfg.src_linear_units, gain=0.5)
    for n in ("norm1", "norm2", "norm3"):
        _ln(s, f"src_attention.0.{n}", H)
    _linear(s, "spk_embed_affine_layer", H, pcfg.spk_embed_dim)
    return s


def phoneme_lm_state_dict(pcfg, lcfg: LlmConfig, seed: int = 1986, round_to=None):
    sd = materialize(phoneme_lm_specs(pcfg, lcfg), seed, round_to)
    if lcfg.tie_word_embeddings:
        sd["llm.model.lm_head.weight"] = sd["llm.model.model.embed_tokens.weight"]
    return sd


# --------------------------------------------------------------------------- CosyVoice-v1 TransformerLM
def _transformer_layer(specs, name, dim, heads, units):
    """TransformerEncoderLayer with rel-pos attention (encoder_layer.py:24-107): same tensors as a conformer layer, norm1 / norm2."""
    dk = dim // heads
    for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
        _linear(specs, f"{name}.self_attn.{n}", dim, dim)
    _linear(specs, f"{name}.self_attn.linear_pos", dim, dim, bias=False)
    bound = math.sqrt(6.0 / (heads + dk))
    specs.append((f"{name}.self_attn.pos_bias_u", (heads, dk), "uniform", bound))
    specs.append((f"{name}.self_attn.pos_bias_v", (heads, dk), "uniform", bound))
    _linear(specs, f"{name}.feed_forward.w_1", units, dim)
    _linear(specs, f"{name}.feed_forward.w_2", dim, units)
    _ln(specs, f"{name}.norm1", dim)
    _ln(specs, f"{name}.norm2", dim)


def transformer_lm_specs(cfg) -> List[Spec]:
    s: List[Spec] = []
    s.append(("text_embedding.weight", (cfg.text_token_size, cfg.text_encoder_input_size), "normal", 1.0))
    _linear(s, "text_encoder.embed.out.0", cfg.enc_dim, cfg.text_encoder_input_size)
    _ln(s, "text_encoder.embed.out.1", cfg.enc_dim)
    _ln(s, "text_encoder.after_norm", cfg.enc_dim)
    for i in range(cfg.enc_blocks):
        _conformer_layer(s, f"text_encoder.encoders.{i}", cfg.enc_dim, cfg.enc_heads, cfg.enc_linear_units)
    _linear(s, "text_encoder_affine_layer", cfg.llm_dim, cfg.enc_dim)
    s.append(("llm_embedding.weight", (2, cfg.llm_dim), "normal", 1.0))
    _linear(s, "llm.embed.out.0", cfg.llm_dim, cfg.llm_dim)
    _ln(s, "llm.embed.out.1", cfg.llm_dim)
    _ln(s, "llm.after_norm", cfg.llm_dim)
    for i in range(cfg.llm_blocks):
        _transformer_layer(s, f"llm.encoders.{i}", cfg.llm_dim, cfg.llm_heads, cfg.llm_linear_units)
    _linear(s, "llm_decoder", cfg.speech_token_size + 1, cfg.llm_dim, gain=2.0, bias_std=0.1)
    s.append(("speech_embedding.weight", (cfg.speech_token_size, cfg.llm_dim), "normal", 1.0))
    _linear(s, "spk_embed_affine_layer", cfg.llm_dim, cfg.spk_embed_dim)
    return s


def transformer_lm_state_dict(cfg, seed: int = 1986, round_to=None):
    return materialize(transformer_lm_specs(cfg), seed, round_to)


# --------------------------------------------------------------------------- CosyVoice-v1 flow (MaskedDiffWithXvec)
def estimator_v1_specs(cfg, prefix: str = "decoder.estimator.") -> List[Spec]:
    """Non-causal ConditionalDecoder channels=[C, C] (flow/decoder.py:110-206): down_blocks.0 ends in Downsample1D (`.2.conv`,
    k3 stride 2), down_blocks.1 in a plain Conv1d, up_blocks.0 in Upsample1D (`.2.conv`, ConvTranspose1d(4,2,1)), up_blocks.1
    in a plain Conv1d; every Block1D norm is a GroupNorm at `.block.1` (Conv1d, GroupNorm, Mish; the causal block has a Transpose in between)."""
    s: List[Spec] = []
    C, tdim = cfg.est_channels, cfg.est_time_dim
    inner, ff = cfg.est_inner, cfg.est_channels * cfg.est_ff_mult
    _linear(s, f"{prefix}time_mlp.linear_1", tdim, cfg.est_in_channels)
    _linear(s, f"{prefix}time_mlp.linear_2", tdim, tdim)

    def stage(name, cin):
        _est_resnet(s, f"{name}.0", cin, C, tdim, norm_idx=1)
        for j in range(cfg.est_n_blocks):
            _est_tblock(s, f"{name}.1.{j}", C, inner, ff)

    stage(f"{prefix}down_blocks.0", cfg.est_in_channels)
    _conv(s, f"{prefix}down_blocks.0.2.conv", C, C, 3)
    stage(f"{prefix}down_blocks.1", C)
    _conv(s, f"{prefix}down_blocks.1.2", C, C, 3)
    for i in range(cfg.est_mid_blocks):
        stage(f"{prefix}mid_blocks.{i}", C)
    stage(f"{prefix}up_blocks.0", 2 * C)
    s.append((f"{prefix}up_blocks.0.2.conv.weight", (C, C, 4), "normal", 1.0 / math.sqrt(C * 2)))
    s.append((f"{prefix}up_blocks.0.2.conv.bias", (C,), "normal", 0.02))
    stage(f"{prefix}up_blocks.1", 2 * C)
    _conv(s, f"{prefix}up_blocks.1.2", C, C, 3)
    _conv(s, f"{prefix}final_block.block.0", C, C, 3)
    _ln(s, f"{prefix}final_block.block.1", C)
    _conv(s, f"{prefix}final_proj", cfg.output_size, C, 1)
    return s


def flow_v1_specs(cfg) -> List[Spec]:
    """flow/flow.py:47-62 module tree: input_embedding, spk_embed_affine_layer, encoder (ConformerEncoder), encoder_proj,
    length_regulator.model (Conv1d k3, GroupNorm, Mish) x reg_layers + Conv1d k1, decoder.estimator."""
    s: List[Spec] = []
    D, O = cfg.enc_dim, cfg.output_size
    s.append(("input_embedding.weight", (cfg.vocab_size, cfg.input_size), "normal", 1.0))
    _linear(s, "spk_embed_affine_layer", O, cfg.spk_embed_dim, gain=3.0)
    _linear(s, "encoder.embed.out.0", D, cfg.input_size)
    _ln(s, "encoder.embed.out.1", D)
    _ln(s, "encoder.after_norm", D)
    for i in range(cfg.enc_blocks):
        _conformer_layer(s, f"encoder.encoders.{i}", D, cfg.enc_heads, cfg.enc_linear_units)
    _linear(s, "encoder_proj", O, D)
    for i in range(cfg.reg_layers):
        _conv(s, f"length_regulator.model.{3 * i}", O, O, 3)
        _ln(s, f"length_regulator.model.{3 * i + 1}", O)
    _conv(s, f"length_regulator.model.{3 * cfg.reg_layers}", O, O, 1)
    s += estimator_v1_specs(cfg)
    return s


def flow_v1_state_dict(cfg, seed: int = 1986, round_to=None):
    return materialize(flow_v1_specs(cfg), seed, round_to)


# --------------------------------------------------------------------------- CAM++ speaker encoder
# CAMPPlus(feat_dim=80, embedding_size=192) (speaker/speaker_encoder.py:154-159; module tree speaker/CAMPPlus.py:214-451).
CAMPPLUS_BLOCKS = ((12, 1), (24, 2), (16, 2))   # (layers, dilation) of block1..3; growth 32, bottleneck 128, k3
CAMPPLUS_EMBED = 192


def _campplus_bn(specs, name, ch, affine=True):
    """BatchNorm with running statistics: gain 1 + N(0, 0.1), bias and running_mean N(0, 0.1), running_var U(0.5, 1.5)."""
    if affine:
        specs.append((f"{name}.weight", (ch,), "norm_w", 0.1))
        specs.append((f"{name}.bias", (ch,), "normal", 0.1))
    specs.append((f"{name}.running_mean", (ch,), "normal", 0.1))
    specs.append((f"{name}.running_var", (ch,), "alpha", 0.0))
    specs.append((f"{name}.num_batches_tracked", (), "count", 0.0))


def _campplus_conv2d(specs, name, cout, cin, k):
    # nn.Conv2d's own initialiser: kaiming_uniform_(a=sqrt(5)) = U(+-1/sqrt(fan_in))
    specs.append((name, (cout, cin, k, k), "uniform", 1.0 / math.sqrt(cin * k * k)))


def _campplus_conv1d(specs, name, cout, cin, k, bias=False):
    # CAMPPlus.__init__ re-initialises every Conv1d: kaiming_normal_ (std sqrt(2 / fan_in)); biases drawn small instead of zero
    specs.append((f"{name}.weight", (cout, cin, k), "normal", math.sqrt(2.0 / (cin * k))))
    if bias:
        specs.append((f"{name}.bias", (cout,), "normal", 0.1))


def campplus_specs() -> List[Spec]:
    s: List[Spec] = []
    _campplus_conv2d(s, "head.conv1.weight", 32, 1, 3)
    _campplus_bn(s, "head.bn1", 32)
    for layer in ("layer1", "layer2"):
        for i in (0, 1):
            p = f"head.{layer}.{i}"
            _campplus_conv2d(s, f"{p}.conv1.weight", 32, 32, 3)
            _campplus_bn(s, f"{p}.bn1", 32)
            _campplus_conv2d(s, f"{p}.conv2.weight", 32, 32, 3)
            _campplus_bn(s, f"{p}.bn2", 32)
            if i == 0:
                _campplus_conv2d(s, f"{p}.shortcut.0.weight", 32, 32, 1)
                _campplus_bn(s, f"{p}.shortcut.1", 32)
    _campplus_conv2d(s, "head.conv2.weight", 32, 32, 3)
    _campplus_bn(s, "head.bn2", 32)
    _campplus_conv1d(s, "xvector.tdnn.linear", 128, 320, 5)
    _campplus_bn(s, "xvector.tdnn.nonlinear.batchnorm", 128)
    ch = 128
    for bi, (n, _) in enumerate(CAMPPLUS_BLOCKS, 1):
        for i in range(n):
            p = f"xvector.block{bi}.tdnnd{i + 1}"
            _campplus_bn(s, f"{p}.nonlinear1.batchnorm", ch + 32 * i)
            _campplus_conv1d(s, f"{p}.linear1", 128, ch + 32 * i, 1)
            _campplus_bn(s, f"{p}.nonlinear2.batchnorm", 128)
            _campplus_conv1d(s, f"{p}.cam_layer.linear_local", 32, 128, 3)
            _campplus_conv1d(s, f"{p}.cam_layer.linear1", 64, 128, 1, bias=True)
            _campplus_conv1d(s, f"{p}.cam_layer.linear2", 32, 64, 1, bias=True)
        ch += 32 * n
        _campplus_bn(s, f"xvector.transit{bi}.nonlinear.batchnorm", ch)
        _campplus_conv1d(s, f"xvector.transit{bi}.linear", ch // 2, ch, 1)
        ch //= 2
    _campplus_bn(s, "xvector.out_nonlinear.batchnorm", ch)
    _campplus_conv1d(s, "xvector.dense.linear", CAMPPLUS_EMBED, 2 * ch, 1)
    _campplus_bn(s, "xvector.dense.nonlinear.batchnorm", CAMPPLUS_EMBED, affine=False)
    return s


def campplus_state_dict(seed: int = 1986) -> Dict[str, torch.Tensor]:
    """Key-seeded CAM++ weights in the reference module's key order (num_batches_tracked = 0, int64)."""
    specs = campplus_specs()
    sd = materialize([sp for sp in specs if sp[2] != "count"], seed)
    return {k: (torch.zeros(shape, dtype=torch.int64) if kind == "count" else sd[k]) for k, shape, kind, _ in specs}


# --------------------------------------------------------------------------- speaker encoder v2 (512-d)
# SpeakerEmbedding (speaker/speaker_encoder.py:119-221): enc_q = PosteriorEncoder(513, 512, 512, 5, 1, 16) (posterior_encoder.py:24-27,
# WN modules.py:157-188), speaker_encoder = CAMPPlus(80, 192), style_encoder = StyleEncoder_v2(512, 256, 512, 5, 4, num_layers=6)
# (style_encoder.py:40-70), gst = GlobalStyleTokens_v2(4096, 512, 8, 6) (:131-146), speaker_adapter = StyleFuser(512, 192, "Add") (:165).
SPK2_SPEC, SPK2_HIDDEN, SPK2_WN_LAYERS, SPK2_WN_K = 513, 512, 16, 5
SPK2_STYLE_HIDDEN, SPK2_STYLE_HEADS, SPK2_STYLE_LAYERS, SPK2_STYLE_K = 256, 4, 6, 5
SPK2_GST_TOKENS, SPK2_GST_HEADS, SPK2_GST_LAYERS, SPK2_DIM = 4096, 8, 6, 512
# Gains over nn.Linear's own initialiser U(+-1/sqrt(fan_in)).  At that initialiser every softmax of the model is uniform (a wrong
# score moves nothing); these put the mean entropy of every style self-attention layer and every style-token layer at least one nat
# away from both uniform and one-hot on the committed cases (asserted where the goldens are minted, tests/golden/make_golden_style.py).
SPK2_GAINS = {"in_fc": 2.0, "spectral": 2.4, "mha_qk": 3.0, "gst_qk": 6.0, "gst_v": 5.0}


def _lin_u(specs, name, out_f, in_f, bias=True, gain=1.0):
    specs.append((f"{name}.weight", (out_f, in_f), "uniform", gain / math.sqrt(in_f)))
    if bias:
        specs.append((f"{name}.bias", (out_f,), "uniform", 1.0 / math.sqrt(in_f)))


def _wn_conv_bgv(specs, name, cout, cin, k):
    """Legacy weight_norm registration order: bias, weight_g, weight_v."""
    specs.append((f"{name}.bias", (cout,), "normal", 0.02))
    specs.append((f"{name}.weight_g", (cout, 1, 1), "wn_g", 0.0))
    specs.append((f"{name}.weight_v", (cout, cin, k), "normal", 1.0 / math.sqrt(cin * k)))


def posterior_encoder_specs(prefix: str = "enc_q.") -> List[Spec]:
    s: List[Spec] = []
    H = SPK2_HIDDEN
    _conv(s, f"{prefix}pre", H, SPK2_SPEC, 1)
    for i in range(SPK2_WN_LAYERS):
        _wn_conv_bgv(s, f"{prefix}enc.in_layers.{i}", 2 * H, H, SPK2_WN_K)
    for i in range(SPK2_WN_LAYERS):
        _wn_conv_bgv(s, f"{prefix}enc.res_skip_layers.{i}", 2 * H if i < SPK2_WN_LAYERS - 1 else H, H, 1)
    _conv(s, f"{prefix}proj", 2 * H, H, 1, gain=0.1)
    return s


def style_specs(gains=None) -> List[Spec]:
    """style_encoder.*, gst.* and speaker_adapter.* in the reference's key order."""
    g = dict(SPK2_GAINS, **(gains or {}))
    s: List[Spec] = []
    D, H, L = SPK2_STYLE_HIDDEN, SPK2_HIDDEN, SPK2_STYLE_LAYERS
    for i in range(L):
        _lin_u(s, f"style_encoder.spectral_layers.{i}.0.fc", D, D, gain=g["spectral"])
        _lin_u(s, f"style_encoder.spectral_layers.{i}.3.fc", D, D, gain=g["spectral"])
    for i in range(L):
        for j in (0, 1):
            n = f"style_encoder.temporal_layers.{i}.{j}.conv1.conv"
            s.append((f"{n}.weight", (2 * D, D, SPK2_STYLE_K), "uniform", 1.0 / math.sqrt(D * SPK2_STYLE_K)))
            s.append((f"{n}.bias", (2 * D,), "uniform", 1.0 / math.sqrt(D * SPK2_STYLE_K)))
    for i in range(L):
        n = f"style_encoder.attn_layers.{i}"
        _lin_u(s, f"{n}.w_qs", D, D, gain=g["mha_qk"])
        _lin_u(s, f"{n}.w_ks", D, D, gain=g["mha_qk"])
        _lin_u(s, f"{n}.w_vs", D, D)
        _lin_u(s, f"{n}.fc", D, D)
    _lin_u(s, "style_encoder.in_fc.fc", D, H, gain=g["in_fc"])
    _lin_u(s, "style_encoder.fc.fc", SPK2_DIM, D)
    dk = SPK2_DIM // SPK2_GST_HEADS
    for i in range(SPK2_GST_LAYERS):
        s.append((f"gst.embeds.{i}", (SPK2_GST_TOKENS, dk), "normal", 0.5))
    for i in range(SPK2_GST_LAYERS):
        n = f"gst.attentions.{i}"
        _lin_u(s, f"{n}.W_query", SPK2_DIM, SPK2_DIM, bias=False, gain=g["gst_qk"])
        _lin_u(s, f"{n}.W_key", SPK2_DIM, dk, bias=False, gain=g["gst_qk"])
        _lin_u(s, f"{n}.W_value", SPK2_DIM, dk, bias=False, gain=g["gst_v"])
    _lin_u(s, "speaker_adapter.style_fuser", SPK2_DIM, CAMPPLUS_EMBED, bias=False)
    return s


def speaker_embedding_specs(post_enc: bool = True, gains=None) -> List[Spec]:
    """Keys and shapes of SpeakerEmbedding (``post_enc``) / SpeakerEmbedding_wo_PostEnc (enc_q = nn.Linear(513, 512)) in the
    reference's state-dict order: enc_q.*, speaker_encoder.* (CAM++), style_encoder.*, gst.*, speaker_adapter.*."""
    s: List[Spec] = posterior_encoder_specs() if post_enc else []
    if not post_enc:
        _lin_u(s, "enc_q", SPK2_HIDDEN, SPK2_SPEC, gain=0.62)   # z at the scale the posterior encoder gives it
    s += [("speaker_encoder." + k, shape, kind, p) for k, shape, kind, p in campplus_specs()]
    return s + style_specs(gains)


def speaker_embedding_state_dict(seed: int = 1986, post_enc: bool = True, gains=None) -> Dict[str, torch.Tensor]:
    """Key-seeded, full-size (72.0 M state-dict elements, 71.9 M of them parameters) weights of the 512-d speaker encoder; the CAM++ tensors are those of
    ``campplus_state_dict(seed)`` under ``speaker_encoder.``."""
    specs = speaker_embedding_specs(post_enc, gains)
    cam = campplus_state_dict(seed)
    sd = materialize([sp for sp in specs if not sp[0].startswith("speaker_encoder.")], seed)
    return {k: (cam[k[len("speaker_encoder."):]] if k.startswith("speaker_encoder.") else sd[k]) for k, _, _, _ in specs}
