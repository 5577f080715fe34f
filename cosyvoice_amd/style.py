"""Speaker encoder v2 on MI355X: the 512-d vector of ``SpeakerEmbedding`` (cosyvoice/speaker/speaker_encoder.py:119-270,
``speaker_encoder_ckpt: speaker_encoder_v2.pt`` of the cosyvoice2 recipes; produced offline by bin/extract_speaker_vec.py:98) and of
``SpeakerEmbedding_wo_PostEnc`` (:273-418).

    timbre  = CAMPPlus(Kaldi fbank of the prompt at 16 kHz, minus its mean)            -> 192   (speaker.py)
    spec    = |stft(reflect-padded 24 kHz prompt, 1024, hop 300, hann)|, eps 1e-6       -> (T, 513), T = S // 300
    z       = PosteriorEncoder(spec): pre 1x1, 16 WaveNet layers, proj, m + noise * exp(logs)   (or Linear(513, 512) without it)
    style   = StyleEncoder_v2(z): 6 x [2 x (Linear, Mish), 2 x Conv1dGLU, self-attention + residual], fc, mean over time
    gst     = GlobalStyleTokens_v2(style): 6 attentions over 4096 tanh'd tokens each, query -> next query
    g       = gst + W timbre                                                          -> 512

Launches: the DFT, every 1x1 conv and every Linear are exact-f32 cv_gemm calls; one cv_wn_layer per WaveNet layer, one cv_glu_conv
per Conv1dGLU, cv_style_attention, cv_masked_mean, cv_gst_attention (include/cosyvoice_amd_style.h).  The keys and values of the
style-token attentions depend on weights only and are computed at load.  One captured graph per (batch, 64-frame bucket), on one
stream.

Ragged batches: every utterance is reflect-padded at its OWN ends and carries its frame count on the device; row b equals the
reference's batch-1 result for that utterance (the reference's padded batch is not: its reflect padding reads the batch's zeros and
its style convs read un-zeroed rows past the length), bit-identical to running it alone here.

The reference draws the posterior noise (posterior_encoder.py:36) at inference too, so its embedding differs from call to call;
``noise=`` fixes it, otherwise it is ``torch.randn`` on the device from ``generator``.

The reference resamples 24 -> 16 kHz for the fbank with librosa (CAMPPlus.py:304-338), which is not part of the pinned
environment; here it is ``frontend.Resample(24000, 16000)`` — parity unpinned at that boundary."""
import ctypes as C
import math

import torch

from . import _lib as L
from . import ops
from . import speaker as spk
from .frontend import Resample, _stack_waves
from .weights import (CAMPPLUS_EMBED, SPK2_DIM, SPK2_GST_HEADS, SPK2_GST_LAYERS, SPK2_GST_TOKENS, SPK2_HIDDEN, SPK2_SPEC,
                      SPK2_STYLE_HEADS, SPK2_STYLE_HIDDEN, SPK2_STYLE_K, SPK2_STYLE_LAYERS, SPK2_WN_K, SPK2_WN_LAYERS,
                      fold_weight_norm, speaker_embedding_specs)

SAMPLE_RATE, NFFT, HOP = 24000, 1024, 300
PAD = (NFFT - HOP) // 2                     # 362
NBINS = NFFT // 2 + 1                       # 513
LD_SPEC = (2 * NBINS + 3) // 4 * 4          # [re | im | pad]
LD_MAG = (NBINS + 3) // 4 * 4               # 516
FRAME_BUCKET = 64
MAX_FRAMES = 2400                           # cv_style_attention keeps a 16 x T score block in LDS


def num_frames(S: int) -> int:
    """Frames of an S-sample prompt: (S + 2 * 362 - 1024) // 300 + 1 = S // 300."""
    return int(S) // HOP


def _stage_reflect(buf, S, ld):
    """buf (B, S_max) with S[b] valid samples per row -> (B, ld): row b = its own samples reflect-padded by 362 at both of ITS ends,
    zeros behind.  What ``buf`` holds past a row's length is never read."""
    dev = buf.device
    lens = torch.tensor(S, dtype=torch.int64).to(dev).unsqueeze(1)
    i = torch.arange(ld, device=dev).unsqueeze(0)
    j = (i - PAD).abs()
    j = torch.where(j >= lens, 2 * (lens - 1) - j, j)
    stage = torch.gather(buf, 1, j.clamp_(0, buf.shape[1] - 1))
    return torch.where(i < lens + 2 * PAD, stage, torch.zeros((), device=dev)).contiguous()


def _dft_basis(device):
    n = torch.arange(NFFT, dtype=torch.float64)
    k = torch.arange(NBINS, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.outer(k, n) / NFFT
    win = torch.hann_window(NFFT, periodic=True, dtype=torch.float64)
    basis = torch.zeros(LD_SPEC, NFFT, dtype=torch.float64)
    basis[:NBINS] = torch.cos(ang) * win
    basis[NBINS:2 * NBINS] = -torch.sin(ang) * win
    return basis.to(device, torch.float32).contiguous()


def _enqueue_spectrogram(dft, stage, ld_stage, B, T, spec, mag):
    """stage (B, ld_stage) -> mag (B * T, LD_MAG): frame t of row b = stage[b, 300 t : 300 t + 1024] (lda = hop)."""
    ops.gemm(stage, dft, T, LD_SPEC, NFFT, batch=B, a_bs=(ld_stage, 0), lda=HOP, a_rows=T, out_f32=spec, o32_bs=(T * LD_SPEC, 0),
             ldo32=LD_SPEC, dtype=L.CV_F32)
    L.check(L.lib().cv_stft_magnitude(spec.data_ptr(), LD_SPEC, mag.data_ptr(), LD_MAG, B * T, NBINS, 1e-6, L.stream_ptr()),
            "cv_stft_magnitude")


def _check_waves(S):
    if min(S) <= PAD:
        raise ValueError(f"a waveform of {min(S)} samples cannot be reflect-padded by {PAD}")


class LinearSpectrogram:
    """spectrogram_torch(y, 1024, 24000, 300, 1024) (speaker/mel_processing.py:40-68), ragged: a (S,) / (B, S) tensor, a list of 1-D
    waveforms or ``(buf (B, S_max), lens)`` -> (spec (B, T_max, 513) fp32 channels-last, frames list[int]); row b reflects at its own
    end, frames at or past S_b // 300 are 0."""

    def __init__(self, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("cosyvoice_amd needs an MI355X (no CPU fallback)")
        self.device = torch.device(device)
        self.dft = _dft_basis(self.device)

    @torch.no_grad()
    def __call__(self, waves):
        buf, S = _stack_waves(waves, self.device)
        _check_waves(S)
        frames = [num_frames(s) for s in S]
        B, T = len(S), max(max(frames), 1)
        ld = ((T - 1) * HOP + NFFT + 3) // 4 * 4
        stage = _stage_reflect(buf, S, ld)
        spec = torch.empty(B * T, LD_SPEC, device=self.device)
        mag = torch.empty(B * T, LD_MAG, device=self.device)
        _enqueue_spectrogram(self.dft, stage, ld, B, T, spec, mag)
        out = mag.view(B, T, LD_MAG)[:, :, :NBINS]
        nf = torch.tensor(frames, dtype=torch.int64).to(self.device).view(B, 1, 1)
        return out.masked_fill(torch.arange(T, device=self.device).view(1, T, 1) >= nf, 0.0), frames


def _f32(t, dev):
    return t.to(dev, torch.float32).contiguous()


class PosteriorEncoder:
    """PosteriorEncoder(513, 512, 512, 5, 1, 16, gin_channels=0) (speaker/posterior_encoder.py:6-37) over channels-last rows.
    ``fused``: one cv_wn_layer per WaveNet layer; otherwise the layer as cv_gemm launches (conv, then the 1x1 from a gate product
    that goes through HBM) — kept for the comparison of tools/style_bench.py, not bit-identical to the fused form."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.p = None

    def load_state_dict(self, sd, prefix="enc_q."):
        dev, H = self.device, SPK2_HIDDEN
        pre = torch.zeros(H, LD_MAG, dtype=torch.float32)
        pre[:, :SPK2_SPEC] = sd[prefix + "pre.weight"][:, :, 0]
        P = dict(pre_w=_f32(pre, dev), pre_b=_f32(sd[prefix + "pre.bias"], dev), layers=[],
                 proj_w=_f32(sd[prefix + "proj.weight"][:, :, 0], dev), proj_b=_f32(sd[prefix + "proj.bias"], dev))
        for i in range(SPK2_WN_LAYERS):
            w_in = fold_weight_norm(sd, f"{prefix}enc.in_layers.{i}").double()          # (1024, 512, 5): weight norm folded at load
            w_rs = fold_weight_norm(sd, f"{prefix}enc.res_skip_layers.{i}").double()    # (1024 | 512, 512, 1)
            P["layers"].append(dict(w_in=_f32(w_in.permute(0, 2, 1).reshape(2 * H, SPK2_WN_K * H), dev),      # k = tap * 512 + ci
                                    b_in=_f32(sd[f"{prefix}enc.in_layers.{i}.bias"], dev), w_rs=_f32(w_rs[:, :, 0], dev),
                                    b_rs=_f32(sd[f"{prefix}enc.res_skip_layers.{i}.bias"], dev)))
        self.p = P
        return self

    def workspace(self, B, T):
        e = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
        return dict(x0=e(B * T, SPK2_HIDDEN), x1=e(B * T, SPK2_HIDDEN), skip=e(B * T, SPK2_HIDDEN), stats=e(B * T, 2 * SPK2_HIDDEN))

    def enqueue(self, mag, lens, B, T, ws, fused=True, extra=None):
        """mag (B * T, LD_MAG) -> ws['stats'] (B * T, 1024) = [m | logs]; rows at or past a length hold proj's bias (never read)."""
        P, H = self.p, SPK2_HIDDEN
        ops.gemm(mag, P["pre_w"], B * T, H, LD_MAG, lda=LD_MAG, bias=P["pre_b"], out_f32=ws["x0"], ldo32=H, dtype=L.CV_F32)
        x, y = ws["x0"], ws["x1"]
        for i, lay in enumerate(P["layers"]):
            if fused:
                wn_layer(x, y, ws["skip"], lens, B, T, lay, first=i == 0)
            else:
                _wn_layer_composed(x, y, ws["skip"], lens, B, T, lay, extra, first=i == 0)
            if i < SPK2_WN_LAYERS - 1:
                x, y = y, x
        ops.gemm(ws["skip"], P["proj_w"], B * T, 2 * H, H, lda=H, bias=P["proj_b"], out_f32=ws["stats"], ldo32=2 * H, dtype=L.CV_F32)


def wn_layer(x, x_out, skip, lens, B, T, lay, first):
    """One cv_wn_layer launch: x, x_out, skip (B * T, 512) contiguous; ``lay`` = dict(w_in, b_in, w_rs, b_rs)."""
    H = SPK2_HIDDEN
    p = L.WnLayerParams()
    p.B, p.T, p.C, p.taps = B, T, H, SPK2_WN_K
    p.len = lens.data_ptr()
    p.x, p.x_bs, p.ldx = x.data_ptr(), T * H, H
    p.w_in, p.b_in, p.w_rs, p.b_rs = (lay[k].data_ptr() for k in ("w_in", "b_in", "w_rs", "b_rs"))
    p.n_rs, p.skip_init = lay["w_rs"].shape[0], int(first)
    if p.n_rs == 2 * H:
        p.x_out, p.xo_bs, p.ldxo = x_out.data_ptr(), T * H, H
    p.skip, p.skip_bs, p.ldskip = skip.data_ptr(), T * H, H
    L.check(L.style_lib().cv_wn_layer(C.byref(p), L.stream_ptr()), "cv_wn_layer")


def _wn_layer_composed(x, x_out, skip, lens, B, T, lay, extra, first):
    """The same layer without the row-block kernel: the k5 conv as a ragged cv_gemm, cv_wn_gate, the 1x1 as two cv_gemm launches
    with the residual / skip sums in their epilogues; ``extra`` = dict(a (B * T, 1024), g (B * T, 512)).  Rows past a length are
    not zeroed (they are never read)."""
    H = SPK2_HIDDEN
    a = extra["a"]
    ops.gemm(x, lay["w_in"], T, 2 * H, SPK2_WN_K * H, batch=B, batch_inner=B, a_bs=(T * H, 0), lda=H, a_rows=T, cin=H, tap_base=-2, tap_step=1,
             bias=lay["b_in"], out_f32=a, o32_bs=(T * 2 * H, 0), ldo32=2 * H, lens=lens, a_len=(1, 0), dtype=L.CV_F32)
    g = extra["g"]
    L.check(L.style_lib().cv_wn_gate(a.data_ptr(), 2 * H, g.data_ptr(), H, B * T, H, L.stream_ptr()), "cv_wn_gate")
    n_rs = lay["w_rs"].shape[0]
    if n_rs == 2 * H:
        ops.gemm(g, lay["w_rs"], B * T, H, H, lda=H, bias=lay["b_rs"], res=x, ldres=H, out_f32=x_out, ldo32=H, dtype=L.CV_F32)
        w2, b2 = lay["w_rs"][H:], lay["b_rs"][H:]
    else:
        w2, b2 = lay["w_rs"], lay["b_rs"]
    ops.gemm(g, w2, B * T, H, H, lda=H, bias=b2, res=None if first else skip, ldres=0 if first else H, out_f32=skip, ldo32=H,
             dtype=L.CV_F32)


def glu_conv(x, y, lens, B, T, w, bias):
    D = SPK2_STYLE_HIDDEN
    p = L.GluConvParams()
    p.B, p.T, p.C, p.taps = B, T, D, SPK2_STYLE_K
    p.len = lens.data_ptr()
    p.x, p.x_bs, p.ldx = x.data_ptr(), T * D, D
    p.w, p.bias = w.data_ptr(), bias.data_ptr()
    p.y, p.y_bs, p.ldy = y.data_ptr(), T * D, D
    L.check(L.style_lib().cv_glu_conv(C.byref(p), L.stream_ptr()), "cv_glu_conv")


def style_attention(qkv, out, lens, B, T, scale):
    """qkv (B * T, 768) = [q | k | v] rows, 4 heads x 64 each -> out (B * T, 256)."""
    D = SPK2_STYLE_HIDDEN
    q = qkv.data_ptr()
    L.check(L.style_lib().cv_style_attention(q, q + 4 * D, q + 8 * D, T * 3 * D, 3 * D, out.data_ptr(), T * D, D, lens.data_ptr(), B, T,
                                             SPK2_STYLE_HEADS, scale, L.stream_ptr()), "cv_style_attention")


def masked_mean(x, lens, B, T, Cc, out):
    L.check(L.style_lib().cv_masked_mean(x.data_ptr(), T * x.stride(0), x.stride(0), lens.data_ptr(), B, T, Cc, out.data_ptr(),
                                         out.stride(0), L.stream_ptr()), "cv_masked_mean")


def posterior_sample(stats, noise, z, lens, B, T):
    L.check(L.style_lib().cv_posterior_sample(stats.data_ptr(), stats.stride(0), noise.data_ptr(), z.data_ptr(), z.stride(0),
                                              lens.data_ptr(), B, T, SPK2_HIDDEN, L.stream_ptr()), "cv_posterior_sample")


def gst_attention(q, k, v, out, B, scale):
    L.check(L.style_lib().cv_gst_attention(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), out.data_ptr(), out.stride(0), B,
                                           k.shape[0], k.shape[1], scale, L.stream_ptr()), "cv_gst_attention")


class StyleEncoder:
    """StyleEncoder_v2(512, 256, 512, 5, 4, num_layers=6) (speaker/style_encoder.py:21-114): z (B * T, 512) rows -> (B, 512)."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.p = None

    def load_state_dict(self, sd, prefix="style_encoder."):
        dev, D = self.device, SPK2_STYLE_HIDDEN
        w = lambda k: _f32(sd[prefix + k], dev)  # noqa: E731
        P = dict(in_w=w("in_fc.fc.weight"), in_b=w("in_fc.fc.bias"), fc_w=w("fc.fc.weight"), fc_b=w("fc.fc.bias"), layers=[])
        for i in range(SPK2_STYLE_LAYERS):
            a = f"attn_layers.{i}."
            lay = dict(s0_w=w(f"spectral_layers.{i}.0.fc.weight"), s0_b=w(f"spectral_layers.{i}.0.fc.bias"),
                       s1_w=w(f"spectral_layers.{i}.3.fc.weight"), s1_b=w(f"spectral_layers.{i}.3.fc.bias"),
                       qkv_w=_f32(torch.cat([sd[prefix + a + n + ".weight"] for n in ("w_qs", "w_ks", "w_vs")]), dev),
                       qkv_b=_f32(torch.cat([sd[prefix + a + n + ".bias"] for n in ("w_qs", "w_ks", "w_vs")]), dev),
                       o_w=w(a + "fc.weight"), o_b=w(a + "fc.bias"), glu=[])
            for j in (0, 1):
                cw = sd[f"{prefix}temporal_layers.{i}.{j}.conv1.conv.weight"]                      # (512, 256, 5)
                lay["glu"].append((_f32(cw.permute(0, 2, 1).reshape(2 * D, SPK2_STYLE_K * D), dev),
                                   w(f"temporal_layers.{i}.{j}.conv1.conv.bias")))
            P["layers"].append(lay)
        self.p = P
        return self

    def workspace(self, B, T):
        e = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
        D = SPK2_STYLE_HIDDEN
        return dict(h0=e(B * T, D), h1=e(B * T, D), qkv=e(B * T, 3 * D), ao=e(B * T, D), fc=e(B * T, SPK2_DIM), style=e(B, SPK2_DIM))

    def enqueue(self, z, lens, B, T, ws):
        P, D, M = self.p, SPK2_STYLE_HIDDEN, B * T
        lin = lambda a, w, b, o, **kw: ops.gemm(a, w, M, w.shape[0], w.shape[1], lda=a.stride(0), bias=b, out_f32=o,  # noqa: E731
                                                ldo32=o.stride(0), dtype=L.CV_F32, **kw)
        # cv_gemm's out_f32 is the value BEFORE the activation; the activated one is out_act (fp32 here: the launch's dtype)
        mish = lambda a, w, b, o: ops.gemm(a, w, M, w.shape[0], w.shape[1], lda=a.stride(0), bias=b, act=ops.ACT_MISH, out_act=o,  # noqa: E731
                                           ldoa=o.stride(0), dtype=L.CV_F32)
        h0, h1 = ws["h0"], ws["h1"]
        lin(z, P["in_w"], P["in_b"], h0)
        for lay in P["layers"]:
            mish(h0, lay["s0_w"], lay["s0_b"], h1)
            mish(h1, lay["s1_w"], lay["s1_b"], h0)
            glu_conv(h0, h1, lens, B, T, *lay["glu"][0])
            glu_conv(h1, h0, lens, B, T, *lay["glu"][1])          # rows past a length are 0 from here: the reference's masked_fill
            lin(h0, lay["qkv_w"], lay["qkv_b"], ws["qkv"])
            style_attention(ws["qkv"], ws["ao"], lens, B, T, 1.0 / math.sqrt(D))           # temperature sqrt(d_model), modules.py:566
            lin(ws["ao"], lay["o_w"], lay["o_b"], h1, res=h0, ldres=D)
            h0, h1 = h1, h0
        lin(h0, P["fc_w"], P["fc_b"], ws["fc"])
        masked_mean(ws["fc"], lens, B, T, SPK2_DIM, ws["style"])


class GlobalStyleTokens:
    """GlobalStyleTokens_v2(4096, 512, 8, num_layers=6) (speaker/style_encoder.py:117-157): (B, 512) -> (B, 512).  Per layer the
    keys tanh(E) W_key^T and values tanh(E) W_value^T (fp64 at load, stored fp32 head-major) are fixed; a call is W_query (cv_gemm)
    and cv_gst_attention per layer."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.p = None

    def load_state_dict(self, sd, prefix="gst."):
        dev, Hh = self.device, SPK2_GST_HEADS
        layers = []
        for i in range(SPK2_GST_LAYERS):
            e = torch.tanh(sd[f"{prefix}embeds.{i}"].float()).double()
            if tuple(e.shape) != (SPK2_GST_TOKENS, SPK2_DIM // Hh):
                raise ValueError(f"{prefix}embeds.{i}: expected ({SPK2_GST_TOKENS}, {SPK2_DIM // Hh}), got {tuple(e.shape)}")
            hm = lambda wk: _f32((e @ sd[f"{prefix}attentions.{i}.{wk}.weight"].double().t())  # noqa: E731
                                 .view(SPK2_GST_TOKENS, Hh, -1).permute(1, 0, 2), dev)
            layers.append(dict(q_w=_f32(sd[f"{prefix}attentions.{i}.W_query.weight"], dev), k=hm("W_key"), v=hm("W_value")))
        self.p = layers
        return self

    def workspace(self, B):
        e = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
        return dict(q=e(B, SPK2_DIM), a=e(B, SPK2_DIM), b=e(B, SPK2_DIM))

    def enqueue(self, x, B, ws):
        """x (B, 512) -> the tensor of ``ws`` that holds the result."""
        outs = (ws["a"], ws["b"])
        for i, lay in enumerate(self.p):
            ops.gemm(x, lay["q_w"], B, SPK2_DIM, SPK2_DIM, lda=x.stride(0), out_f32=ws["q"], ldo32=SPK2_DIM, dtype=L.CV_F32)
            x = outs[i & 1]
            gst_attention(ws["q"], lay["k"], lay["v"], x, B, 1.0 / math.sqrt(SPK2_DIM // SPK2_GST_HEADS))
        return x


class SpeakerEmbedding:
    """``SpeakerEmbedding()`` of the reference with its state-dict keys.  ``model(waves, wave_lengths=None, noise=None,
    generator=None, graph=True)`` -> (B, 512) fp32 on the device.  ``waves``: (B, 1, S) / (B, S) at 24 kHz with ``wave_lengths``
    samples per row, or a list of 1-D waveforms.  ``noise``: (B, 512, T) or a list of (512, T_b) (channels first, as the reference
    draws it); default ``torch.randn`` on the device from ``generator`` — the reference's embedding is random per call as well.
    ``timbre=`` replaces the CAM++ branch by given (B, 192) vectors (tests).  ``stages`` of the last call: m, logs (B, T, 512),
    style_vec, gst_out, g."""

    POST_ENC = True

    def __init__(self, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("cosyvoice_amd needs an MI355X (no CPU fallback)")
        self.device = torch.device(device)
        self.dft = _dft_basis(self.device)
        self.campplus = spk.CAMPPlus(device=device)
        self.to_16k = Resample(SAMPLE_RATE, spk.SAMPLE_RATE, device=device)
        self.enc_q = PosteriorEncoder(device) if self.POST_ENC else None
        self.style_encoder, self.gst = StyleEncoder(device), GlobalStyleTokens(device)
        self.p = None
        self._ws, self._graphs = {}, {}
        self.stages = {}

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict=None):
        """The reference's keys: enc_q.* (weight_g / weight_v, or plain weight when the norm was removed), speaker_encoder.*,
        style_encoder.*, gst.embeds.N, gst.attentions.N.*, speaker_adapter.style_fuser.weight.  Strict for SpeakerEmbedding; the
        class without the posterior encoder ignores unexpected keys (speaker_encoder.py:369 loads with strict=False)."""
        strict = self.POST_ENC if strict is None else strict
        ops.drop_graphs(self._graphs)
        self._ws.clear()
        want = [k for k, _, _, _ in speaker_embedding_specs(self.POST_ENC)]
        have = set(sd)
        alt = {k: k[:-2] for k in want if k.endswith(".weight_g") or k.endswith(".weight_v")}      # norm already removed
        missing = [k for k in want if k not in have and not (k in alt and alt[k] in have)]
        if missing:
            raise KeyError(f"missing keys: {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        if strict:
            extra = sorted(have - set(want) - set(alt.values()))
            if extra:
                raise KeyError(f"unexpected keys: {extra[:5]}{' ...' if len(extra) > 5 else ''}")
        dev = self.device
        self.campplus.load_state_dict({k[len("speaker_encoder."):]: v for k, v in sd.items() if k.startswith("speaker_encoder.")})
        if self.POST_ENC:
            self.enc_q.load_state_dict(sd)
            self.p = {}
        else:
            w = torch.zeros(SPK2_HIDDEN, LD_MAG)
            w[:, :SPK2_SPEC] = sd["enc_q.weight"]
            self.p = dict(lin_w=_f32(w, dev), lin_b=_f32(sd["enc_q.bias"], dev))
        self.style_encoder.load_state_dict(sd)
        self.gst.load_state_dict(sd)
        self.p["fuse_w"] = _f32(sd["speaker_adapter.style_fuser.weight"], dev)
        return self

    # ------------------------------------------------------------------ launches
    def _workspace(self, B, T):
        e = lambda *s: torch.empty(*s, device=self.device)  # noqa: E731
        ld = ((T - 1) * HOP + NFFT + 3) // 4 * 4
        ws = dict(B=B, T=T, ld=ld, lens=torch.zeros(B, dtype=torch.int32, device=self.device), stage=e(B, ld), spec=e(B * T, LD_SPEC),
                  mag=e(B * T, LD_MAG), z=e(B * T, SPK2_HIDDEN), noise=e(B * T, SPK2_HIDDEN), timbre=e(B, CAMPPLUS_EMBED), g=e(B, SPK2_DIM))
        if self.POST_ENC:
            ws.update(self.enc_q.workspace(B, T))
        ws.update(self.style_encoder.workspace(B, T))
        ws["gst"] = self.gst.workspace(B)
        return ws

    def _enqueue(self, ws):
        B, T, lens = ws["B"], ws["T"], ws["lens"]
        _enqueue_spectrogram(self.dft, ws["stage"], ws["ld"], B, T, ws["spec"], ws["mag"])
        if self.POST_ENC:
            self.enc_q.enqueue(ws["mag"], lens, B, T, ws)
            posterior_sample(ws["stats"], ws["noise"], ws["z"], lens, B, T)
        else:
            ops.gemm(ws["mag"], self.p["lin_w"], B * T, SPK2_HIDDEN, LD_MAG, lda=LD_MAG, bias=self.p["lin_b"], out_f32=ws["z"],
                     ldo32=SPK2_HIDDEN, dtype=L.CV_F32)
        self.style_encoder.enqueue(ws["z"], lens, B, T, ws)
        ws["gst_out"] = self.gst.enqueue(ws["style"], B, ws["gst"])
        ops.gemm(ws["timbre"], self.p["fuse_w"], B, SPK2_DIM, CAMPPLUS_EMBED, lda=CAMPPLUS_EMBED, res=ws["gst_out"], ldres=SPK2_DIM,
                 out_f32=ws["g"], ldo32=SPK2_DIM, dtype=L.CV_F32)

    @staticmethod
    def bucket(frames: int) -> int:
        return (max(frames, 1) + FRAME_BUCKET - 1) // FRAME_BUCKET * FRAME_BUCKET

    @torch.no_grad()
    def __call__(self, waves, wave_lengths=None, noise=None, generator=None, graph=True, timbre=None):
        if self.p is None:
            raise RuntimeError("load_state_dict first")
        dev = self.device
        if isinstance(waves, torch.Tensor):
            if waves.dim() == 3:
                if waves.shape[1] != 1:
                    raise ValueError(f"expected (B, 1, S), got {tuple(waves.shape)}")
                waves = waves[:, 0]
            if wave_lengths is not None:
                waves = (waves if waves.dim() == 2 else waves.unsqueeze(0), [int(v) for v in wave_lengths])
        elif wave_lengths is not None:
            raise ValueError("wave_lengths goes with a padded tensor; a list of waveforms carries its own lengths")
        buf, S = _stack_waves(waves, dev)
        _check_waves(S)
        if timbre is None and min(S) * 2 // 3 < spk.WIN + 2 * spk.HOP:
            raise ValueError(f"a waveform of {min(S)} samples gives fewer than the 3 fbank frames CAM++ needs")
        frames = [num_frames(s) for s in S]
        if max(frames) > MAX_FRAMES:
            raise ValueError(f"{max(frames)} frames: prompts longer than {MAX_FRAMES // 80} s are not supported")
        B, T = len(S), self.bucket(max(frames))
        key = (B, T)
        ops.bound_cache(self._ws, key, self._graphs)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = self._workspace(B, T)
        ws["stage"].copy_(_stage_reflect(buf, S, ws["ld"]))
        ws["lens"].copy_(torch.tensor(frames, dtype=torch.int32))
        if self.POST_ENC:
            nz = ws["noise"].view(B, T, SPK2_HIDDEN)
            if noise is None:
                nz.copy_(torch.randn(B, T, SPK2_HIDDEN, device=dev, generator=generator))
            else:
                rows = list(noise) if not isinstance(noise, torch.Tensor) else [noise[b] for b in range(noise.shape[0])]
                if len(rows) != B:
                    raise ValueError("one noise tensor per utterance")
                nz.zero_()
                for b, r in enumerate(rows):
                    if r.shape[0] != SPK2_HIDDEN or r.shape[1] < frames[b]:
                        raise ValueError(f"noise row {b}: expected (512, >= {frames[b]}), got {tuple(r.shape)}")
                    nz[b, :frames[b]].copy_(r[:, :frames[b]].t())
        if timbre is None:
            w16, l16 = self.to_16k([buf[b, :S[b]] for b in range(B)])
            timbre = self.campplus.extract_spk_embedding([w16[b, :l16[b]] for b in range(B)], graph=graph)
        ws["timbre"].copy_(torch.as_tensor(timbre).to(dev, torch.float32).reshape(B, CAMPPLUS_EMBED))
        if graph:
            g = self._graphs.get(key)
            if g is None:
                g = self._graphs[key] = ops.Graph().capture(lambda: self._enqueue(ws))
            g.launch()
        else:
            self._enqueue(ws)
        self.stages = dict(style_vec=ws["style"], gst_out=ws["gst_out"], g=ws["g"], frames=frames)
        if self.POST_ENC:
            st = ws["stats"].view(B, T, 2 * SPK2_HIDDEN)
            self.stages.update(m=st[:, :, :SPK2_HIDDEN], logs=st[:, :, SPK2_HIDDEN:], z=ws["z"].view(B, T, SPK2_HIDDEN))
        return ws["g"].clone()

    def num_launches(self, key):
        """Kernel launches in the captured graph of ``key`` = (B, frame bucket), or None when it has not been captured."""
        g = self._graphs.get(key)
        return None if g is None else g.num_launches


class SpeakerEmbeddingWoPostEnc(SpeakerEmbedding):
    """``SpeakerEmbedding_wo_PostEnc`` (speaker_encoder.py:273-418, cosyvoice_pho_llm_spk_ft3.yaml): ``enc_q`` is nn.Linear(513, 512)
    on the spectrogram, there is no noise, and the checkpoint loads non-strictly."""

    POST_ENC = False
