"""CPU restatement of the 512-d speaker encoder (cosyvoice/speaker/speaker_encoder.py:223-270), stage by stage over the
reference's state-dict keys and independent of cosyvoice_amd.style:

* ``linear_spectrogram`` — spectrogram_torch (mel_processing.py:40-68): reflect pad 362, stft(1024, hop 300, hann, center=False),
  sqrt(re^2 + im^2 + 1e-6);
* ``posterior_encoder`` — PosteriorEncoder(513, 512, 512, 5, 1, 16) (posterior_encoder.py:29-37; WN modules.py:190-219);
* ``style_encoder`` — StyleEncoder_v2(512, 256, 512, 5, 4, num_layers=6) (style_encoder.py:83-114; modules.py:498-630);
* ``gst`` — GlobalStyleTokens_v2(4096, 512, 8, 6) (style_encoder.py:148-157; modules.py:689-710);
* ``fuse`` — StyleFuser "Add" (style_encoder.py:182-184).

One utterance at a time (the contract of the device path: a batch row equals the reference's batch-1 result).  ``dtype`` float32
or float64; ``products="bf16x3"`` computes every matrix product as three bf16 x bf16 products of hi / lo splits with fp32
accumulation (what a CV_F32X3 kernel would do).  ``fault`` injects one deliberate error (tests/test_style_cpu.py shows that each is
seen at the tolerance of its stage): "mask+1" (the length mask one frame too wide), "tap" (the last conv tap dropped), "gate_swap"
(tanh and sigmoid halves exchanged), "mha_scale" (1/8 instead of 1/16), "gst_tokens" (4095 tokens).
"""
import math

import torch
import torch.nn.functional as F

HOP, NFFT, PAD = 300, 1024, 362
HIDDEN, WN_LAYERS, STYLE_HIDDEN, STYLE_HEADS, STYLE_LAYERS, GST_LAYERS, GST_HEADS = 512, 16, 256, 4, 6, 6, 8
FAULTS = ("mask+1", "tap", "gate_swap", "mha_scale", "gst_tokens")


def _bf16_split(a):
    hi = a.to(torch.bfloat16).to(torch.float32)
    return hi, (a - hi).to(torch.bfloat16).to(torch.float32)


class Ctx:
    def __init__(self, sd, dtype=torch.float32, products="exact", fault=None):
        assert products in ("exact", "bf16x3") and (fault is None or fault in FAULTS)
        self.sd, self.dtype, self.products, self.fault = sd, dtype, products, fault

    def w(self, key):
        return self.sd[key].to(self.dtype)

    def wn(self, name):
        """weight-normed conv weight: g * v / ||v|| per output channel, or the plain weight of a checkpoint with the norm removed."""
        if name + ".weight" in self.sd:
            return self.w(name + ".weight")
        v, g = self.w(name + ".weight_v"), self.w(name + ".weight_g")
        return v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape))

    def mm(self, a, b):
        """a (M, K) @ b (K, N)."""
        if self.products == "exact":
            return a @ b
        ah, al = _bf16_split(a.float())
        bh, bl = _bf16_split(b.float())
        return (ah @ bh + (ah @ bl + al @ bh)).to(self.dtype)

    def linear(self, x, w, b=None):
        y = self.mm(x, w.t())
        return y if b is None else y + b

    def conv(self, x, w, b, pad):
        """x (T, Cin) channels-last, w (Cout, Cin, k) -> (T, Cout); zero padding ``pad`` on both sides."""
        k = w.shape[2]
        if self.fault == "tap" and k > 1:
            w = w.clone()
            w[:, :, k - 1] = 0
        if self.products == "exact":
            return F.conv1d(x.t().unsqueeze(0), w, b, padding=pad)[0].t()
        xp = F.pad(x, (0, 0, pad, pad))
        cols = torch.cat([xp[j:j + x.shape[0]] for j in range(k)], dim=1)            # k = tap * Cin + ci
        return self.mm(cols, w.permute(0, 2, 1).reshape(w.shape[0], -1).t()) + b


def num_frames(S):
    return S // HOP


def linear_spectrogram(wave, dtype=torch.float32):
    """1-D waveform at 24 kHz -> (S // 300, 513)."""
    y = torch.as_tensor(wave).reshape(1, 1, -1).to(dtype)
    y = F.pad(y, (PAD, PAD), mode="reflect")[0]
    spec = torch.stft(y, NFFT, hop_length=HOP, win_length=NFFT, window=torch.hann_window(NFFT, dtype=dtype), center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    spec = torch.view_as_real(spec)
    return torch.sqrt(spec.pow(2).sum(-1) + 1e-6)[0].t().contiguous()


def linear_spectrogram_dft(wave, dtype=torch.float32):
    """The same spectrogram as a matrix product: frames of the reflect-padded signal times a hann-windowed [cos | -sin] basis that
    is built in fp64 and rounded to ``dtype`` — the arithmetic of a DFT done as a GEMM, whose fp32 error is that of 1024-term
    sums, not of an FFT."""
    y = F.pad(torch.as_tensor(wave).reshape(1, 1, -1).to(dtype), (PAD, PAD), mode="reflect")[0, 0]
    frames = y.unfold(0, NFFT, HOP)
    n = torch.arange(NFFT, dtype=torch.float64)
    k = torch.arange(NFFT // 2 + 1, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.outer(k, n) / NFFT
    win = torch.hann_window(NFFT, periodic=True, dtype=torch.float64)
    re = frames @ (torch.cos(ang) * win).to(dtype).t()
    im = frames @ (-torch.sin(ang) * win).to(dtype).t()
    return torch.sqrt(re * re + im * im + 1e-6)


def posterior_encoder(c: Ctx, spec, noise=None, prefix="enc_q."):
    """spec (T, 513); noise (T, 512) or None (z = m) -> dict(m, logs, z), each (T, 512)."""
    x = c.conv(spec, c.w(prefix + "pre.weight"), c.w(prefix + "pre.bias"), 0)
    out = torch.zeros_like(x)
    H = HIDDEN
    for i in range(WN_LAYERS):
        a = c.conv(x, c.wn(f"{prefix}enc.in_layers.{i}"), c.w(f"{prefix}enc.in_layers.{i}.bias"), 2)
        t, s = (a[:, H:], a[:, :H]) if c.fault == "gate_swap" else (a[:, :H], a[:, H:])
        acts = torch.tanh(t) * torch.sigmoid(s)
        rs = c.conv(acts, c.wn(f"{prefix}enc.res_skip_layers.{i}"), c.w(f"{prefix}enc.res_skip_layers.{i}.bias"), 0)
        if i < WN_LAYERS - 1:
            x = x + rs[:, :H]
            out = out + rs[:, H:]
        else:
            out = out + rs
    stats = c.conv(out, c.w(prefix + "proj.weight"), c.w(prefix + "proj.bias"), 0)
    m, logs = stats[:, :H], stats[:, H:]
    z = m if noise is None else m + noise.to(c.dtype) * torch.exp(logs)
    return {"m": m, "logs": logs, "z": z}


def _mish(x):
    return x * torch.tanh(F.softplus(x))


def _entropy(p):
    return float(-(p * torch.log(p.clamp_min(1e-300 if p.dtype == torch.float64 else 1e-38))).sum(-1).mean())


def style_encoder(c: Ctx, z, entropies=None, p="style_encoder."):
    """z (T, 512) -> style vector (512,).  ``entropies``: a list that receives the mean attention entropy of every layer."""
    D, Hh = STYLE_HIDDEN, STYLE_HEADS
    x = c.linear(z, c.w(p + "in_fc.fc.weight"), c.w(p + "in_fc.fc.bias"))
    T = x.shape[0]
    for i in range(STYLE_LAYERS):
        x = _mish(c.linear(x, c.w(f"{p}spectral_layers.{i}.0.fc.weight"), c.w(f"{p}spectral_layers.{i}.0.fc.bias")))
        x = _mish(c.linear(x, c.w(f"{p}spectral_layers.{i}.3.fc.weight"), c.w(f"{p}spectral_layers.{i}.3.fc.bias")))
        for j in (0, 1):
            n = f"{p}temporal_layers.{i}.{j}.conv1.conv"
            a = c.conv(x, c.w(n + ".weight"), c.w(n + ".bias"), 2)
            x = x + a[:, :D] * torch.sigmoid(a[:, D:])
        n = f"{p}attn_layers.{i}"
        q = c.linear(x, c.w(n + ".w_qs.weight"), c.w(n + ".w_qs.bias")).view(T, Hh, D // Hh).transpose(0, 1)
        k = c.linear(x, c.w(n + ".w_ks.weight"), c.w(n + ".w_ks.bias")).view(T, Hh, D // Hh).transpose(0, 1)
        v = c.linear(x, c.w(n + ".w_vs.weight"), c.w(n + ".w_vs.bias")).view(T, Hh, D // Hh).transpose(0, 1)
        temp = 8.0 if c.fault == "mha_scale" else math.sqrt(D)
        s = torch.stack([c.mm(q[h], k[h].t()) for h in range(Hh)]) / temp
        pa = torch.softmax(s, dim=-1)
        if entropies is not None:
            entropies.append(_entropy(pa))
        o = torch.stack([c.mm(pa[h], v[h]) for h in range(Hh)]).transpose(0, 1).reshape(T, D)
        x = c.linear(o, c.w(n + ".fc.weight"), c.w(n + ".fc.bias")) + x
    x = c.linear(x, c.w(p + "fc.fc.weight"), c.w(p + "fc.fc.bias"))
    return x.sum(dim=0) / T


def gst(c: Ctx, style_vec, entropies=None, p="gst."):
    """style vector (512,) -> (512,)."""
    q = style_vec.reshape(1, -1)
    Hh = GST_HEADS
    for i in range(GST_LAYERS):
        e = torch.tanh(c.w(f"{p}embeds.{i}"))
        if c.fault == "gst_tokens":
            e = e[:-1]
        qs = c.linear(q, c.w(f"{p}attentions.{i}.W_query.weight"))
        ks = c.linear(e, c.w(f"{p}attentions.{i}.W_key.weight"))
        vs = c.linear(e, c.w(f"{p}attentions.{i}.W_value.weight"))
        dk = e.shape[1]
        outs = []
        ent = []
        for h in range(Hh):
            sl = slice(h * dk, (h + 1) * dk)
            pa = torch.softmax(c.mm(qs[:, sl], ks[:, sl].t()) / math.sqrt(dk), dim=-1)
            ent.append(_entropy(pa))
            outs.append(c.mm(pa, vs[:, sl]))
        if entropies is not None:
            entropies.append(sum(ent) / Hh)
        q = torch.cat(outs, dim=1)
    return q[0]


def fuse(c: Ctx, gst_out, timbre):
    return gst_out + c.linear(timbre.to(c.dtype).reshape(1, -1), c.w("speaker_adapter.style_fuser.weight"))[0]


def speaker_embedding(sd, wave, n_samples, noise, timbre, dtype=torch.float32, products="exact", fault=None, post_enc=True,
                      entropies=None):
    """One utterance: ``wave[:n_samples]`` at 24 kHz, ``noise`` (512, T) as the reference draws it (channels first), ``timbre`` the
    (192,) CAM++ vector -> dict(spec, m, logs, z, style_vec, gst_out, g).  Without ``post_enc`` (SpeakerEmbedding_wo_PostEnc,
    speaker_encoder.py:399) z = Linear(513, 512)(spec) and there is no m / logs."""
    c = Ctx(sd, dtype, products, fault)
    n = n_samples + HOP if fault == "mask+1" else n_samples
    spec = linear_spectrogram(torch.as_tensor(wave)[:n], dtype)
    out = {"spec": spec}
    if post_enc:
        nz = None if noise is None else torch.as_tensor(noise).to(dtype).t()
        if nz is not None and nz.shape[0] < spec.shape[0]:
            nz = F.pad(nz, (0, 0, 0, spec.shape[0] - nz.shape[0]))
        out.update(posterior_encoder(c, spec, nz))
    else:
        out["z"] = c.linear(spec, c.w("enc_q.weight"), c.w("enc_q.bias"))
    ent = {"style": [], "gst": []} if entropies is None else entropies
    out["style_vec"] = style_encoder(c, out["z"], ent["style"])
    out["gst_out"] = gst(c, out["style_vec"], ent["gst"])
    out["g"] = fuse(c, out["gst_out"], torch.as_tensor(timbre))
    return out


def test_signal(S, seed=0, sr=24000):
    """Speech-like synthetic prompt: a few harmonics with vibrato plus noise, amplitude ~0.3."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S, dtype=torch.float64) / sr
    f0 = 140 + 30 * torch.sin(2 * math.pi * 3 * t)
    ph = 2 * math.pi * torch.cumsum(f0, 0) / sr
    x = sum(0.3 / k * torch.sin(k * ph) for k in range(1, 9))
    x = x * (0.6 + 0.4 * torch.sin(2 * math.pi * 1.7 * t)) + 0.02 * torch.randn(S, generator=g, dtype=torch.float64)
    return x.float()
