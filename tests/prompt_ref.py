"""CPU restatement of the prompt front end of CosyVoiceFrontEnd (cosyvoice/cli/frontend.py:141-195), step by step and independent
of cosyvoice_amd.frontend:

* ``sinc_resample`` — torchaudio.transforms.Resample(orig, new) at its defaults (``sinc_interp_hann``, lowpass_filter_width 6,
  rolloff 0.99), restated from torchaudio's published ``_get_sinc_resample_kernel`` / ``_apply_sinc_resample_kernel`` as one strided
  ``torch.conv1d`` (torchaudio is not in the container: parity unpinned at that boundary; tests/test_prompt_cpu.py checks the
  restatement against an analytic sine instead);
* ``zero_shot`` / ``cross_lingual`` / ``instruct2`` / ``vc`` — the ``model_input`` dicts of frontend.py:141-195 with the token ids, the
  prompt mel and the speaker embedding given as finished tensors;
* ``prompt_feat`` — resample -> ``oracle.frontend.mel_spectrogram`` -> (1, T, 80), the chain of frontend.py:144-145 / :102-106.
"""
import math

import torch


def resample_geometry(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """(o, n, base, width): the reduced rates, the cut-off in units of the reduced rates and the filter half-width in input samples."""
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * rolloff
    return o, n, base, math.ceil(lowpass_filter_width * o / base)


def sinc_kernel(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """(n, 1, 2 * width + o) float64: one windowed-sinc filter per output phase."""
    o, n, base, width = resample_geometry(orig, new, lowpass_filter_width, rolloff)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t = (t * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    sinc = torch.where(t == 0, torch.ones_like(t), t.sin() / torch.where(t == 0, torch.ones_like(t), t))
    return sinc * window * (base / o), width


def resample_len(S, orig, new):
    o, n, _, _ = resample_geometry(orig, new)
    return -(-n * S // o)


def sinc_resample(x, orig, new, lowpass_filter_width=6, rolloff=0.99, dtype=torch.float64):
    """1-D waveform -> 1-D resampled waveform of ceil(new * S / orig) samples.  The filters are computed in float64 and cast to
    ``dtype``, the convolution runs in ``dtype`` (float32 = what torchaudio does to a float32 waveform)."""
    x = torch.as_tensor(x).reshape(-1).to(dtype)
    if int(orig) == int(new):
        return x
    o, n, _, _ = resample_geometry(orig, new, lowpass_filter_width, rolloff)
    k, width = sinc_kernel(orig, new, lowpass_filter_width, rolloff)
    xp = torch.nn.functional.pad(x[None, None], (width, width + o))
    y = torch.nn.functional.conv1d(xp, k.to(dtype), stride=o)           # (1, n, frames)
    return y.transpose(1, 2).reshape(-1)[:resample_len(x.numel(), orig, new)]


def mel_frames(S, n_fft=1920, hop=480):
    return (S + 2 * ((n_fft - hop) // 2) - n_fft) // hop + 1


def prompt_feat(wave_16k, resample_rate, mel_basis, **mel_kw):
    """frontend.py:144-145 with :102-106: (S,) 16 kHz -> (1, T, 80) float32 log-mel of the resampled prompt."""
    from oracle import frontend as ofe
    y = sinc_resample(wave_16k, 16000, resample_rate).float()
    return ofe.mel_spectrogram(y[None], mel_basis, **mel_kw).squeeze(0).transpose(0, 1).unsqueeze(0)


def _n(t):
    return torch.tensor([t.shape[1]], dtype=torch.int32)


def zero_shot(text, prompt_text, speech_feat, speech_token, embedding, resample_rate):
    """frontend.py:141-159.  text / prompt_text / speech_token (1, n) ints, speech_feat (1, T, 80), embedding (1, 192)."""
    feat_len, token_len = _n(speech_feat), _n(speech_token)
    if resample_rate == 24000:                                           # :147-151 cosyvoice2: feat_len == 2 * token_len
        k = min(int(speech_feat.shape[1] / 2), speech_token.shape[1])
        speech_feat, speech_token = speech_feat[:, :2 * k], speech_token[:, :k]
        feat_len[:], token_len[:] = 2 * k, k
    return {"text": text, "text_len": _n(text), "prompt_text": prompt_text, "prompt_text_len": _n(prompt_text),               # :153-158
            "llm_prompt_speech_token": speech_token, "llm_prompt_speech_token_len": token_len,
            "flow_prompt_speech_token": speech_token, "flow_prompt_speech_token_len": token_len,
            "prompt_speech_feat": speech_feat, "prompt_speech_feat_len": feat_len,
            "llm_embedding": embedding, "flow_embedding": embedding}


def cross_lingual(text, speech_feat, speech_token, embedding, resample_rate):
    """frontend.py:161-168."""
    d = zero_shot(text, torch.zeros(1, 0, dtype=torch.int32), speech_feat, speech_token, embedding, resample_rate)
    for k in ("prompt_text", "prompt_text_len", "llm_prompt_speech_token", "llm_prompt_speech_token_len"):
        d.pop(k)
    return d


def instruct2(text, instruct_text, speech_feat, speech_token, embedding, resample_rate):
    """frontend.py:179-183."""
    d = zero_shot(text, instruct_text, speech_feat, speech_token, embedding, resample_rate)
    d.pop("llm_prompt_speech_token")
    d.pop("llm_prompt_speech_token_len")
    return d


def vc(source_speech_token, prompt_speech_feat, prompt_speech_token, embedding):
    """frontend.py:185-195."""
    return {"source_speech_token": source_speech_token, "source_speech_token_len": _n(source_speech_token),
            "flow_prompt_speech_token": prompt_speech_token, "flow_prompt_speech_token_len": _n(prompt_speech_token),
            "prompt_speech_feat": prompt_speech_feat, "prompt_speech_feat_len": _n(prompt_speech_feat),
            "flow_embedding": embedding}


ZERO_SHOT_KEYS = ("text", "text_len", "prompt_text", "prompt_text_len", "llm_prompt_speech_token", "llm_prompt_speech_token_len",
                  "flow_prompt_speech_token", "flow_prompt_speech_token_len", "prompt_speech_feat", "prompt_speech_feat_len",
                  "llm_embedding", "flow_embedding")
CROSS_LINGUAL_KEYS = tuple(k for k in ZERO_SHOT_KEYS if k not in ("prompt_text", "prompt_text_len", "llm_prompt_speech_token",
                                                                  "llm_prompt_speech_token_len"))
INSTRUCT2_KEYS = tuple(k for k in ZERO_SHOT_KEYS if k not in ("llm_prompt_speech_token", "llm_prompt_speech_token_len"))
VC_KEYS = ("source_speech_token", "source_speech_token_len", "flow_prompt_speech_token", "flow_prompt_speech_token_len",
           "prompt_speech_feat", "prompt_speech_feat_len", "flow_embedding")
