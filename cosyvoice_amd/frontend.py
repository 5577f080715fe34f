"""Prompt-feature front half on MI355X: drop-in for the reference's ``mel_spectrogram``
(/root/reference/cosyvoice/dataset/processor_kaldidata.py:37-74, configured by cosyvoice2/conf/cosyvoice.yaml:120-128:
n_fft = win 1920, hop 480, 80 mels, fmin 0, fmax 8000, center=False) and the 24 kHz ``feat = 2 x token`` trimming of
``frontend_zero_shot`` (cli/frontend.py:141-159).

The reference builds its mel basis with ``librosa.filters.mel`` (a third-party dependency that is not in the container and
not pinned by the reference): ``slaney_mel_basis`` restates librosa's published default algorithm (Slaney mel scale,
htk=False, norm='slaney') — **parity unpinned at that boundary**; everything after the basis is pinned by running the
reference function itself with this basis substituted (tests/golden/make_golden.py).

Device path: reflect pad (data movement, torch) -> frames as a strided view of the padded signal (row stride = hop) times a
hann-windowed cos/-sin DFT basis = one fp32 cv_gemm -> |.| (cv_stft_magnitude) -> mel projection (cv_gemm) -> log-clamp +
channels-first store (cv_log_clamp_channels_first).

What turns a recording into those inputs is here as well: ``Resample`` (``torchaudio.transforms.Resample`` of
cli/frontend.py:144,187 and utils/file_utils.py:41-47: polyphase windowed-sinc interpolation as one exact-f32 cv_gemm over a
strided view of the signal; torchaudio is not a pinned part of the reference, so its published ``sinc_interp_hann`` algorithm is
restated — **parity unpinned at that boundary**), ``MelSpectrogram.ragged`` (prompts of different lengths in one
pass, every row bit-identical to that prompt alone) and ``PromptFrontEnd`` (the ``model_input`` dicts of cli/frontend.py:141-195
and the argument lists of ``CosyVoice2Model.tts_batch``)."""
import math

import numpy as np
import torch

from . import _lib as L
from . import ops


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel_basis(sr: int, n_fft: int, n_mels: int, fmin: float, fmax: float) -> np.ndarray:
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with its defaults (htk=False, norm='slaney', float32):
    triangular filters on the Slaney mel scale, each normalised by 2 / (f_hi - f_lo).  Shape (n_mels, n_fft // 2 + 1)."""
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float64)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, None]
    return weights.astype(np.float32)


class MelSpectrogram:
    """Callable with the reference signature: ``y (B, S) float in [-1, 1] -> (B, num_mels, T) float32`` with
    T = (S + 2 * pad - n_fft) // hop + 1, pad = (n_fft - hop) // 2."""

    def __init__(self, n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0, fmax=8000, center=False,
                 device="cuda"):
        if center or win_size != n_fft:
            raise ValueError("built for the reference's configuration: center=False, win_size == n_fft")
        if not torch.cuda.is_available():
            raise RuntimeError("cosyvoice_amd needs an MI355X (no CPU fallback)")
        self.n_fft, self.hop, self.n_mels = n_fft, hop_size, num_mels
        self.nbins = n_fft // 2 + 1
        self.device = torch.device(device)
        assert n_fft % 4 == 0 and hop_size % 4 == 0, "16-byte rows of the frame view"
        # hann-windowed DFT basis, rows = [cos k (nbins) | -sin k (nbins) | zero pad], fp64 -> fp32
        n = torch.arange(n_fft, dtype=torch.float64)
        k = torch.arange(self.nbins, dtype=torch.float64)
        ang = 2.0 * math.pi * torch.outer(k, n) / n_fft
        win = torch.hann_window(win_size, periodic=True, dtype=torch.float64)
        self.ld_spec = (2 * self.nbins + 3) // 4 * 4
        basis = torch.zeros(self.ld_spec, n_fft, dtype=torch.float64)
        basis[:self.nbins] = torch.cos(ang) * win
        basis[self.nbins:2 * self.nbins] = -torch.sin(ang) * win
        self.dft = basis.to(self.device, torch.float32).contiguous()
        self.ld_mag = (self.nbins + 3) // 4 * 4
        mel = torch.zeros(num_mels, self.ld_mag)
        mel[:, :self.nbins] = torch.from_numpy(slaney_mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax))
        self.mel = mel.to(self.device).contiguous()

    @torch.no_grad()
    def __call__(self, y: torch.Tensor) -> torch.Tensor:
        if y.dim() == 1:
            y = y.unsqueeze(0)
        y = y.to(self.device, torch.float32)
        B, S = y.shape
        pad = (self.n_fft - self.hop) // 2
        yp = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
        Sp = yp.shape[1]
        T = (Sp - self.n_fft) // self.hop + 1
        ldp = (Sp + 3) // 4 * 4
        buf = torch.zeros(B, ldp, device=self.device)
        buf[:, :Sp] = yp
        return self._from_padded(buf, B, T)

    def _from_padded(self, buf, B, T):
        """buf (B, ldp) padded signals, ldp % 4 == 0 -> (B, n_mels, T): T frames per row, whatever a row holds there."""
        ldp = buf.shape[1]
        spec = torch.empty(B, T, self.ld_spec, device=self.device)
        # frame t of sequence b = buf[b, t*hop : t*hop + n_fft]: A rows overlap (lda = hop), K = n_fft contiguous
        ops.gemm(buf, self.dft, T, self.ld_spec, self.n_fft, batch=B, a_bs=(ldp, 0), lda=self.hop, a_rows=T,
                 out_f32=spec, o32_bs=(spec.stride(0), 0), ldo32=self.ld_spec)
        mag = torch.empty(B * T, self.ld_mag, device=self.device)
        L.check(L.lib().cv_stft_magnitude(spec.data_ptr(), self.ld_spec, mag.data_ptr(), self.ld_mag, B * T, self.nbins, 1e-9,
                                          L.stream_ptr()), "cv_stft_magnitude")
        melo = torch.empty(B * T, self.n_mels, device=self.device)
        ops.gemm(mag, self.mel, B * T, self.n_mels, self.ld_mag, lda=self.ld_mag, out_f32=melo, ldo32=self.n_mels)
        out = torch.empty(B, self.n_mels, T, device=self.device)
        L.check(L.lib().cv_log_clamp_channels_first(melo.data_ptr(), self.n_mels, out.data_ptr(), B, T, self.n_mels, 1e-5,
                                                    L.stream_ptr()), "cv_log_clamp_channels_first")
        return out

    def num_frames(self, S: int) -> int:
        """Frames of an S-sample signal: (S + 2 * pad - n_fft) // hop + 1."""
        return (S + 2 * ((self.n_fft - self.hop) // 2) - self.n_fft) // self.hop + 1

    @torch.no_grad()
    def ragged(self, waves):
        """Signals of different lengths in one pass: a list of 1-D waveforms, or ``(buf (B, S_max), lens)`` -> (mel (B, n_mels, T_max)
        fp32, frames list[int]).  Every row is reflect-padded at its OWN ends (one index gather builds the padded staging buffer), so
        row b, columns [0, T_b), is bit-identical to ``self(wave_b)``: a frame's K order in the GEMM does not depend on the batch.
        Columns at or past T_b are 0.  What ``buf`` holds past a row's length is never read."""
        buf, S = _stack_waves(waves, self.device)
        B, S_max = buf.shape
        pad = (self.n_fft - self.hop) // 2
        if min(S) <= pad:
            raise ValueError(f"a waveform of {min(S)} samples cannot be reflect-padded by {pad}")
        frames = [self.num_frames(s) for s in S]
        T = max(frames)
        ldp = (S_max + 2 * pad + 3) // 4 * 4
        lens = torch.tensor(S, dtype=torch.int64).to(self.device).unsqueeze(1)
        i = torch.arange(ldp, device=self.device).unsqueeze(0)
        j = (i - pad).abs()
        j = torch.where(j >= lens, 2 * (lens - 1) - j, j)            # reflect at the row's own last sample
        stage = torch.gather(buf, 1, j.clamp_(0, S_max - 1))
        stage = torch.where(i < lens + 2 * pad, stage, torch.zeros((), device=self.device)).contiguous()
        out = self._from_padded(stage, B, T)
        nf = torch.tensor(frames, dtype=torch.int64).to(self.device).view(B, 1, 1)
        out.masked_fill_(torch.arange(T, device=self.device).view(1, 1, T) >= nf, 0.0)
        return out, frames


def _stack_waves(waves, device):
    """(S,) / (B, S) tensor, list of 1-D waveforms or (buf (B, S_max), lens) -> (fp32 (B, S_max) on the device, sample counts)."""
    if isinstance(waves, tuple) and len(waves) == 2 and isinstance(waves[0], torch.Tensor) and waves[0].dim() == 2 \
            and not isinstance(waves[1], torch.Tensor):
        buf, S = waves[0].to(device, torch.float32), [int(s) for s in waves[1]]
        if len(S) != buf.shape[0] or not S or min(S) < 1 or max(S) > buf.shape[1]:
            raise ValueError("lengths do not fit the padded buffer")
        return buf, S
    if isinstance(waves, torch.Tensor):
        if waves.dim() not in (1, 2) or waves.numel() == 0:
            raise ValueError(f"expected a (S,) or (B, S) waveform tensor, got {tuple(waves.shape)}")
        buf = waves.reshape(-1, waves.shape[-1]).to(device, torch.float32)
        return buf, [buf.shape[1]] * buf.shape[0]
    rows = [torch.as_tensor(w).reshape(-1) for w in waves]
    S = [int(w.numel()) for w in rows]
    if not rows or min(S) < 1:
        raise ValueError("no waveform, or an empty one")
    buf = torch.zeros(len(rows), max(S), device=device)
    for b, w in enumerate(rows):
        buf[b, :S[b]].copy_(w)
    return buf, S


RESAMPLE_WEIGHT_CAP = 64 << 20     # bytes of the fp32 device matrix


class Resample:
    """``torchaudio.transforms.Resample(orig_freq, new_freq)`` at its defaults (``sinc_interp_hann``, lowpass_filter_width 6,
    rolloff 0.99) on the device: a (S,) / (B, S) tensor or a list of 1-D waveforms -> (out (B, S_out_max) fp32, out_lens list[int]);
    row b holds ceil(new * S_b / orig) samples and is 0 after them.  ``orig_freq == new_freq`` hands the samples back unfiltered.

    With o = orig / gcd, n = new / gcd, base = min(o, n) * rolloff, width = ceil(lpw * o / base), the published algorithm is
    y[q * n + p] = sum_j k[p][j] * xpad[q * o + j] over the 2 * width + o taps of phase p, xpad = x behind ``width`` zeros, with
    k[p][j] = sinc(pi t) cos^2(pi t / (2 lpw)) base / o at t = clamp((-p / n + (j - width) / o) base, +-lpw) (fp64, stored fp32).
    That is a GEMM over overlapping frames of xpad, as the DFTs of ``MelSpectrogram`` and the Kaldi fbank are: g = 4 / gcd(o, 4) input
    strides are blocked into one row so that rows stay 16-byte aligned (lda = g * o, N = g * n, K = 2 * width + g * o rounded up to 4,
    W[r * n + p][r * o + j] = k[p][j]), the fp32 output with ldo32 = N is the interleaved signal itself, and the whole batch is one
    exact-f32 cv_gemm launch.  A batch row is bit-identical to that waveform resampled alone."""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, device="cuda"):
        orig_freq, new_freq = int(orig_freq), int(new_freq)
        if orig_freq <= 0 or new_freq <= 0 or lowpass_filter_width <= 0:
            raise ValueError("sample rates and the filter width must be positive")
        self.orig_freq, self.new_freq, self.lpw, self.rolloff = orig_freq, new_freq, lowpass_filter_width, rolloff
        self.device = torch.device(device)
        g0 = math.gcd(orig_freq, new_freq)
        self.o, self.n = orig_freq // g0, new_freq // g0
        self.base = min(self.o, self.n) * rolloff
        self.width = math.ceil(lowpass_filter_width * self.o / self.base)
        self.g = 4 // math.gcd(self.o, 4)
        self.lda, self.N = self.g * self.o, self.g * self.n
        self.K = (2 * self.width + self.g * self.o + 3) // 4 * 4
        if orig_freq != new_freq and self.N * self.K * 4 > RESAMPLE_WEIGHT_CAP:
            raise ValueError(f"{orig_freq} -> {new_freq} Hz needs a {self.N} x {self.K} interpolation matrix (over "
                             f"{RESAMPLE_WEIGHT_CAP >> 20} MB): resample through an intermediate rate")
        self._w64, self._w = None, None

    def kernel(self) -> np.ndarray:
        """k (n, 2 * width + o) float64: the taps of every output phase."""
        o, n, w = self.o, self.n, self.width
        p = np.arange(n, dtype=np.float64)[:, None]
        j = np.arange(-w, w + o, dtype=np.float64)[None, :]
        t = np.clip((-p / n + j / o) * self.base, -self.lpw, self.lpw)
        window = np.cos(t * math.pi / self.lpw / 2) ** 2
        t = t * math.pi
        sinc = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
        return sinc * window * (self.base / o)

    def weights(self) -> np.ndarray:
        """The blocked interpolation matrix W (N, K) in float64 (the device holds its fp32 rounding), built once."""
        if self._w64 is None:
            k = self.kernel()
            taps = k.shape[1]
            W = np.zeros((self.N, self.K), dtype=np.float64)
            for r in range(self.g):
                W[r * self.n:(r + 1) * self.n, r * self.o:r * self.o + taps] = k
            self._w64 = W
        return self._w64

    def out_len(self, S: int) -> int:
        return (self.n * int(S) + self.o - 1) // self.o

    @torch.no_grad()
    def __call__(self, waves):
        if not torch.cuda.is_available():
            raise RuntimeError("cosyvoice_amd needs an MI355X (no CPU fallback)")
        dev = self.device
        if self.orig_freq == self.new_freq:
            return _stack_waves(waves, dev)
        if isinstance(waves, torch.Tensor):
            if waves.dim() not in (1, 2) or waves.numel() == 0:
                raise ValueError(f"expected a (S,) or (B, S) waveform tensor, got {tuple(waves.shape)}")
            rows = waves.reshape(-1, waves.shape[-1])
        else:
            rows = [torch.as_tensor(w).reshape(-1) for w in waves]
        S = [int(w.numel()) for w in rows]
        if not S or min(S) < 1:
            raise ValueError("no waveform, or an empty one")
        if self._w is None:
            self._w = torch.from_numpy(self.weights().astype(np.float32)).to(dev).contiguous()
        B = len(S)
        lens = [self.out_len(s) for s in S]
        M = (max(lens) + self.N - 1) // self.N
        # row b of the staging buffer = xpad of waveform b: ``width`` zeros, the signal, zeros; GEMM row m reads [m * lda, m * lda + K)
        ld = (M - 1) * self.lda + self.K
        stage = torch.zeros(B, ld, device=dev)
        if isinstance(rows, torch.Tensor):
            stage[:, self.width:self.width + S[0]].copy_(rows)
        else:
            for b, w in enumerate(rows):
                stage[b, self.width:self.width + S[b]].copy_(w)
        out = torch.empty(B, M * self.N, device=dev)
        ops.gemm(stage, self._w, M, self.N, self.K, batch=B, a_bs=(ld, 0), lda=self.lda, a_rows=M, out_f32=out,
                 o32_bs=(M * self.N, 0), ldo32=self.N, dtype=L.CV_F32)
        out = out[:, :max(lens)]
        # the frames behind the last input sample ring on past ceil(n * S / o): the published algorithm truncates there
        nl = torch.tensor(lens, dtype=torch.int64).to(dev).unsqueeze(1)
        out.masked_fill_(torch.arange(max(lens), device=dev).unsqueeze(0) >= nl, 0.0)
        return out, lens


def to_16k(wave, sample_rate, device="cuda"):
    """utils/file_utils.py:41-47 (``load_wav`` behind the file read): (channels, S) or (S,) at ``sample_rate`` -> the channel mean at
    16 kHz, (out (1, S_16k) fp32 on the device, [S_16k])."""
    wave = torch.as_tensor(wave)
    if wave.dim() == 2:
        wave = wave.to(torch.float32).mean(dim=0)
    return Resample(sample_rate, 16000, device=device)(wave)


def align_prompt_24k(speech_feat: torch.Tensor, speech_token: torch.Tensor):
    """cli/frontend.py:148-152 (cosyvoice2): force feat_len == 2 * token_len.  speech_feat (1, T, 80), speech_token (1, N)
    -> (speech_feat[:, :2n], speech_feat_len, speech_token[:, :n], speech_token_len) with n = min(T // 2, N)."""
    n = min(int(speech_feat.shape[1] / 2), speech_token.shape[1])
    return (speech_feat[:, :2 * n], torch.tensor([2 * n], dtype=torch.int32), speech_token[:, :n], torch.tensor([n], dtype=torch.int32))


def extract_speech_feat(feat_extractor, speech: torch.Tensor):
    """cli/frontend.py:102-106: (1, S) waveform -> (speech_feat (1, T, 80), speech_feat_len (1,) int32)."""
    feat = feat_extractor(speech).squeeze(dim=0).transpose(0, 1).unsqueeze(dim=0)
    return feat, torch.tensor([feat.shape[1]], dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# model_input assembly (cli/frontend.py:141-195).  Pure functions of finished tensors (host or device): every length comes from a
# shape, nothing is read back from the device.

def _len32(n):
    return torch.tensor([int(n)], dtype=torch.int32)


def _row(t):
    """(N,) / (1, N) int tokens -> (1, N)."""
    t = torch.as_tensor(t)
    return t.reshape(1, -1)


def assemble_zero_shot(text, prompt_text, speech_feat, speech_token, embedding, resample_rate):
    """cli/frontend.py:147-159: the 12-key ``model_input`` from the text tokens (1, n), the prompt mel (1, T, 80), the prompt speech
    tokens and the speaker embedding (1, 192).  At 24 kHz (cosyvoice2) feat and tokens are cut to feat_len == 2 * token_len."""
    text, prompt_text, speech_token = _row(text), _row(prompt_text), _row(speech_token)
    feat_len, token_len = _len32(speech_feat.shape[1]), _len32(speech_token.shape[1])
    if resample_rate == 24000:
        speech_feat, feat_len, speech_token, token_len = align_prompt_24k(speech_feat, speech_token)
    return {"text": text, "text_len": _len32(text.shape[1]),
            "prompt_text": prompt_text, "prompt_text_len": _len32(prompt_text.shape[1]),
            "llm_prompt_speech_token": speech_token, "llm_prompt_speech_token_len": token_len,
            "flow_prompt_speech_token": speech_token, "flow_prompt_speech_token_len": token_len,
            "prompt_speech_feat": speech_feat, "prompt_speech_feat_len": feat_len,
            "llm_embedding": embedding, "flow_embedding": embedding}


def assemble_cross_lingual(text, speech_feat, speech_token, embedding, resample_rate):
    """cli/frontend.py:161-168: zero-shot without the LLM's prompt (8 keys)."""
    d = assemble_zero_shot(text, torch.zeros(1, 0, dtype=torch.int32), speech_feat, speech_token, embedding, resample_rate)
    for k in ("prompt_text", "prompt_text_len", "llm_prompt_speech_token", "llm_prompt_speech_token_len"):
        del d[k]
    return d


def assemble_instruct2(text, instruct_text, speech_feat, speech_token, embedding, resample_rate):
    """cli/frontend.py:179-183: the instruction (its tokens, end-of-prompt marker included) as prompt text, no LLM speech prompt
    (10 keys)."""
    d = assemble_zero_shot(text, instruct_text, speech_feat, speech_token, embedding, resample_rate)
    for k in ("llm_prompt_speech_token", "llm_prompt_speech_token_len"):
        del d[k]
    return d


def assemble_vc(source_speech_token, prompt_speech_feat, prompt_speech_token, embedding):
    """cli/frontend.py:185-195: the 7-key voice-conversion input (no 24 kHz trim there)."""
    src, tok = _row(source_speech_token), _row(prompt_speech_token)
    return {"source_speech_token": src, "source_speech_token_len": _len32(src.shape[1]),
            "flow_prompt_speech_token": tok, "flow_prompt_speech_token_len": _len32(tok.shape[1]),
            "prompt_speech_feat": prompt_speech_feat, "prompt_speech_feat_len": _len32(prompt_speech_feat.shape[1]),
            "flow_embedding": embedding}


def assemble_batch(texts, prompt_texts, speech_feats, speech_tokens, embeddings, resample_rate=24000, adapters=None):
    """B prompts -> the arguments of ``CosyVoice2Model.tts_batch`` by name (also one ``tts_batches`` batch).  ``speech_feats``: per
    utterance (1, T_b, 80); ``speech_tokens``: per utterance (N_b,) / (1, N_b); ``embeddings`` (B, 192).  Each prompt is trimmed as
    ``assemble_zero_shot`` trims it.  Prompts that end up with the same lengths are stacked — (B, Np) tokens, (B, Tp, 80) feats, the
    equal-shape flow pass; otherwise the entries are lists of (Np_b,) / (Tp_b, 80) and the flow runs its ragged pass.  ``adapters``: per
    utterance the LoRA adapter of the LLM's attached bank (``tts_batch``'s ``adapters``; None = the base path)."""
    B = len(texts)
    if adapters is not None and len(adapters) != B:
        raise ValueError("one adapter per utterance")
    if not (len(prompt_texts) == len(speech_feats) == len(speech_tokens) == embeddings.shape[0] == B) or B == 0:
        raise ValueError("one text, prompt text, prompt mel, token row and embedding row per utterance")
    feats, toks = [], []
    for f, t in zip(speech_feats, speech_tokens):
        t = _row(t)
        if resample_rate == 24000:
            f, _, t, _ = align_prompt_24k(f, t)
        feats.append(f[0])
        toks.append(t[0])
    same = all(f.shape == feats[0].shape and t.shape == toks[0].shape for f, t in zip(feats, toks))
    return {"texts": [_row(t) for t in texts], "prompt_texts": [_row(t) for t in prompt_texts],
            "llm_prompt_speech_tokens": [t.unsqueeze(0) for t in toks],
            "flow_prompt_speech_tokens": torch.stack(toks) if same else toks,
            "prompt_speech_feats": torch.stack(feats) if same else feats,
            "flow_embeddings": embeddings, "adapters": None if adapters is None else list(adapters)}


class PromptFrontEnd:
    """The prompt half of ``CosyVoiceFrontEnd`` (cli/frontend.py:141-195) on the device: 16 kHz prompt waveform + token ids in, the
    reference's ``model_input`` dicts out.  ``feat_extractor``: a ``MelSpectrogram`` at the model's rate; ``campplus``: a loaded
    ``speaker.CAMPPlus``.  Text and speech tokens come in as int tensors (the tokenizers and the speech-tokenizer model are not part
    of this package).  ``batch`` serves ``tts_batch`` / ``tts_batches``: B prompts of any lengths through ONE resampling launch, one
    ragged mel pass and one speaker-embedding graph; all lengths follow from the sample counts on the host, so nothing waits for
    the device between the upload and the returned tensors.

    ``speaker_encoder`` (optional): a loaded ``style.SpeakerEmbedding`` / ``SpeakerEmbeddingWoPostEnc``.  When given, the embedding of
    the dicts and of ``batch`` is its 512-d vector of the 24 kHz prompt (what the recipes with ``spk_embed_dim: 512`` condition on)
    instead of the 192-d CAM++ vector; its posterior noise is drawn per call, as the reference draws it."""

    def __init__(self, feat_extractor, campplus, device="cuda", speaker_encoder=None):
        self.feat_extractor, self.campplus, self.speaker_encoder = feat_extractor, campplus, speaker_encoder
        self.device = torch.device(device)
        self._resamplers = {}

    def resampler(self, resample_rate):
        r = self._resamplers.get(resample_rate)
        if r is None:
            r = self._resamplers[resample_rate] = Resample(16000, resample_rate, device=self.device)
        return r

    @torch.no_grad()
    def prompt_features(self, prompt_speech_16k, resample_rate):
        """list of 16 kHz waveforms ((S,) or (1, S)) -> (per utterance prompt mel (1, T_b, 80), embeddings (B, 192) — (B, 512) with a
        ``speaker_encoder``), on the device."""
        waves = [torch.as_tensor(w).reshape(-1) for w in prompt_speech_16k]
        buf, lens = self.resampler(resample_rate)(waves)
        mel, frames = self.feat_extractor.ragged((buf, lens))
        if self.speaker_encoder is None:
            emb = self.campplus.extract_spk_embedding(waves)
        else:
            b24, l24 = (buf, lens) if resample_rate == 24000 else self.resampler(24000)(waves)
            emb = self.speaker_encoder(b24, wave_lengths=l24)
        mel = mel.transpose(1, 2)                                           # (B, T_max, 80)
        return [mel[b:b + 1, :frames[b]] for b in range(len(waves))], emb

    def frontend_zero_shot(self, text, prompt_text, prompt_speech_16k, speech_token, resample_rate):
        feats, emb = self.prompt_features([prompt_speech_16k], resample_rate)
        return assemble_zero_shot(text, prompt_text, feats[0], speech_token, emb, resample_rate)

    def frontend_cross_lingual(self, text, prompt_speech_16k, speech_token, resample_rate):
        feats, emb = self.prompt_features([prompt_speech_16k], resample_rate)
        return assemble_cross_lingual(text, feats[0], speech_token, emb, resample_rate)

    def frontend_instruct2(self, text, instruct_text, prompt_speech_16k, speech_token, resample_rate):
        feats, emb = self.prompt_features([prompt_speech_16k], resample_rate)
        return assemble_instruct2(text, instruct_text, feats[0], speech_token, emb, resample_rate)

    def frontend_vc(self, source_speech_token, prompt_speech_16k, prompt_speech_token, resample_rate):
        feats, emb = self.prompt_features([prompt_speech_16k], resample_rate)
        return assemble_vc(source_speech_token, feats[0], prompt_speech_token, emb)

    def batch(self, texts, prompt_texts, prompt_speech_16k, speech_tokens, resample_rate=24000, adapters=None):
        feats, emb = self.prompt_features(prompt_speech_16k, resample_rate)
        return assemble_batch(texts, prompt_texts, feats, speech_tokens, emb, resample_rate, adapters)
