"""Speaker embedding on MI355X: CosyVoiceFrontEnd._extract_spk_embedding (/root/reference/cosyvoice/cli/frontend.py:91-100) =
Kaldi fbank of the 16 kHz prompt (80 bins, dither 0) minus its per-bin mean, then CAM++ (cosyvoice/speaker/CAMPPlus.py:384-451,
the reference's campplus.onnx) -> the 192-d ``flow_embedding`` / v1 x-vector.

The fbank restates torchaudio.compliance.kaldi.fbank at its defaults (torchaudio is not a pinned part of the reference): frames of
400 samples, shift 160, snip_edges; per frame DC removal, pre-emphasis 0.97 (x[-1] := x[0]), Povey window, zero pad to 512, power
spectrum, Kaldi mel banks (20 Hz .. Nyquist, triangles in 1127 ln(1 + f / 700)), log(max(., FLT_EPSILON)) — **parity unpinned at
that boundary** (DESIGN.md §2).  The three per-frame steps are linear, so they are folded into the DFT basis: the frames (a strided
view of the waveform, lda = 160) times a [cos | sin] x 256-bin basis is one fp32 cv_gemm, then cv_spk_power, the mel projection
(cv_gemm) and cv_spk_log_cmn.

CAM++ runs channels-last: the FCM head's (time, frequency) rows x 32 channels, then [time][channels] for the TDNN part.  Every
conv is cv_spk_conv (exact-f32 MFMA); BatchNorms after a conv are folded into its weights at load_state_dict, BatchNorm -> ReLU
before a conv is the conv's A-operand prologue; the dense blocks write their 32 new channels at their column offset of one
preallocated block buffer (the concatenation costs nothing); the CAM gate is one small kernel per layer over 4-row partial sums
written by the bottleneck conv's epilogue.  One call = ~180 launches, captured once per padded shape as a graph.

Ragged batches: lengths travel on the device; a batch row is bit-identical to that prompt run alone."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .weights import CAMPPLUS_BLOCKS, CAMPPLUS_EMBED

SAMPLE_RATE, WIN, HOP, NFFT, NBINS, NMELS = 16000, 400, 160, 512, 256, 80
SEG_LEN = 100          # CAMLayer.seg_pooling segment length
BN_EPS = 1e-5
FLT_EPSILON = float(np.finfo(np.float32).eps)


def num_frames(S: int) -> int:
    """Kaldi frame count with snip_edges=True: 1 + (S - 400) // 160, none when S < 400."""
    return 0 if S < WIN else 1 + (S - WIN) // HOP


def tdnn_frames(T: int) -> int:
    """Frames after the stride-2, k5, pad-2 TDNN conv."""
    return (T - 1) // 2 + 1


def povey_window(n: int = WIN) -> np.ndarray:
    i = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2 * math.pi * i / (n - 1))) ** 0.85


def kaldi_mel_banks(n_mels: int = NMELS, n_fft: int = NFFT, sr: int = SAMPLE_RATE, low: float = 20.0) -> np.ndarray:
    """(n_mels, n_fft // 2) triangles in the mel domain over FFT bins 0 .. n_fft/2 - 1 (the Nyquist bin has zero weight)."""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)  # noqa: E731
    lo, hi = mel(low), mel(sr / 2.0)
    delta = (hi - lo) / (n_mels + 1)
    m = mel(np.arange(n_fft // 2) * (sr / n_fft))
    left = lo + np.arange(n_mels)[:, None] * delta
    up = (m[None] - left) / delta
    down = (left + 2 * delta - m[None]) / delta
    return np.maximum(0.0, np.minimum(up, down))


def fbank_basis() -> np.ndarray:
    """(2 * 256, 400): rows [cos k | sin k] of the 512-point DFT applied after DC removal, pre-emphasis and the Povey window,
    all folded into one linear map of the 400 raw frame samples."""
    n = WIN
    dc = np.eye(n) - 1.0 / n
    pre = np.eye(n)
    pre[np.arange(1, n), np.arange(n - 1)] = -0.97
    pre[0, 0] = 1.0 - 0.97
    frame = povey_window(n)[:, None] * (pre @ dc)
    ang = 2 * math.pi * np.outer(np.arange(NBINS), np.arange(n)) / NFFT
    return np.concatenate([np.cos(ang), np.sin(ang)]) @ frame


def _check(rc, what):
    L.check(rc, what)


def _lens_dev(lens, device):
    return torch.tensor(lens, dtype=torch.int32).to(device)


class _Fbank:
    """Device constants + the four launches of the fbank (DFT gemm, power, mel gemm, log / CMN)."""

    def __init__(self, device):
        self.dft = torch.from_numpy(fbank_basis()).to(device, torch.float32).contiguous()
        self.mel = torch.from_numpy(kaldi_mel_banks()).to(device, torch.float32).contiguous()

    def enqueue(self, wave, ldw, lens, B, T, cmn, spec, pw, melo, out, ldo):
        ops.gemm(wave, self.dft, T, 2 * NBINS, WIN, batch=B, a_bs=(ldw, 0), lda=HOP, a_rows=T, out_f32=spec,
                 o32_bs=(T * 2 * NBINS, 0), ldo32=2 * NBINS, dtype=L.CV_F32)
        st = L.stream_ptr()
        _check(L.lib().cv_spk_power(spec.data_ptr(), 2 * NBINS, pw.data_ptr(), NBINS, B * T, NBINS, st),
               "cv_spk_power")
        ops.gemm(pw, self.mel, B * T, NMELS, NBINS, lda=NBINS, out_f32=melo, ldo32=NMELS, dtype=L.CV_F32)
        _check(L.lib().cv_spk_log_cmn(melo.data_ptr(), NMELS, lens.data_ptr(), B, T, NMELS, int(cmn),
                                      out.data_ptr(), ldo, st), "cv_spk_log_cmn")


def _pad_waves(waves):
    """(B, S) tensor / (S,) / list of 1-D waveforms -> (padded fp32 CPU (B, S_pad), sample counts).  S_pad is a multiple of 1600
    (0.1 s): fewer distinct shapes to capture, and the padding is never read into a sequence's own frames."""
    if isinstance(waves, torch.Tensor) and waves.dim() <= 2:
        waves = [waves] if waves.dim() == 1 else list(waves)
    waves = [torch.as_tensor(w).detach().reshape(-1).to("cpu", torch.float32) for w in waves]
    if not waves:
        raise ValueError("no waveform")
    S = [int(w.numel()) for w in waves]
    if min(S) < WIN:
        raise ValueError(f"a waveform of {min(S)} samples is shorter than one {WIN}-sample Kaldi frame")
    S_pad = (max(S) + 1599) // 1600 * 1600
    buf = torch.zeros(len(waves), S_pad)
    for i, w in enumerate(waves):
        buf[i, :S[i]] = w
    return buf, S


class KaldiFbank:
    """torchaudio.compliance.kaldi.fbank(wave, num_mel_bins=80, sample_frequency=16000, dither=0) on the device, batched:
    (B, S) tensor or a list of 1-D waveforms -> (feat (B, T, 80) fp32, frames (B,) int32); no CMN; frames past a length are 0."""

    def __init__(self, num_mel_bins=NMELS, sample_frequency=SAMPLE_RATE, device="cuda"):
        if num_mel_bins != NMELS or sample_frequency != SAMPLE_RATE:
            raise ValueError("built for the reference's configuration: 80 bins at 16 kHz")
        if not torch.cuda.is_available():
            raise RuntimeError("cosyvoice_amd needs an MI355X (no CPU fallback)")
        self.device = torch.device(device)
        self.fb = _Fbank(self.device)

    @torch.no_grad()
    def __call__(self, waves):
        buf, S = _pad_waves(waves)
        B, S_pad = buf.shape
        T = num_frames(S_pad)
        dev = self.device
        wave = buf.to(dev)
        lens = [num_frames(s) for s in S]
        spec = torch.empty(B * T, 2 * NBINS, device=dev)
        pw = torch.empty(B * T, NBINS, device=dev)
        melo = torch.empty(B * T, NMELS, device=dev)
        out = torch.empty(B, T, NMELS, device=dev)
        self.fb.enqueue(wave, S_pad, _lens_dev(lens, dev), B, T, False, spec, pw, melo, out, NMELS)
        Tm = max(lens)
        return out[:, :Tm], torch.tensor(lens, dtype=torch.int32)


def _bn_affine(sd, p):
    """(scale, shift) of an eval-mode BatchNorm: y = x * scale + shift (float64)."""
    rv = sd[p + ".running_var"].double()
    s = 1.0 / torch.sqrt(rv + BN_EPS)
    if p + ".weight" in sd:
        s = s * sd[p + ".weight"].double()
    h = -sd[p + ".running_mean"].double() * s
    if p + ".bias" in sd:
        h = h + sd[p + ".bias"].double()
    return s, h


def _pad_k(w2d):
    K = w2d.shape[1]
    Kp = (K + 15) // 16 * 16
    return torch.nn.functional.pad(w2d, (0, Kp - K)) if Kp != K else w2d


class CAMPPlus:
    """CAMPPlus(feat_dim=80, embedding_size=192) with the reference's state-dict keys.  ``model(x (B, 80, T), lengths=None)``
    -> (B, 192) fp32 on the device; ``lengths`` = frames per row (default T)."""

    def __init__(self, feat_dim=NMELS, embedding_size=CAMPPLUS_EMBED, device="cuda"):
        if feat_dim != NMELS or embedding_size != CAMPPLUS_EMBED:
            raise ValueError("built for CAMPPlus(feat_dim=80, embedding_size=192)")
        if not torch.cuda.is_available():
            raise RuntimeError("cosyvoice_amd needs an MI355X (no CPU fallback)")
        self.device = torch.device(device)
        self.fb = _Fbank(self.device)
        self.p = None
        self._ws, self._graphs = {}, {}

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd):
        """Reference keys (num_batches_tracked accepted and ignored); BatchNorms folded, weights packed K-major."""
        ops.drop_graphs(self._graphs)
        self._ws.clear()
        dev = self.device
        f32 = lambda t: t.to(dev, torch.float32).contiguous()  # noqa: E731
        P = {}

        def conv2d(name, bn):
            w = sd[name].double()
            co, ci, kh, kw = w.shape
            s, h = _bn_affine(sd, bn)
            wp = w.permute(0, 2, 3, 1).reshape(co, kh * kw * ci) * s[:, None]
            return f32(_pad_k(wp)), f32(h)

        P["c1"] = conv2d("head.conv1.weight", "head.bn1")
        for layer in ("layer1", "layer2"):
            for i in (0, 1):
                p = f"head.{layer}.{i}"
                P[p + ".c1"] = conv2d(p + ".conv1.weight", p + ".bn1")
                P[p + ".c2"] = conv2d(p + ".conv2.weight", p + ".bn2")
                if p + ".shortcut.0.weight" in sd:
                    P[p + ".sc"] = conv2d(p + ".shortcut.0.weight", p + ".shortcut.1")
        P["c2"] = conv2d("head.conv2.weight", "head.bn2")
        # TDNN: reference input channel c * 10 + f; the head writes f * 32 + c -> permute the weight columns instead of the data
        w = sd["xvector.tdnn.linear.weight"].double()                        # (128, 320, 5)
        s, h = _bn_affine(sd, "xvector.tdnn.nonlinear.batchnorm")
        wp = w.reshape(128, 32, 10, 5).permute(0, 3, 2, 1).reshape(128, 5 * 320) * s[:, None]
        P["tdnn"] = (f32(wp), f32(h))
        ch = 128
        for bi, (n, dil) in enumerate(CAMPPLUS_BLOCKS, 1):
            for i in range(n):
                p = f"xvector.block{bi}.tdnnd{i + 1}"
                s1, h1 = _bn_affine(sd, p + ".nonlinear1.batchnorm")
                s2, h2 = _bn_affine(sd, p + ".nonlinear2.batchnorm")
                w1 = sd[p + ".linear1.weight"].double()[:, :, 0] * s2[:, None]
                wl = sd[p + ".cam_layer.linear_local.weight"].double().permute(0, 2, 1).reshape(32, 3 * 128)
                P[p] = dict(pre=(f32(s1), f32(h1)), w1=f32(w1), b1=f32(h2), wl=f32(wl),
                            g1=f32(sd[p + ".cam_layer.linear1.weight"][:, :, 0]), gb1=f32(sd[p + ".cam_layer.linear1.bias"]),
                            g2=f32(sd[p + ".cam_layer.linear2.weight"][:, :, 0]), gb2=f32(sd[p + ".cam_layer.linear2.bias"]))
            ch += 32 * n
            s, h = _bn_affine(sd, f"xvector.transit{bi}.nonlinear.batchnorm")
            P[f"transit{bi}"] = dict(pre=(f32(s), f32(h)), w=f32(sd[f"xvector.transit{bi}.linear.weight"][:, :, 0]))
            ch //= 2
        s, h = _bn_affine(sd, "xvector.out_nonlinear.batchnorm")
        P["out_nl"] = (f32(s), f32(h))
        s, h = _bn_affine(sd, "xvector.dense.nonlinear.batchnorm")
        P["dense"] = (f32(sd["xvector.dense.linear.weight"].double()[:, :, 0] * s[:, None]), f32(h))
        self.p = P
        return self

    # ------------------------------------------------------------------ launches
    @staticmethod
    def _conv(x, x_bs, ldx, T_in, F_in, cin, w, y, y_bs, ldy, T_out, F_out, B, *, k=(1, 1), s=(1, 1), pad=(0, 0), dt=1, in_len=None,
              out_len=None, pre=None, bias=None, res=None, relu=False, gate=None, gate_bs=0, psum=None, psum_bs=0, y_off=0):
        p = L.SpkConvParams()
        p.B, p.T_in, p.F_in, p.cin = B, T_in, F_in, cin
        p.x, p.x_bs, p.ldx, p.in_len = x.data_ptr(), x_bs, ldx, L.ptr(in_len)
        p.kf, p.kt, p.sf, p.st, p.dt, p.pf, p.pt = k[0], k[1], s[0], s[1], dt, pad[0], pad[1]
        if pre is not None:
            p.pre_scale, p.pre_shift = pre[0].data_ptr(), pre[1].data_ptr()
        p.w, p.ldw = w.data_ptr(), w.shape[1]
        p.N, p.T_out, p.F_out = w.shape[0], T_out, F_out
        p.bias = L.ptr(bias)
        if res is not None:
            p.res, p.res_bs, p.ldres = res.data_ptr(), y_bs, ldy
        p.relu = int(relu)
        if gate is not None:
            p.gate, p.gate_bs, p.gate_seg = gate.data_ptr(), gate_bs, SEG_LEN
        p.y, p.y_bs, p.ldy = y.data_ptr() + 4 * y_off, y_bs, ldy
        p.out_len = L.ptr(out_len)
        p.psum, p.psum_bs = L.ptr(psum), psum_bs
        _check(L.lib().cv_spk_conv(C.byref(p), L.stream_ptr()), "cv_spk_conv")

    def _workspace(self, B, T, S_pad=0):
        dev = self.device
        T2 = tdnn_frames(T)
        e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
        ws = dict(B=B, T=T, T2=T2, S_pad=S_pad,
                  lens=torch.zeros(B, dtype=torch.int32, device=dev), lens2=torch.zeros(B, dtype=torch.int32, device=dev),
                  feat=e(B, T, NMELS), a80=e(B, T, 80, 32), h40=e(B, T, 40, 32), s40=e(B, T, 40, 32), x40=e(B, T, 40, 32),
                  y40=e(B, T, 40, 32), h20=e(B, T, 20, 32), s20=e(B, T, 20, 32), x20=e(B, T, 20, 32), y20=e(B, T, 20, 32),
                  head=e(B, T, 10, 32), blk=[e(B, T2, 512), e(B, T2, 1024), e(B, T2, 1024)], tr3=e(B, T2, 512),
                  h=e(B, T2, 128), psum=e(B, (T2 + 3) // 4, 128), gate=e(B, (T2 + SEG_LEN - 1) // SEG_LEN, 32),
                  stats=e(B, 1024), emb=e(B, CAMPPLUS_EMBED))
        if S_pad:
            ws.update(wave=e(B, S_pad), spec=e(B * T, 2 * NBINS), pw=e(B * T, NBINS), melo=e(B * T, NMELS))
        return ws

    def _enqueue(self, ws, with_fbank=False):
        P, B, T, T2 = self.p, ws["B"], ws["T"], ws["T2"]
        lens, lens2 = ws["lens"], ws["lens2"]
        if with_fbank:
            self.fb.enqueue(ws["wave"], ws["S_pad"], lens, B, T, True, ws["spec"], ws["pw"], ws["melo"], ws["feat"], NMELS)
        cv = self._conv
        # FCM head over (time, frequency) rows, 32 channels; every conv k3 pad 1, time stride 1
        k3 = dict(k=(3, 3), pad=(1, 1), in_len=lens, out_len=lens)
        cv(ws["feat"], T * 80, 1, T, 80, 1, P["c1"][0], ws["a80"], T * 80 * 32, 32, T, 80, B, bias=P["c1"][1], relu=True, **k3)
        x, F = ws["a80"], 80
        for layer, (hb, sb, xa, xb) in (("layer1", ("h40", "s40", "x40", "y40")), ("layer2", ("h20", "s20", "x20", "y20"))):
            Fo = F // 2
            for i, out in ((0, xa), (1, xb)):
                p, st = f"head.{layer}.{i}", (2 if i == 0 else 1)
                Fi = F if i == 0 else Fo
                cv(x, T * Fi * 32, 32, T, Fi, 32, P[p + ".c1"][0], ws[hb], T * Fo * 32, 32, T, Fo, B, s=(st, 1), bias=P[p + ".c1"][1],
                   relu=True, **k3)
                if p + ".sc" in P:
                    cv(x, T * Fi * 32, 32, T, Fi, 32, P[p + ".sc"][0], ws[sb], T * Fo * 32, 32, T, Fo, B, s=(st, 1),
                       bias=P[p + ".sc"][1], in_len=lens, out_len=lens)
                    res = ws[sb]
                else:
                    res = x
                cv(ws[hb], T * Fo * 32, 32, T, Fo, 32, P[p + ".c2"][0], ws[out], T * Fo * 32, 32, T, Fo, B, bias=P[p + ".c2"][1],
                   res=res, relu=True, **k3)
                x = ws[out]
            F = Fo
        cv(x, T * 20 * 32, 32, T, 20, 32, P["c2"][0], ws["head"], T * 10 * 32, 32, T, 10, B, s=(2, 1), bias=P["c2"][1], relu=True,
           **k3)
        # TDNN: (T, 320) rows -> block1 columns [0, 128)
        blk = ws["blk"]
        widths = (512, 1024, 1024)
        cv(ws["head"], T * 320, 320, T, 1, 320, P["tdnn"][0], blk[0], T2 * 512, 512, T2, 1, B, k=(1, 5), s=(1, 2), pad=(0, 2),
           bias=P["tdnn"][1], relu=True, in_len=lens, out_len=lens2)
        ch = 128
        h, psum, gate = ws["h"], ws["psum"], ws["gate"]
        psum_bs, gate_bs = psum.stride(0), gate.stride(0)
        st = L.stream_ptr()
        for bi, (n, dil) in enumerate(CAMPPLUS_BLOCKS, 1):
            X, Cb = blk[bi - 1], widths[bi - 1]
            for i in range(n):
                q = P[f"xvector.block{bi}.tdnnd{i + 1}"]
                cin = ch + 32 * i
                cv(X, T2 * Cb, Cb, T2, 1, cin, q["w1"], h, T2 * 128, 128, T2, 1, B, pre=q["pre"], bias=q["b1"], relu=True,
                   in_len=lens2, out_len=lens2, psum=psum, psum_bs=psum_bs)
                _check(L.lib().cv_spk_cam_gate(psum.data_ptr(), psum_bs, lens2.data_ptr(), B, T2, SEG_LEN, q["g1"].data_ptr(),
                                               q["gb1"].data_ptr(), q["g2"].data_ptr(), q["gb2"].data_ptr(), gate.data_ptr(), gate_bs, st),
                       "cv_spk_cam_gate")
                cv(h, T2 * 128, 128, T2, 1, 128, q["wl"], X, T2 * Cb, Cb, T2, 1, B, k=(1, 3), pad=(0, dil), dt=dil, in_len=lens2,
                   out_len=lens2, gate=gate, gate_bs=gate_bs, y_off=cin)
            ch += 32 * n
            t = P[f"transit{bi}"]
            Y, Cy = (blk[bi], widths[bi]) if bi < 3 else (ws["tr3"], 512)
            cv(X, T2 * Cb, Cb, T2, 1, Cb, t["w"], Y, T2 * Cy, Cy, T2, 1, B, pre=t["pre"], in_len=lens2, out_len=lens2)
            ch //= 2
        sc, sh = P["out_nl"]
        _check(L.lib().cv_spk_stats_pool(ws["tr3"].data_ptr(), T2 * 512, 512, lens2.data_ptr(), B, T2, 512, sc.data_ptr(), sh.data_ptr(),
                                         ws["stats"].data_ptr(), 1024, st), "cv_spk_stats_pool")
        cv(ws["stats"], 1024, 1024, 1, 1, 1024, P["dense"][0], ws["emb"], CAMPPLUS_EMBED, CAMPPLUS_EMBED, 1, 1, B, bias=P["dense"][1])

    def _run(self, key, B, T, frames, fill, S_pad=0, graph=True):
        if self.p is None:
            raise RuntimeError("load_state_dict first")
        if min(frames) < 3:
            raise ValueError(f"{min(frames)} fbank frames give fewer than 2 TDNN frames: the unbiased std is undefined")
        ops.bound_cache(self._ws, key, self._graphs)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = self._workspace(B, T, S_pad)
        fill(ws)
        ws["lens"].copy_(torch.tensor(frames, dtype=torch.int32))
        ws["lens2"].copy_(torch.tensor([tdnn_frames(f) for f in frames], dtype=torch.int32))
        if graph:
            g = self._graphs.get(key)
            if g is None:
                g = self._graphs[key] = ops.Graph().capture(lambda: self._enqueue(ws, with_fbank=S_pad > 0))
            g.launch()
        else:
            self._enqueue(ws, with_fbank=S_pad > 0)
        return ws["emb"].clone()

    @torch.no_grad()
    def embed_frames_last(self, feat, lengths=None, graph=True):
        """feat (B, T, 80) (the ONNX session's layout) -> (B, 192)."""
        feat = torch.as_tensor(feat)
        if feat.dim() != 3 or feat.shape[2] != NMELS:
            raise ValueError(f"expected (B, T, {NMELS}), got {tuple(feat.shape)}")
        B, T, _ = feat.shape
        frames = [T] * B if lengths is None else [int(v) for v in lengths]
        if any(f > T or f < 0 for f in frames):
            raise ValueError("a length exceeds the padded frame count")

        def fill(ws):
            ws["feat"].copy_(feat.to(self.device, torch.float32))
        return self._run(("feat", B, T), B, T, frames, fill, graph=graph)

    @torch.no_grad()
    def __call__(self, x, lengths=None, graph=True):
        """x (B, 80, T) as the reference module takes it -> (B, 192)."""
        x = torch.as_tensor(x)
        if x.dim() != 3 or x.shape[1] != NMELS:
            raise ValueError(f"expected (B, {NMELS}, T), got {tuple(x.shape)}")
        return self.embed_frames_last(x.transpose(1, 2), lengths, graph=graph)

    @torch.no_grad()
    def extract_spk_embedding(self, speech_16k, graph=True):
        """frontend.py:91-100 end to end: (1, S) / (S,) 16 kHz waveform -> (1, 192) on the device; a list of waveforms (or a (B, S)
        tensor) -> (B, 192), one row per prompt."""
        buf, S = _pad_waves(speech_16k)
        B, S_pad = buf.shape
        T = num_frames(S_pad)
        frames = [num_frames(s) for s in S]

        def fill(ws):
            ws["wave"].copy_(buf)
        return self._run(("wave", B, S_pad), B, T, frames, fill, S_pad=S_pad, graph=graph)

    def num_launches(self, key):
        g = self._graphs.get(key)
        return None if g is None else g.num_launches


def extract_spk_embedding(model: CAMPPlus, speech_16k):
    """CosyVoiceFrontEnd._extract_spk_embedding with ``model`` in place of the onnxruntime session."""
    return model.extract_spk_embedding(speech_16k)


class _NodeArg:
    def __init__(self, name, shape):
        self.name, self.shape, self.type = name, shape, "tensor(float)"


class CampplusSession:
    """Drop-in for ``CosyVoiceFrontEnd.campplus_session`` (frontend.py:49-52, 97-99): ``run(None, {name: (B, T, 80) float32})`` ->
    ``[ndarray (B, 192) float32]``."""

    def __init__(self, model: CAMPPlus, input_name="input"):
        self.model = model
        self._inputs = [_NodeArg(input_name, ["B", "T", NMELS])]

    def get_inputs(self):
        return self._inputs

    def get_outputs(self):
        return [_NodeArg("output", ["B", CAMPPLUS_EMBED])]

    def run(self, output_names, input_feed, run_options=None):
        name = self._inputs[0].name
        if set(input_feed) != {name}:
            raise ValueError(f"expected one input named {name!r}, got {sorted(input_feed)}")
        x = np.ascontiguousarray(input_feed[name], dtype=np.float32)
        return [self.model.embed_frames_last(torch.from_numpy(x)).cpu().numpy()]
