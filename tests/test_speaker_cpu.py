"""CPU: the speaker-embedding restatement (tests/speaker_ref.py) against the reference CAMPPlus goldens, the key-seeded weights'
key list, closed-form invariants of the Kaldi fbank, and argument validation of the cv_spk_* entry points."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speaker_ref as R  # noqa: E402


def test_restatement_matches_reference_goldens(golden_dir):
    from cosyvoice_amd.weights import campplus_state_dict
    sd = campplus_state_dict()
    for T in (150, 998):
        z = np.load(os.path.join(golden_dir, f"campplus_t{T}.npz"))
        assert z["feat"].shape == (1, 80, T)
        e = R.campplus(sd, torch.from_numpy(z["feat"]))
        assert (e - torch.from_numpy(z["embedding"])).abs().max().item() <= 1e-5


def test_state_dict_has_reference_keys_and_shapes(golden_dir):
    from cosyvoice_amd.weights import campplus_state_dict
    z = np.load(os.path.join(golden_dir, "campplus_keys.npz"))
    sd = campplus_state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    assert len(sd) == 937
    for k, s in zip(z["keys"], z["shapes"]):
        assert list(sd[str(k)].shape) == json.loads(str(s)), k
    assert sum(v.numel() for k, v in sd.items() if not k.rsplit(".", 1)[1].startswith(("running_", "num_batches"))) == 6848544


def test_fbank_frame_count():
    for S, T in ((399, 0), (400, 1), (559, 1), (560, 2), (16000, 98), (160000, 998), (480000, 2998)):
        assert R.num_frames(S) == T
        if T:
            assert R.kaldi_fbank(torch.zeros(S) + 0.1).shape == (T, 80)


def test_fbank_pure_tone_lands_in_nearest_mel_bin():
    banks = R.mel_banks()
    lo, hi = R.mel_scale(20.0), R.mel_scale(8000.0)
    delta = (hi - lo) / 81
    centres_mel = lo + (torch.arange(80, dtype=torch.float64) + 1) * delta
    for f in (300.0, 1000.0, 2500.0, 6000.0):
        t = torch.arange(16000, dtype=torch.float64) / 16000
        feat = R.kaldi_fbank(0.5 * torch.sin(2 * math.pi * f * t))
        assert int(feat.mean(0).argmax()) == int((centres_mel - R.mel_scale(f)).abs().argmin()), f
    assert banks[:, 256].abs().max() == 0.0          # the Nyquist bin has zero weight


def test_fbank_constant_signal_is_log_flt_epsilon():
    feat = R.kaldi_fbank(torch.full((4000,), 0.25))
    assert torch.all(feat == math.log(float(np.finfo(np.float32).eps)))


def test_window_and_mel_banks_closed_forms():
    from cosyvoice_amd import speaker as S
    i = np.arange(400)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * i / 399)) ** 0.85
    assert np.abs(R.povey().numpy() - win).max() < 1e-15
    assert np.abs(S.povey_window() - win).max() < 1e-15
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)  # noqa: E731
    lo, hi = mel(20.0), mel(8000.0)
    d = (hi - lo) / 81
    fm = mel(np.arange(256) * 31.25)
    for b in (0, 17, 79):
        want = np.maximum(0.0, np.minimum((fm - (lo + b * d)) / d, (lo + (b + 2) * d - fm) / d))
        assert np.abs(R.mel_banks().numpy()[b, :256] - want).max() < 1e-12
    assert np.abs(S.kaldi_mel_banks() - R.mel_banks().numpy()[:, :256]).max() < 1e-12
    # the folded DFT basis (DC removal + pre-emphasis + window + DFT) reproduces the step-by-step power spectrum
    w = R.test_signal(4000).double()
    fr = w.unfold(0, 400, 160)
    spec = fr @ torch.from_numpy(S.fbank_basis()).T
    pw = spec[:, :256] ** 2 + spec[:, 256:] ** 2
    mine = (pw @ torch.from_numpy(S.kaldi_mel_banks()).T).clamp(min=R.FLT_EPSILON).log()
    assert (mine - R.kaldi_fbank(w)).abs().max().item() < 1e-9


def test_speaker_entry_points_return_status_codes_without_a_gpu():
    from cosyvoice_amd import _lib as L
    lib = L.lib()
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(16)
    assert lib.cv_sizeof_spk_conv_params() == ctypes.sizeof(L.SpkConvParams)
    assert lib.cv_spk_power(None, 512, None, 256, 1, 256, null) < 0
    assert lib.cv_spk_power(one, 256, one, 256, 1, 256, null) < 0          # ld_spec < 2 * nbins
    assert lib.cv_spk_log_cmn(one, 80, None, 1, 10, 80, 1, one, 80, null) < 0
    assert lib.cv_spk_log_cmn(one, 80, one, 1, 10, 300, 1, one, 300, null) < 0   # more than 256 bins
    assert lib.cv_spk_conv(None, null) < 0
    p = L.SpkConvParams()
    assert lib.cv_spk_conv(ctypes.byref(p), null) < 0                      # all zero
    p.B, p.T_in, p.F_in, p.cin, p.x, p.ldx, p.x_bs = 1, 8, 1, 24, 16, 24, 192   # cin neither 1 nor a multiple of 16
    p.kf = p.kt = p.sf = p.st = p.dt = 1
    p.w, p.ldw, p.N, p.T_out, p.F_out, p.y, p.ldy = 16, 32, 32, 8, 1, 16, 32
    assert lib.cv_spk_conv(ctypes.byref(p), null) < 0
    p.cin, p.ldx = 32, 32
    p.N = 48                                                                # N % 32
    assert lib.cv_spk_conv(ctypes.byref(p), null) < 0
    p.N, p.psum, p.F_out = 32, 16, 2                                        # psum needs F_out == 1
    assert lib.cv_spk_conv(ctypes.byref(p), null) < 0
    assert lib.cv_spk_cam_gate(one, ctypes.c_int64(1 << 20), one, 1, 250, 98, one, one, one, one, one, ctypes.c_int64(1 << 20),
                               null) < 0                                    # segment length not a multiple of 4
    assert lib.cv_spk_cam_gate(one, ctypes.c_int64(128), one, 1, 250, 100, one, one, one, one, one, ctypes.c_int64(96), null) < 0
    assert lib.cv_spk_stats_pool(one, ctypes.c_int64(512), 512, one, 1, 10, 500, None, None, one, ctypes.c_int64(1000), null) < 0
    assert lib.cv_spk_stats_pool(one, ctypes.c_int64(512), 512, one, 1, 10, 512, one, None, one, ctypes.c_int64(1024), null) < 0
