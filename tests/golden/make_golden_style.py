#!/usr/bin/env python3
"""Mint tests/golden/style_*.npz by running the REFERENCE's own SpeakerEmbedding / SpeakerEmbedding_wo_PostEnc
(cosyvoice/speaker/speaker_encoder.py:119-418) on the key-seeded weights of cosyvoice_amd.weights.speaker_embedding_state_dict.

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_style.py

Stubs: those of make_golden.install_stubs plus name-only stand-ins for torchaudio.functional and librosa.filters.mel (imported by
the reference's modules, never called on this path).  ``torch.stft(..., return_complex=False)`` of mel_processing.py:62 is gone
from current torch: the call is served by view_as_real of the complex result, which is what that flag returned.  The timbre
branch (librosa resampling, Kaldi fbank, CAM++) is not run: its chain is pinned by campplus_*.npz, and the fusion is fed a given
192-d vector.  The posterior noise is drawn from a seeded CPU generator and handed to the reference through torch.randn_like.

The script asserts what the weights' gains are chosen for: the mean entropy of every style self-attention layer lies in
[1, log T - 1] nats and of every style-token layer in [1, log 4096 - 1]."""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

CASES = (("t100", 100 * 300 + 117, 11), ("t300", 300 * 300 + 41, 12))      # name, samples, seed
ROW_IDX = (0, 1, 2, 3, 17, 31, 32, 33, 49, 63, 64, 65, 80, 97, 98, 99)      # frames of m / logs that are stored (all < 100)


def import_reference():
    mg.install_stubs()
    mg._stub("torchaudio.functional")
    lib = mg._stub("librosa")
    lib.filters = mg._stub("librosa.filters", mel=lambda *a, **k: None)
    sys.path.insert(0, mg.REF)
    real_stft = torch.stft

    def stft(*a, return_complex=None, **k):
        out = real_stft(*a, return_complex=True, **k)
        return out if return_complex else torch.view_as_real(out)
    torch.stft = stft
    from cosyvoice.speaker import speaker_encoder as se
    return se


def entropy(p):
    return float(-(p * torch.log(p.clamp_min(1e-38))).sum(-1).mean())


def run_case(model, se, wave, n, seed, post_enc):
    import cosyvoice.speaker.commons as commons
    from cosyvoice.speaker.mel_processing import spectrogram_torch
    spec = spectrogram_torch(wave[:n].unsqueeze(0), 1024, 24000, 300, 1024)
    T = spec.shape[-1]
    assert T == n // 300
    lengths = torch.tensor([n]) // 300
    out = {}
    if post_enc:
        g = torch.Generator().manual_seed(seed)
        noise = torch.randn(1, 512, T, generator=g)
        real = torch.randn_like
        torch.randn_like = lambda t, **k: noise
        try:
            z, m, logs, _ = model.enc_q(spec, lengths, g=None)
        finally:
            torch.randn_like = real
        out.update(m=m[0].t(), logs=logs[0].t(), noise=noise[0])
    else:
        z = model.enc_q(spec.transpose(1, 2)).transpose(1, 2)
    ent_style, ent_gst, hooks = [], [], []
    for att in model.style_encoder.attn_layers:
        hooks.append(att.register_forward_hook(lambda mod, i, o: ent_style.append(entropy(o[1]))))

    def gst_hook(mod, inp, o):
        q, k = mod.W_query(inp[0]), mod.W_key(inp[1])
        hs = mod.num_units // mod.num_heads
        s = torch.stack([q[..., h * hs:(h + 1) * hs] @ k[..., h * hs:(h + 1) * hs].transpose(1, 2) for h in range(mod.num_heads)])
        ent_gst.append(entropy(torch.softmax(s / mod.key_dim ** 0.5, dim=-1)))
    for att in model.gst.attentions:
        hooks.append(att.register_forward_hook(gst_hook))
    mask = commons.sequence_mask(lengths, T).unsqueeze(1)
    style_vec = model.style_encoder(z.transpose(1, 2), mask)
    gst_out = model.gst(style_vec)
    for h in hooks:
        h.remove()
    tg = torch.Generator().manual_seed(seed + 1000)
    timbre = torch.randn(192, generator=tg)
    g_out = model.speaker_adapter(gst_out, timbre.view(1, 1, -1))
    lo, hi_s, hi_g = 1.0, math.log(T) - 1.0, math.log(4096) - 1.0
    assert all(lo <= e <= hi_s for e in ent_style), ("style attention entropy outside the band", ent_style, hi_s)
    assert all(lo <= e <= hi_g for e in ent_gst), ("style-token entropy outside the band", ent_gst, hi_g)
    out.update(style_vec=style_vec[0], gst_out=gst_out[0, 0], g=g_out[0, 0], timbre=timbre, ent_style=torch.tensor(ent_style),
               ent_gst=torch.tensor(ent_gst))
    return out


def main():
    from style_ref import test_signal
    from cosyvoice_amd.weights import speaker_embedding_specs, speaker_embedding_state_dict
    se = import_reference()
    torch.manual_seed(0)
    for post_enc, cls, tag, cases in ((True, se.SpeakerEmbedding, "style", CASES), (False, se.SpeakerEmbedding_wo_PostEnc, "style_wo", CASES[:1])):
        model = cls().eval()
        ref_keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        specs = speaker_embedding_specs(post_enc)
        assert ref_keys == [(k, tuple(s)) for k, s, _, _ in specs], "key order / shapes differ from speaker_embedding_specs()"
        n_params = sum(p.numel() for p in model.parameters())
        model.load_state_dict(speaker_embedding_state_dict(1986, post_enc), strict=True)
        with torch.no_grad():
            for name, n, seed in cases:
                wave = test_signal(n + 300, seed=seed)           # 300 samples behind the utterance: what a too-wide mask would read
                o = run_case(model, se, wave, n, seed, post_enc)
                fx = dict(wave=wave.numpy(), n_samples=np.int64(n), seed=np.int64(seed), n_params=np.int64(n_params),
                          style_vec=o["style_vec"].numpy(), gst_out=o["gst_out"].numpy(), g=o["g"].numpy(), timbre=o["timbre"].numpy(),
                          ent_style=o["ent_style"].numpy(), ent_gst=o["ent_gst"].numpy())
                if post_enc:
                    idx = np.array(ROW_IDX)
                    nz = o["noise"].double()
                    fx.update(row_idx=idx, m_rows=o["m"][idx].numpy(), logs_rows=o["logs"][idx].numpy(),
                              m_absmax=np.float32(o["m"].abs().max()), logs_absmax=np.float32(o["logs"].abs().max()),
                              noise_checksum=np.array([float(nz.sum()), float(nz.pow(2).sum()), float(nz[:, -1].sum())]))
                path = os.path.join(HERE, f"{tag}_{name}.npz")
                np.savez_compressed(path, **fx)
                print(path, os.path.getsize(path), "bytes; style entropies", [round(float(e), 2) for e in o["ent_style"]], "gst",
                      [round(float(e), 2) for e in o["ent_gst"]])
        if post_enc:
            np.savez_compressed(os.path.join(HERE, "style_keys.npz"), keys=json.dumps([[k, list(s)] for k, s in ref_keys]),
                                n_params=np.int64(n_params))


if __name__ == "__main__":
    main()
