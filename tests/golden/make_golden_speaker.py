#!/usr/bin/env python3
"""Mint tests/golden/campplus_*.npz by running the REFERENCE's own CAMPPlus (cosyvoice/speaker/CAMPPlus.py:384-451, configured
as speaker/speaker_encoder.py:154-159) on the key-seeded weights of cosyvoice_amd.weights.campplus_state_dict.

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_speaker.py

Imports go through make_golden.install_stubs() (name-only stand-ins for absent third-party modules; torchaudio.compliance.kaldi
among them, so the fbank INPUT is the CPU restatement tests/speaker_ref.kaldi_fbank of a synthetic prompt, minus its mean).
Fixtures: campplus_t150.npz / campplus_t998.npz = {feat (1, 80, T), embedding (1, 192)}; campplus_keys.npz = the reference
module's state-dict keys and shapes."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF = "/root/reference"


def main():
    import make_golden
    import speaker_ref
    from cosyvoice_amd.weights import campplus_state_dict
    make_golden.install_stubs()
    sys.path.insert(0, REF)
    from cosyvoice.speaker.CAMPPlus import CAMPPlus
    torch.manual_seed(0)
    model = CAMPPlus(feat_dim=80, embedding_size=192).eval()
    ref_sd = model.state_dict()
    sd = campplus_state_dict()
    model.load_state_dict(sd)
    keys = list(ref_sd.keys())
    np.savez_compressed(os.path.join(HERE, "campplus_keys.npz"), keys=np.array(keys),
                        shapes=np.array([json.dumps(list(ref_sd[k].shape)) for k in keys]))
    for T, seed in ((150, 1), (998, 2)):
        wave = speaker_ref.test_signal(160 * (T - 1) + 400, seed=seed)
        feat = speaker_ref.kaldi_fbank(wave)
        assert feat.shape[0] == T
        feat = (feat - feat.mean(dim=0, keepdim=True)).T.unsqueeze(0).float().contiguous()
        with torch.no_grad():
            emb = model(feat)
        np.savez_compressed(os.path.join(HERE, f"campplus_t{T}.npz"), feat=feat.numpy(), embedding=emb.numpy())
        print(f"campplus_t{T}: embedding std {emb.std().item():.4f}  |max| {emb.abs().max().item():.4f}")


if __name__ == "__main__":
    main()
