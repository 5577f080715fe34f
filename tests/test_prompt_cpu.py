"""CPU: the prompt front end's host side — the blocked interpolation matrix of frontend.Resample applied in numpy against the
conv1d restatement (tests/prompt_ref.py), the restatement itself against an analytic sine (torchaudio is absent: an external check
of what everything else is compared with), the model_input / tts_batch dict assembly against the restatement of
cli/frontend.py:141-195, and the size cap of the interpolation matrix."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as P  # noqa: E402

RATES = [(16000, 24000), (24000, 16000), (44100, 16000), (48000, 16000), (22050, 24000), (16000, 22050)]


def _apply_weights(rs, x):
    """What the device launch computes, in float64: rows of a strided view of the zero-padded signal times W^T."""
    W = rs.weights()
    N, K = W.shape
    assert W.dtype == np.float64 and (N, K) == (rs.N, rs.K) and K % 4 == 0 and rs.lda % 4 == 0
    n_out = rs.out_len(x.size)
    M = -(-n_out // N)
    xp = np.zeros((M - 1) * rs.lda + K)
    xp[rs.width:rs.width + x.size] = x
    A = np.lib.stride_tricks.as_strided(xp, (M, K), (8 * rs.lda, 8))
    return (A @ W.T).reshape(-1)[:n_out]


@pytest.mark.parametrize("orig,new", RATES)
def test_blocked_weights_match_conv1d_restatement(orig, new):
    from cosyvoice_amd.frontend import Resample
    rs = Resample(orig, new)
    go = rs.g * rs.o
    assert go == rs.lda and rs.g == 4 // math.gcd(rs.o, 4)
    assert rs.weights() is rs.weights()                                   # built once
    rng = np.random.default_rng(orig + new)
    for S in sorted({1, 2, go - 1, go, go + 1, 4801}):
        x = rng.uniform(-1, 1, S)
        ref = P.sinc_resample(torch.from_numpy(x), orig, new).numpy()
        got = _apply_weights(rs, x)
        assert got.shape == ref.shape == (math.ceil(new * S / orig),), S
        assert np.abs(got - ref).max() <= 1e-12, S


def test_geometry_of_the_two_documented_cases():
    from cosyvoice_amd.frontend import Resample
    a, b = Resample(16000, 24000), Resample(44100, 16000)
    assert (a.g, a.lda, a.N, a.K) == (2, 4, 6, 20)
    assert (b.g, b.lda, b.N, b.K) == (4, 1764, 640, 1800)


@pytest.mark.parametrize("orig,new", RATES)
def test_restatement_resamples_a_sine(orig, new):
    S, f = 4801, 440.0
    x = torch.sin(2 * math.pi * f * torch.arange(S, dtype=torch.float64) / orig)
    y = P.sinc_resample(x, orig, new)
    assert y.numel() == math.ceil(new * S / orig)
    want = torch.sin(2 * math.pi * f * torch.arange(y.numel(), dtype=torch.float64) / new)
    err = (y - want)[200:-200].abs().max().item()
    print(f"sine {orig}->{new}: {err:.3e}")
    assert err <= 1e-3


def test_weight_cap_raises():
    from cosyvoice_amd.frontend import Resample
    with pytest.raises(ValueError):
        Resample(16001, 16000)
    Resample(16000, 16000)                                                # the identity needs no matrix at all


def _parts(T, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(text=torch.randint(0, 500, (1, 7), generator=g, dtype=torch.int32),
                prompt_text=torch.randint(0, 500, (1, 4), generator=g, dtype=torch.int32),
                speech_feat=torch.randn(1, T, 80, generator=g),
                speech_token=torch.randint(0, 6561, (1, N), generator=g, dtype=torch.int32),
                embedding=torch.randn(1, 192, generator=g))


def _same(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("T,N", [(50, 30), (61, 30), (60, 30), (7, 30), (50, 0)])
def test_zero_shot_dict_trims_at_24k(T, N):
    from cosyvoice_amd import frontend as F
    p = _parts(T, N)
    d = F.assemble_zero_shot(resample_rate=24000, **p)
    _same(d, P.zero_shot(resample_rate=24000, **p))
    assert tuple(d.keys()) == P.ZERO_SHOT_KEYS and len(d) == 12
    n = min(T // 2, N)
    assert d["prompt_speech_feat"].shape == (1, 2 * n, 80) and d["flow_prompt_speech_token"].shape == (1, n)
    assert torch.equal(d["prompt_speech_feat"], p["speech_feat"][:, :2 * n])
    assert torch.equal(d["llm_prompt_speech_token"], p["speech_token"][:, :n])
    for k, v in (("prompt_speech_feat_len", 2 * n), ("flow_prompt_speech_token_len", n), ("llm_prompt_speech_token_len", n),
                 ("text_len", 7), ("prompt_text_len", 4)):
        assert d[k].dtype == torch.int32 and d[k].shape == (1,) and int(d[k]) == v, k
    assert d["llm_embedding"] is d["flow_embedding"]


def test_zero_shot_dict_keeps_everything_at_22050():
    from cosyvoice_amd import frontend as F
    p = _parts(86, 30)
    d = F.assemble_zero_shot(resample_rate=22050, **p)
    _same(d, P.zero_shot(resample_rate=22050, **p))
    assert d["prompt_speech_feat"].shape == (1, 86, 80) and int(d["prompt_speech_feat_len"]) == 86
    assert d["flow_prompt_speech_token"].shape == (1, 30) and int(d["flow_prompt_speech_token_len"]) == 30


def test_other_modes_key_sets_and_values():
    from cosyvoice_amd import frontend as F
    p = _parts(51, 40, seed=3)
    feat, tok, emb = p["speech_feat"], p["speech_token"], p["embedding"]
    d = F.assemble_cross_lingual(p["text"], feat, tok, emb, 24000)
    _same(d, P.cross_lingual(p["text"], feat, tok, emb, 24000))
    assert tuple(d.keys()) == P.CROSS_LINGUAL_KEYS and len(d) == 8
    d = F.assemble_instruct2(p["text"], p["prompt_text"], feat, tok, emb, 24000)
    _same(d, P.instruct2(p["text"], p["prompt_text"], feat, tok, emb, 24000))
    assert tuple(d.keys()) == P.INSTRUCT2_KEYS and len(d) == 10
    src = torch.arange(17, dtype=torch.int32)[None]
    d = F.assemble_vc(src, feat, tok, emb)
    _same(d, P.vc(src, feat, tok, emb))
    assert tuple(d.keys()) == P.VC_KEYS and len(d) == 7
    assert d["prompt_speech_feat"].shape == (1, 51, 80) and int(d["flow_prompt_speech_token_len"]) == 40   # no trim in vc


def test_batch_dict_has_tts_batch_parameter_names_and_stacks_equal_prompts():
    import inspect
    from cosyvoice_amd import frontend as F
    from cosyvoice_amd.model import CosyVoice2Model
    ps = [_parts(50, 30, seed=1), _parts(32, 20, seed=2)]
    emb = torch.cat([p["embedding"] for p in ps])
    args = ([p["text"] for p in ps], [p["prompt_text"] for p in ps], [p["speech_feat"] for p in ps], [p["speech_token"][0] for p in ps], emb)
    d = F.assemble_batch(*args)
    params = [k for k in inspect.signature(CosyVoice2Model.tts_batch).parameters if k not in ("self", "forced", "to_host")]
    assert list(d.keys()) == params
    assert isinstance(d["flow_prompt_speech_tokens"], list) and isinstance(d["prompt_speech_feats"], list)
    for b, (p, n) in enumerate(zip(ps, (25, 16))):
        ref = P.zero_shot(p["text"], p["prompt_text"], p["speech_feat"], p["speech_token"], p["embedding"], 24000)
        assert torch.equal(d["flow_prompt_speech_tokens"][b], ref["flow_prompt_speech_token"][0]) and d["flow_prompt_speech_tokens"][b].shape == (n,)
        assert torch.equal(d["prompt_speech_feats"][b], ref["prompt_speech_feat"][0]) and d["prompt_speech_feats"][b].shape == (2 * n, 80)
        assert torch.equal(d["llm_prompt_speech_tokens"][b], ref["llm_prompt_speech_token"])
        assert torch.equal(d["texts"][b], p["text"]) and torch.equal(d["prompt_texts"][b], p["prompt_text"])
    assert d["flow_embeddings"].shape == (2, 192)
    # prompts that trim to the same length: stacked tensors, the equal-shape flow pass
    ps = [_parts(50, 30, seed=1), _parts(51, 25, seed=2)]
    d = F.assemble_batch([p["text"] for p in ps], [p["prompt_text"] for p in ps], [p["speech_feat"] for p in ps],
                         [p["speech_token"] for p in ps], emb)
    assert d["flow_prompt_speech_tokens"].shape == (2, 25) and d["prompt_speech_feats"].shape == (2, 50, 80)
    assert torch.equal(d["prompt_speech_feats"][1], ps[1]["speech_feat"][0, :50])


def test_lengths_follow_from_sample_counts():
    from cosyvoice_amd.frontend import Resample
    for orig, new in RATES:
        rs = Resample(orig, new)
        for S in (1, 2, 511, 4801, 16037, 480000):
            assert rs.out_len(S) == P.resample_len(S, orig, new) == math.ceil(new * S / orig)
    assert P.mel_frames(P.resample_len(16037, 16000, 24000)) == 50
    assert P.mel_frames(P.resample_len(16037, 16000, 22050), n_fft=1024, hop=256) == 86
