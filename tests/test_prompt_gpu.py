"""GPU: the prompt front end on the device — frontend.Resample (one exact-f32 cv_gemm over a strided view of the signal) against
the float64 restatement (tests/prompt_ref.py), its ragged batches and MelSpectrogram.ragged against their batch-1 runs (bit-identical),
PromptFrontEnd's model_input dict against the restated chain resample -> oracle mel -> trim and the CPU speaker chain, and
PromptFrontEnd.batch driving CosyVoice2Model.tts_batch with prompts of different lengths."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as P  # noqa: E402
import speaker_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _tile_edge_lengths(go):
    return [1, go - 1, go + 1, 64 * go - 1, 64 * go + 1, 128 * go + 1, 4801]


@pytest.mark.parametrize("orig,new,lengths", [(16000, 24000, _tile_edge_lengths(4)), (24000, 16000, _tile_edge_lengths(12)),
                                              (48000, 16000, _tile_edge_lengths(12)), (44100, 16000, [1763, 1765, 64 * 1764 + 1])])
def test_resample_matches_fp64_restatement(orig, new, lengths):
    """Bound: 4 * e32 + 1e-7, e32 = L-inf of the float32 CPU restatement against float64 on the same input (the MFMA sums up to 475
    non-zero taps in another order than conv1d)."""
    from cosyvoice_amd.frontend import Resample
    rs = Resample(orig, new)
    assert rs.lda == (4 if orig == 16000 else 1764 if orig == 44100 else 12)
    g = torch.Generator().manual_seed(orig + new)
    for S in lengths:
        x = torch.rand(S, generator=g, dtype=torch.float64).mul_(2).sub_(1).float()
        ref = P.sinc_resample(x.double(), orig, new)
        e32 = (P.sinc_resample(x, orig, new, dtype=torch.float32).double() - ref).abs().max().item()
        y, lens = rs(x)
        assert lens == [ref.numel()] and y.shape == (1, ref.numel()) and y.dtype == torch.float32 and y.is_cuda
        err = (y[0].cpu().double() - ref).abs().max().item()
        print(f"resample {orig}->{new} S={S}: gpu err {err:.3e}, fp32 cpu err {e32:.3e}")
        assert err <= 4 * e32 + 1e-7, (S, err, e32)


def test_resample_ragged_rows_bit_identical():
    from cosyvoice_amd.frontend import Resample
    rs = Resample(16000, 24000)
    g = torch.Generator().manual_seed(5)
    waves = [torch.rand(S, generator=g) * 2 - 1 for S in (4801, 511, 9, 1)]
    y, lens = rs(waves)
    assert lens == [7202, 767, 14, 2] and y.shape == (4, 7202)
    for b, w in enumerate(waves):
        alone, n = rs(w)
        assert n == [lens[b]] and torch.equal(y[b, :lens[b]], alone[0]), b
        assert torch.all(y[b, lens[b]:] == 0)
    same, n = Resample(16000, 16000)(waves[1])
    assert n == [511] and torch.equal(same[0].cpu(), waves[1])
    y2, lens2 = rs(torch.stack([waves[0], waves[0].flip(0)]))              # (B, S) tensor input
    assert lens2 == [7202, 7202] and torch.equal(y2[0], y[0])


def test_mel_ragged_rows_bit_identical_and_match_oracle():
    from cosyvoice_amd.frontend import MelSpectrogram, slaney_mel_basis
    from oracle import frontend as ofe
    fe = MelSpectrogram()
    basis = torch.from_numpy(slaney_mel_basis(24000, 1920, 80, 0, 8000))
    g = torch.Generator().manual_seed(11)
    waves = [(torch.randn(S, generator=g) * 0.3).clamp(-1, 1) for S in (721, 1921, 4801, 24000)]
    mel, frames = fe.ragged(waves)
    assert frames == [P.mel_frames(w.numel()) for w in waves] == [1, 4, 10, 50]
    assert mel.shape == (4, 80, 50) and mel.dtype == torch.float32
    for b, w in enumerate(waves):
        alone = fe(w.cuda())
        assert alone.shape == (1, 80, frames[b])
        assert torch.equal(mel[b, :, :frames[b]], alone[0]), b
        assert torch.all(mel[b, :, frames[b]:] == 0)
        ref = ofe.mel_spectrogram(w[None], basis)
        assert (mel[b, :, :frames[b]].cpu() - ref[0]).abs().max().item() < 1e-3
    # the (buf, lens) form, with junk behind the rows' ends
    buf = torch.full((4, 24000), 1e4)
    for b, w in enumerate(waves):
        buf[b, :w.numel()] = w
    mel2, frames2 = fe.ragged((buf.cuda(), [w.numel() for w in waves]))
    assert frames2 == frames and torch.equal(mel2, mel)
    with pytest.raises(ValueError):
        fe.ragged([waves[2], torch.zeros(720)])


@pytest.fixture(scope="module")
def campplus():
    from cosyvoice_amd.speaker import CAMPPlus
    from cosyvoice_amd.weights import campplus_state_dict
    return CAMPPlus().load_state_dict(campplus_state_dict())


def test_frontend_zero_shot_matches_restated_chain(campplus):
    from cosyvoice_amd.frontend import MelSpectrogram, PromptFrontEnd, slaney_mel_basis
    from cosyvoice_amd.weights import campplus_state_dict
    w = R.test_signal(16037)
    g = torch.Generator().manual_seed(2)
    text = torch.randint(0, 500, (1, 9), generator=g, dtype=torch.int32)
    ptext = torch.randint(0, 500, (1, 5), generator=g, dtype=torch.int32)
    tok = torch.randint(0, 6561, (1, 30), generator=g, dtype=torch.int32)
    emb_ref = R.extract_spk_embedding(campplus_state_dict(), w)
    fe = PromptFrontEnd(MelSpectrogram(), campplus)
    d = fe.frontend_zero_shot(text, ptext, w.unsqueeze(0), tok, 24000)
    feat_ref = P.prompt_feat(w, 24000, torch.from_numpy(slaney_mel_basis(24000, 1920, 80, 0, 8000)))
    ref = P.zero_shot(text, ptext, feat_ref, tok, emb_ref, 24000)
    assert tuple(d.keys()) == P.ZERO_SHOT_KEYS
    assert feat_ref.shape == (1, 50, 80) and d["prompt_speech_feat"].shape == ref["prompt_speech_feat"].shape == (1, 50, 80)
    assert d["prompt_speech_feat"].is_cuda and d["flow_embedding"].is_cuda
    assert (d["prompt_speech_feat"].cpu() - ref["prompt_speech_feat"]).abs().max().item() <= 1e-3
    assert (d["flow_embedding"].cpu() - emb_ref).abs().max().item() <= 1e-3 and d["flow_embedding"].shape == (1, 192)
    for k in ("text", "text_len", "prompt_text", "prompt_text_len", "llm_prompt_speech_token", "llm_prompt_speech_token_len",
              "flow_prompt_speech_token", "flow_prompt_speech_token_len", "prompt_speech_feat_len"):
        assert d[k].dtype == ref[k].dtype and torch.equal(d[k].cpu(), ref[k]), k
    assert int(d["flow_prompt_speech_token_len"]) == 25 and int(d["prompt_speech_feat_len"]) == 50
    # the other modes: the same tensors under fewer keys
    assert tuple(fe.frontend_cross_lingual(text, w, tok, 24000).keys()) == P.CROSS_LINGUAL_KEYS
    assert tuple(fe.frontend_instruct2(text, ptext, w, tok, 24000).keys()) == P.INSTRUCT2_KEYS
    v = fe.frontend_vc(tok[:, :11], w, tok, 24000)
    assert tuple(v.keys()) == P.VC_KEYS and v["prompt_speech_feat"].shape == (1, 50, 80) and int(v["flow_prompt_speech_token_len"]) == 30
    assert torch.equal(v["prompt_speech_feat"], d["prompt_speech_feat"])
    # v1 rate: no trim, the frame count of the 22.05 kHz mel of the resampled prompt
    fe1 = PromptFrontEnd(MelSpectrogram(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000), campplus)
    d1 = fe1.frontend_zero_shot(text, ptext, w, tok, 22050)
    T1 = P.mel_frames(P.resample_len(16037, 16000, 22050), n_fft=1024, hop=256)
    assert T1 == 86 and d1["prompt_speech_feat"].shape == (1, T1, 80) and int(d1["prompt_speech_feat_len"]) == T1
    assert torch.equal(d1["flow_prompt_speech_token"], tok) and int(d1["flow_prompt_speech_token_len"]) == 30


def test_batch_drives_tts_batch_with_prompts_of_different_lengths(campplus):
    import test_model_gpu as TM
    from cosyvoice_amd.frontend import MelSpectrogram, PromptFrontEnd
    m, lc, fc, hc = TM._model()
    fe = PromptFrontEnd(MelSpectrogram(), campplus)
    g = torch.Generator().manual_seed(17)
    texts = [torch.randint(0, lc.vocab_size, (1, 6), generator=g, dtype=torch.int32) for _ in range(2)]
    ptexts = [torch.randint(0, lc.vocab_size, (1, 4), generator=g, dtype=torch.int32) for _ in range(2)]
    forced = [torch.randint(0, lc.speech_token_size, (14,), generator=g).tolist() for _ in range(2)]
    toks = [torch.randint(0, lc.speech_token_size, (n,), generator=g, dtype=torch.int32) for n in (30, 20)]
    waves = [R.test_signal(16037, seed=1), R.test_signal(10240, seed=2)]
    d = fe.batch(texts, ptexts, waves, toks)
    assert isinstance(d["flow_prompt_speech_tokens"], list) and [t.numel() for t in d["flow_prompt_speech_tokens"]] == [25, 16]
    assert [tuple(f.shape) for f in d["prompt_speech_feats"]] == [(50, 80), (32, 80)] and d["flow_embeddings"].shape == (2, 192)
    calls, orig = [], m.flow.inference_ragged

    def rec(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    m.flow.inference_ragged = rec
    torch.manual_seed(0)
    wavs = m.tts_batch(**d, forced=forced)
    m.flow.inference_ragged = orig
    assert calls == [1]                                                     # equal generated lengths, ragged prompts: the ragged flow pass
    assert isinstance(wavs, list) and len(wavs) == 2
    for w in wavs:
        assert w.shape == (14 * 2 * hc.total_upsample,) and torch.isfinite(w).all()
    # every utterance's flow mel equals its own batch-1 equal-shape run
    tok = torch.tensor(forced, dtype=torch.int32)
    mels = m.flow.inference_ragged(list(tok), d["flow_prompt_speech_tokens"], d["prompt_speech_feats"], d["flow_embeddings"])
    for b in range(2):
        mel_1 = m.flow.inference_batch(tok[b:b + 1], d["flow_prompt_speech_tokens"][b][None], d["prompt_speech_feats"][b][None],
                                       d["flow_embeddings"][b:b + 1])
        assert mels[b].shape == mel_1[0].shape == (80, 28)
        assert (mel_1[0] - mels[b]).abs().max().item() < 1e-4
    # the single-prompt front end gives the same rows as the batch
    one = fe.frontend_zero_shot(texts[1], ptexts[1], waves[1], toks[1], 24000)
    assert torch.equal(one["prompt_speech_feat"][0], d["prompt_speech_feats"][1]) and torch.equal(one["flow_embedding"][0], d["flow_embeddings"][1])
    # two prompts of equal length: stacked tensors, the tensor path, bit-identical to passing those tensors by hand
    waves = [R.test_signal(16037, seed=1), R.test_signal(16037, seed=3)]
    d = fe.batch(texts, ptexts, waves, [toks[0], toks[0].flip(0)])
    assert d["flow_prompt_speech_tokens"].shape == (2, 25) and d["prompt_speech_feats"].shape == (2, 50, 80)
    m.flow.inference_ragged = rec
    torch.manual_seed(0)
    wav = m.tts_batch(**d, forced=forced)
    m.flow.inference_ragged = orig
    assert calls == [1] and isinstance(wav, torch.Tensor) and wav.shape == (2, 14 * 2 * hc.total_upsample)
    torch.manual_seed(0)
    by_hand = m.tts_batch(d["texts"], d["prompt_texts"], d["llm_prompt_speech_tokens"], d["flow_prompt_speech_tokens"],
                          d["prompt_speech_feats"], d["flow_embeddings"], forced=forced)
    assert torch.equal(wav, by_hand) and torch.isfinite(wav).all()
    m.close()
