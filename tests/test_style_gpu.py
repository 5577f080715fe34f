"""GPU: the 512-d speaker encoder (cosyvoice_amd/style.py, csrc/style.hip) — every kernel against torch fp64 on the CPU with
NaN-poisoned padding, the ragged linear spectrogram, the whole chain stage by stage against the CPU restatement in fp64 and against
the goldens minted from the reference's own modules, the ragged-batch / graph-replay bit-identity contracts, and the
``speaker_encoder`` keyword of PromptFrontEnd."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_ref as R  # noqa: E402

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Tolerances, relative to a stage's own max |value|.  Baseline = tests/style_ref.py in fp32 (the arithmetic of the kernels: every
# product is an exact-f32 MFMA) against the same restatement in fp64 on the committed cases, measured on the CPU, never a GPU
# output:
#                  m        logs     z        style_vec  gst_out  g
#   style_t100     1.64e-6  1.46e-6  8.77e-7  5.68e-7    4.49e-5  2.97e-5
#   style_t300     1.93e-6  1.57e-6  6.28e-7  4.61e-7    1.12e-5  6.08e-6
#   style_wo_t100  -        -        1.15e-6  8.68e-7    2.62e-5  2.01e-5
# (the style-token softmaxes are sharp, entropy 2.6-4.5 of 8.3 nats: they amplify the error of the style vector ~50x.)
# The constants are MARGIN = 8 x the baseline of the case (a different tiling reorders sums of up to 2560 terms).  The reference's own
# fp32 (the goldens) sits at 0.4-1.2 x the baseline.  Every injected fault of test_style_cpu.py moves its stage by at least
# 1.9 x the constant (the 4095-token fault on style_wo_t100: 4.06e-4 against 2.10e-4), all others by 5 x and more.
MARGIN = 8.0
BASELINE = {
    "style_t100": {"m": 1.64e-6, "logs": 1.46e-6, "z": 8.77e-7, "style_vec": 5.68e-7, "gst_out": 4.49e-5, "g": 2.97e-5},
    "style_t300": {"m": 1.93e-6, "logs": 1.57e-6, "z": 6.28e-7, "style_vec": 4.61e-7, "gst_out": 1.12e-5, "g": 6.08e-6},
    "style_wo_t100": {"z": 1.15e-6, "style_vec": 8.68e-7, "gst_out": 2.62e-5, "g": 2.01e-5},
}
TOL = {case: {k: MARGIN * v for k, v in d.items()} for case, d in BASELINE.items()}


def load_case(tag):
    fx = np.load(os.path.join(GOLDEN, tag + ".npz"))
    n, seed = int(fx["n_samples"]), int(fx["seed"])
    post = "m_rows" in fx.files
    noise = torch.randn(1, 512, n // 300, generator=torch.Generator().manual_seed(seed))[0] if post else None
    return dict(fx=fx, n=n, wave=torch.from_numpy(fx["wave"]), timbre=torch.from_numpy(fx["timbre"]), noise=noise, post=post)


def rel_err(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((torch.as_tensor(got).double().cpu() - ref).abs().max() / ref.abs().max())


def op_tol(ref32, ref64):
    """Per-kernel tolerance by the same rule: 8 x the error of the fp32 CPU op against fp64 on these inputs, relative to max |ref|."""
    return MARGIN * float((ref32.double() - ref64).abs().max() / ref64.abs().max())


def nan_buf(*shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.fixture(scope="module")
def sd():
    from cosyvoice_amd.weights import speaker_embedding_state_dict
    return speaker_embedding_state_dict(1986)


@pytest.fixture(scope="module")
def model(sd):
    from cosyvoice_amd.style import SpeakerEmbedding
    return SpeakerEmbedding().load_state_dict(sd)


@pytest.fixture(scope="module")
def model_wo():
    from cosyvoice_amd.style import SpeakerEmbeddingWoPostEnc
    from cosyvoice_amd.weights import speaker_embedding_state_dict
    return SpeakerEmbeddingWoPostEnc().load_state_dict(speaker_embedding_state_dict(1986, post_enc=False))


LENS = [(257, 65, 7), (64,), (63,), (300,)]


def _ragged(lens, C, g, scale=1.0):
    """(B, T + 3 rows of slack, C) with NaN past every length and in the slack; the CPU copy keeps the valid rows only."""
    B, T = len(lens), max(lens)
    x = torch.full((B, T + 3, C), float("nan"))
    rows = [torch.randn(n, C, generator=g) * scale for n in lens]
    for b, r in enumerate(rows):
        x[b, :r.shape[0]] = r
    return x, rows


# ------------------------------------------------------------------------------------------------------------ kernels
@gpu
@pytest.mark.parametrize("lens", LENS)
@pytest.mark.parametrize("layer", [0, 7, 15])
def test_cv_wn_layer_against_fp64(sd, lens, layer):
    from cosyvoice_amd import _lib as L
    from cosyvoice_amd.style import wn_layer
    g = torch.Generator().manual_seed(100 * layer + sum(lens))
    H, B, T = 512, len(lens), max(lens)
    c = R.Ctx(sd)
    w_in, b_in = c.wn(f"enc_q.enc.in_layers.{layer}"), sd[f"enc_q.enc.in_layers.{layer}.bias"]
    w_rs, b_rs = c.wn(f"enc_q.enc.res_skip_layers.{layer}"), sd[f"enc_q.enc.res_skip_layers.{layer}.bias"]
    n_rs = w_rs.shape[0]
    assert n_rs == (512 if layer == 15 else 1024)
    x, rows = _ragged(lens, H, g)
    skip0, srows = _ragged(lens, H, g)
    first = layer == 0
    lay = dict(w_in=w_in.permute(0, 2, 1).reshape(2 * H, 5 * H).contiguous().cuda(), b_in=b_in.cuda(), w_rs=w_rs[:, :, 0].contiguous().cuda(),
               b_rs=b_rs.cuda())
    Tp = T + 3
    xd, sk, xo = x.cuda(), skip0.cuda().clone(), nan_buf(B, Tp, H)
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    p_T = Tp                                          # the kernel sees the slack rows as padded rows of the sequence
    wn_layer(xd.view(B * Tp, H), xo.view(B * Tp, H), sk.view(B * Tp, H), lens_d, B, p_T, lay, first=first)
    torch.cuda.synchronize()
    assert L.STYLE_EXPORTS and "cv_wn_layer" in L.STYLE_EXPORTS and "cv_sizeof_wn_layer_params" in L.STYLE_EXPORTS
    for b, n in enumerate(lens):
        outs = {}
        for dt in (torch.float32, torch.float64):
            xr = rows[b].to(dt)
            a = F.conv1d(xr.t().unsqueeze(0), w_in.to(dt), b_in.to(dt), padding=2)[0].t()
            acts = torch.tanh(a[:, :H]) * torch.sigmoid(a[:, H:])
            rs = acts @ w_rs[:, :, 0].to(dt).t() + b_rs.to(dt)
            sk_ref = rs[:, -H:] if first else srows[b].to(dt) + rs[:, -H:]
            outs[dt] = (xr + rs[:, :H] if n_rs == 2 * H else None, sk_ref)
        x32, s32 = outs[torch.float32]
        x64, s64 = outs[torch.float64]
        assert rel_err(sk[b, :n], s64) <= op_tol(s32, s64), ("skip", b, rel_err(sk[b, :n], s64), op_tol(s32, s64))
        assert torch.all(sk[b, n:] == 0)
        if n_rs == 2 * H:
            assert rel_err(xo[b, :n], x64) <= op_tol(x32, x64), ("x_out", b, rel_err(xo[b, :n], x64), op_tol(x32, x64))
            assert torch.all(xo[b, n:] == 0)                   # rows at and past the length are exactly 0
        else:
            assert torch.isnan(xo).all()                       # the last layer has no residual output


@gpu
def test_cv_wn_gate_and_composed_layers_match_the_fused_ones(model):
    """cv_wn_gate against fp64, and the posterior encoder composed from cv_gemm launches + that gate (what tools/style_bench.py
    times) against the fused one: the same m / logs up to the summation order."""
    from cosyvoice_amd.style import _wn_layer_composed  # noqa: F401
    from cosyvoice_amd import _lib as L
    g = torch.Generator().manual_seed(21)
    a = torch.randn(70, 1024, generator=g) * 2
    out = nan_buf(70, 512)
    L.check(L.style_lib().cv_wn_gate(a.cuda().data_ptr(), 1024, out.data_ptr(), 512, 70, 512, L.stream_ptr()), "cv_wn_gate")
    r64 = torch.tanh(a[:, :512].double()) * torch.sigmoid(a[:, 512:].double())
    r32 = torch.tanh(a[:, :512]) * torch.sigmoid(a[:, 512:])
    assert rel_err(out, r64) <= max(op_tol(r32, r64), MARGIN * 2.0 ** -24)
    lens, B, T = (70, 33), 2, 96
    mag = (torch.randn(B * T, 516, generator=g).abs() * 3).cuda()
    mag[:, 513:] = 0
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    enc = model.enc_q
    ws_f, ws_c = enc.workspace(B, T), enc.workspace(B, T)
    extra = dict(a=nan_buf(B * T, 1024), g=nan_buf(B * T, 512))
    enc.enqueue(mag, lens_d, B, T, ws_f, fused=True)
    enc.enqueue(mag, lens_d, B, T, ws_c, fused=False, extra=extra)
    f, c = ws_f["stats"].view(B, T, 1024), ws_c["stats"].view(B, T, 1024)
    for b, n in enumerate(lens):
        assert torch.isfinite(f[b, :n]).all()
        assert rel_err(c[b, :n], f[b, :n].cpu()) <= TOL["style_t100"]["m"]


@gpu
@pytest.mark.parametrize("lens", LENS)
def test_cv_glu_conv_against_fp64(sd, lens):
    from cosyvoice_amd.style import glu_conv
    g = torch.Generator().manual_seed(sum(lens))
    D, B, T = 256, len(lens), max(lens)
    w, bias = sd["style_encoder.temporal_layers.2.1.conv1.conv.weight"], sd["style_encoder.temporal_layers.2.1.conv1.conv.bias"]
    x, rows = _ragged(lens, D, g)
    Tp = T + 3
    y = nan_buf(B, Tp, D)
    glu_conv(x.cuda().view(B * Tp, D), y.view(B * Tp, D), torch.tensor(lens, dtype=torch.int32).cuda(), B, Tp,
             w.permute(0, 2, 1).reshape(2 * D, 5 * D).contiguous().cuda(), bias.cuda())
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        ref = {}
        for dt in (torch.float32, torch.float64):
            xr = rows[b].to(dt)
            a = F.conv1d(xr.t().unsqueeze(0), w.to(dt), bias.to(dt), padding=2)[0].t()
            ref[dt] = xr + a[:, :D] * torch.sigmoid(a[:, D:])
        tol = op_tol(ref[torch.float32], ref[torch.float64])
        assert rel_err(y[b, :n], ref[torch.float64]) <= tol, (b, rel_err(y[b, :n], ref[torch.float64]), tol)
        assert torch.all(y[b, n:] == 0)


@gpu
@pytest.mark.parametrize("B", [1, 3])
def test_cv_gst_attention_against_fp64(B):
    from cosyvoice_amd.style import gst_attention
    g = torch.Generator().manual_seed(B)
    Hh, N = 8, 4096
    q = torch.randn(B, 512, generator=g) * 3
    k = torch.randn(Hh, N, 64, generator=g)
    v = torch.randn(Hh, N, 64, generator=g)
    out = nan_buf(B, 512)
    gst_attention(q.cuda(), k.cuda(), v.cuda(), out, B, 0.125)
    ref = {}
    for dt in (torch.float32, torch.float64):
        p = torch.softmax(torch.einsum("bhd,hnd->bhn", q.view(B, Hh, 64).to(dt), k.to(dt)) / 8, dim=-1)
        ref[dt] = torch.einsum("bhn,hnd->bhd", p, v.to(dt)).reshape(B, 512)
    tol = op_tol(ref[torch.float32], ref[torch.float64])
    assert rel_err(out, ref[torch.float64]) <= tol, (rel_err(out, ref[torch.float64]), tol)
    if B == 3:                                             # a row does not depend on the batch around it
        one = nan_buf(1, 512)
        gst_attention(q[1:2].cuda(), k.cuda(), v.cuda(), one, 1, 0.125)
        assert torch.equal(one[0], out[1])


@gpu
@pytest.mark.parametrize("lens", LENS)
def test_cv_style_attention_against_fp64(lens):
    from cosyvoice_amd.style import style_attention
    g = torch.Generator().manual_seed(7 + sum(lens))
    D, Hh, B, T = 256, 4, len(lens), max(lens)
    qkv, rows = _ragged(lens, 3 * D, g, scale=2.0)
    Tp = T + 3
    out = nan_buf(B, Tp, D)
    style_attention(qkv.cuda().view(B * Tp, 3 * D), out.view(B * Tp, D), torch.tensor(lens, dtype=torch.int32).cuda(), B, Tp, 1 / 16)
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        ref = {}
        for dt in (torch.float32, torch.float64):
            q, k, v = (rows[b][:, i * D:(i + 1) * D].to(dt).view(n, Hh, 64).transpose(0, 1) for i in range(3))
            p = torch.softmax(q @ k.transpose(1, 2) / 16, dim=-1)
            ref[dt] = (p @ v).transpose(0, 1).reshape(n, D)
        tol = op_tol(ref[torch.float32], ref[torch.float64])
        assert rel_err(out[b, :n], ref[torch.float64]) <= tol, (b, rel_err(out[b, :n], ref[torch.float64]), tol)
        assert torch.all(out[b, n:] == 0)


@gpu
def test_cv_masked_mean_lengths_1_2_T():
    from cosyvoice_amd.style import masked_mean
    g = torch.Generator().manual_seed(5)
    lens, T, Cc = (1, 2, 37, 0), 37, 512
    x, rows = _ragged(lens, Cc, g)
    x = x[:, :T].contiguous()
    out = nan_buf(len(lens), Cc)
    masked_mean(x.cuda().view(len(lens) * T, Cc), torch.tensor(lens, dtype=torch.int32).cuda(), len(lens), T, Cc, out)
    for b, n in enumerate(lens):
        if n == 0:
            assert torch.all(out[b] == 0)
            continue
        r64 = rows[b].double().sum(0) / n
        r32 = rows[b].sum(0) / n
        assert rel_err(out[b], r64) <= max(op_tol(r32, r64), MARGIN * 2.0 ** -24)


@gpu
def test_cv_posterior_sample():
    from cosyvoice_amd.style import posterior_sample
    g = torch.Generator().manual_seed(6)
    lens, T, H = (33, 5), 33, 512
    stats, srows = _ragged(lens, 2 * H, g)
    noise, nrows = _ragged(lens, H, g)
    stats, noise = stats[:, :T].contiguous(), noise[:, :T].contiguous()
    z = nan_buf(2, T, H)
    posterior_sample(stats.cuda().view(2 * T, 2 * H), noise.cuda().view(2 * T, H), z.view(2 * T, H), torch.tensor(lens, dtype=torch.int32).cuda(),
                     2, T)
    for b, n in enumerate(lens):
        r64 = srows[b][:, :H].double() + nrows[b].double() * torch.exp(srows[b][:, H:].double())
        r32 = srows[b][:, :H] + nrows[b] * torch.exp(srows[b][:, H:])
        assert rel_err(z[b, :n], r64) <= max(op_tol(r32, r64), MARGIN * 2.0 ** -24)
        assert torch.all(z[b, n:] == 0)


# ------------------------------------------------------------------------------------------------------------ spectrogram
@gpu
def test_linear_spectrogram_matches_restatement():
    from cosyvoice_amd.style import LinearSpectrogram
    ls = LinearSpectrogram()
    sizes = (363, 600, 30000, 90000)
    waves = [R.test_signal(S, seed=S) for S in sizes]
    refs = [R.linear_spectrogram(w, torch.float64) for w in waves]
    # baseline in the kernel's arithmetic: the DFT as an fp32 matrix product (1024-term sums), not torch's FFT
    tols = [op_tol(R.linear_spectrogram_dft(w, torch.float32), r) for w, r in zip(waves, refs)]
    singles = []
    for w, ref, tol in zip(waves, refs, tols):
        spec, frames = ls(w)
        assert frames == [w.numel() // 300] and spec.shape == (1, max(frames[0], 1), 513) and ref.shape[0] == frames[0]
        assert rel_err(spec[0, :frames[0]], ref) <= tol, (w.numel(), rel_err(spec[0, :frames[0]], ref), tol)
        singles.append(spec[0, :frames[0]].clone())
    buf = torch.full((4, 90000 + 50), float("nan"))
    for b, w in enumerate(waves):
        buf[b, :w.numel()] = w
    spec, frames = ls((buf, list(sizes)))
    assert frames == [1, 2, 100, 300]
    for b, one in enumerate(singles):
        assert torch.equal(spec[b, :frames[b]], one)       # reflects at its own end, independent of the batch and its padding
        assert torch.all(spec[b, frames[b]:] == 0)
    with pytest.raises(ValueError):
        ls(torch.zeros(362))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def refs64(sd):
    """The fp64 restatement of the committed cases, computed once."""
    from cosyvoice_amd.weights import speaker_embedding_state_dict
    out = {}
    for tag in ("style_t100", "style_t300", "style_wo_t100"):
        c = load_case(tag)
        s = sd if c["post"] else speaker_embedding_state_dict(1986, post_enc=False)
        out[tag] = R.speaker_embedding(s, c["wave"], c["n"], c["noise"], c["timbre"], dtype=torch.float64, post_enc=c["post"])
    return out


@gpu
@pytest.mark.parametrize("tag", ["style_t100", "style_t300", "style_wo_t100"])
def test_stages_against_fp64_restatement_and_goldens(model, model_wo, refs64, tag):
    c = load_case(tag)
    m = model if c["post"] else model_wo
    T = c["n"] // 300
    kw = dict(noise=[c["noise"]]) if c["post"] else {}
    g = m([c["wave"][:c["n"]]], timbre=c["timbre"].view(1, -1), **kw)
    st, ref, fx, tol = m.stages, refs64[tag], c["fx"], TOL[tag]
    got = {"style_vec": st["style_vec"][0], "gst_out": st["gst_out"][0], "g": g[0]}
    if c["post"]:
        got.update(m=st["m"][0, :T], logs=st["logs"][0, :T], z=st["z"][0, :T])
    else:
        got["z"] = m._ws[(1, m.bucket(T))]["z"][:T]
    errs = {k: rel_err(v, ref[k]) for k, v in got.items()}
    print(tag, "GPU vs fp64:", {k: "%.2e" % e for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= tol[k], (k, e, tol[k])
    # the reference's own output (fp32 torch on the CPU), same constants
    idx = torch.from_numpy(fx["row_idx"]) if c["post"] else None
    gold = {k: (got[k].cpu(), fx[k], float(np.abs(fx[k]).max())) for k in ("style_vec", "gst_out", "g")}
    if c["post"]:
        gold["m"] = (got["m"].cpu()[idx], fx["m_rows"], float(fx["m_absmax"]))
        gold["logs"] = (got["logs"].cpu()[idx], fx["logs_rows"], float(fx["logs_absmax"]))
    for k, (a, b, scale) in gold.items():
        e = float((a.double() - torch.from_numpy(b).double()).abs().max()) / scale
        print(tag, "GPU vs golden", k, "%.2e" % e)
        assert e <= tol[k], ("golden", k, e, tol[k])


@gpu
def test_ragged_batch_graph_and_replay_are_bit_identical(model):
    frames = (300, 100, 64, 7)
    S = [f * 300 + 11 * (i + 1) for i, f in enumerate(frames)]
    waves = [R.test_signal(s, seed=40 + i) for i, s in enumerate(S)]
    gen = torch.Generator().manual_seed(9)
    noise = [torch.randn(512, f, generator=gen) for f in frames]
    timbre = torch.randn(4, 192, generator=gen)
    singles = [model([w], noise=[n], timbre=timbre[b:b + 1], graph=False)[0].clone() for b, (w, n) in enumerate(zip(waves, noise))]
    for junk in (1e4, -1e4, float("nan")):
        buf = torch.full((4, 1, max(S) + 77), junk)
        for b, w in enumerate(waves):
            buf[b, 0, :S[b]] = w
        for t in model._ws.get((4, 320), {}).values():      # junk in the workspace of this shape as well
            if isinstance(t, torch.Tensor) and t.dtype == torch.float32:
                t.fill_(junk)
        out = model(buf, wave_lengths=S, noise=noise, timbre=timbre, graph=False)
        for b in range(4):
            assert torch.equal(out[b], singles[b]), (junk, b)
    replay = model(buf, wave_lengths=S, noise=noise, timbre=timbre, graph=True)        # captures (4, 320)
    assert torch.equal(replay, out)
    # 2 spectrogram + pre + 16 WaveNet layers + proj + sample + in_fc + 6 x 7 + fc + mean + 6 x 2 style-token + fuse
    n = model.num_launches((4, 320))
    print("launches in the (4, 320) graph:", n)
    assert 79 <= n <= 100 and model.num_launches((9, 64)) is None      # one kernel node or more per launch issued
    # other lengths in the same bucket through the same graph
    frames2 = (290, 257, 33, 300)
    S2 = [f * 300 + 5 for f in frames2]
    waves2 = [R.test_signal(s, seed=50 + i) for i, s in enumerate(S2)]
    noise2 = [torch.randn(512, f, generator=gen) for f in frames2]
    out2 = model(waves2, noise=noise2, timbre=timbre, graph=True)
    for b in range(4):
        one = model([waves2[b]], noise=[noise2[b]], timbre=timbre[b:b + 1], graph=True)
        assert torch.equal(out2[b], one[0]), b


@gpu
def test_full_call_draws_noise_and_runs_campplus(model):
    """No noise and no timbre given: CAM++ on the 16 kHz resampling, noise from the generator; same generator state, same vector."""
    w = R.test_signal(24000, seed=3)
    g1 = torch.Generator(device="cuda").manual_seed(1)
    g2 = torch.Generator(device="cuda").manual_seed(1)
    a, b = model([w], generator=g1), model([w], generator=g2)
    assert a.shape == (1, 512) and torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, model([w], generator=g2))      # the next draw: the embedding is random per call, as the reference's
    with pytest.raises(ValueError):
        model([torch.zeros(362)])
    with pytest.raises(ValueError):
        model([torch.zeros(700)])                             # reflect-paddable, but too short for fbank + CAM++


@gpu
def test_prompt_front_end_speaker_encoder_keyword(model):
    from cosyvoice_amd.frontend import MelSpectrogram, PromptFrontEnd
    fe0 = PromptFrontEnd(MelSpectrogram(), model.campplus)
    fe1 = PromptFrontEnd(MelSpectrogram(), model.campplus, speaker_encoder=model)
    w16 = R.test_signal(16000, seed=8, sr=16000)
    text, ptext, tok = torch.arange(5, dtype=torch.int32), torch.arange(3, dtype=torch.int32), torch.arange(20, dtype=torch.int32)
    d0 = fe0.frontend_zero_shot(text, ptext, w16, tok, 24000)
    d1 = fe1.frontend_zero_shot(text, ptext, w16, tok, 24000)
    assert d0["llm_embedding"].shape == (1, 192) and d1["llm_embedding"].shape == (1, 512) and d1["flow_embedding"].shape == (1, 512)
    assert torch.isfinite(d1["llm_embedding"]).all()
    for k in d0:
        if "embedding" not in k:
            assert torch.equal(torch.as_tensor(d0[k]).cpu(), torch.as_tensor(d1[k]).cpu()), k
    assert torch.equal(d0["llm_embedding"], model.campplus.extract_spk_embedding([w16]))    # without the keyword nothing changes
    b = fe1.batch([text, text], [ptext, ptext], [w16, w16[:12000]], [tok, tok])
    assert b["flow_embeddings"].shape == (2, 512)
