"""GPU: the ragged HiFT vocoder — B utterances of different lengths through ONE launch sequence (HiFTGenerator.decode_ragged /
inference_ragged, cv_hift_decode_desc.lens, cv_gemm_params.len_base), every row against what the vocoder computes for that utterance
alone: the reference-minted goldens, the CPU oracle, and batch-1 runs on the same object.

Tolerances are the existing ones: 1e-4 (fp32 tensors) / 2e-3 (16-bit) on the waveform against the reference, 2e-3 Hz on f0, 1e-6 for
"batch row == single run" (tests/test_hift_gpu.py::test_batched_decode_matches_single, tests/test_headline_shapes_gpu.py), 1e-3 for the
injected-source inference (test_inference_vs_oracle_full_shape).  Padding independence and shape reuse are conditions (torch.equal)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cosyvoice_amd.config import FlowConfig, HiftConfig, LlmConfig
from cosyvoice_amd.weights import flow_state_dict, hift_state_dict, llm_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402
import test_gemm_modes_gpu as GM  # noqa: E402  (operand / buffer builders of the cv_gemm mode tests)

pytestmark = pytest.mark.gpu

CFGS = {"tiny": HiftConfig.tiny(), "v2": HiftConfig.v2(), "v1": HiftConfig.v1()}
_SD = {}


def _sd(tag):
    if tag not in _SD:
        _SD[tag] = hift_state_dict(CFGS[tag])
    return _SD[tag]


def _gen(tag, dt=torch.float32, mode="bf16x3"):
    from cosyvoice_amd.hift import HiFTGenerator
    return HiFTGenerator(CFGS[tag], dtype=dt, f32_products=mode).load_state_dict(_sd(tag))


def _golden(golden_dir, name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, f"hift_{name}.npz")).items()}


def _synth_mel(frames, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.clamp(torch.randn(1, 80, frames, generator=g) * 2.0 - 6.0, -11.5, 2.0)


def _synth_src(cfg, frames, seed):
    return torch.randn(1, 1, frames * cfg.total_upsample, generator=torch.Generator().manual_seed(seed)) * 0.05


# ----------------------------------------------------------------------------- 1. against the reference's goldens
LONG_ROW0 = {"v2": 517, "v1": 870}


@pytest.mark.parametrize("mode", ["bf16x3", "exact"])
@pytest.mark.parametrize("tag", ["v2", "v1"])
def test_ragged_rows_vs_reference_goldens(golden_dir, tag, mode):
    """One ragged batch: row 0 a seeded mel longer than everything else (every other row is padded), row 1 the baseline-length inputs
    of hift_<tag>_long.npz, row 2 the short golden's mel / s, row 3 a seeded mel of an odd length.  Rows 1 and 2 meet their goldens exactly
    as the batch-1 runs of the existing tests do; rows 0 and 3 equal their own batch-1 decode."""
    cfg = CFGS[tag]
    gl, gs = _golden(golden_dir, f"{tag}_long"), _golden(golden_dir, tag)
    frames = int(gl["frames"])
    mels = [_synth_mel(LONG_ROW0[tag], 901), _synth_mel(frames, int(gl["mel_seed"])), gs["mel"], _synth_mel(133, 902)]
    srcs = [_synth_src(cfg, LONG_ROW0[tag], 903), _synth_src(cfg, frames, int(gl["s_seed"])), gs["s"], _synth_src(cfg, 133, 904)]
    m = _gen(tag, mode=mode)
    wavs = [w.cpu() for w in m.decode_ragged([x.cuda() for x in mels], [s.cuda() for s in srcs])]
    assert [w.numel() for w in wavs] == [x.shape[2] * cfg.total_upsample for x in mels]
    # row 1: the long golden (every 8th sample, block statistics), tests/test_headline_shapes_gpu.py
    wav = wavs[1][None]
    assert wav.shape[1] == int(gl["n_samples"])
    e = (wav[:, ::8] - gl["wav_sub8"]).abs().max().item()
    blk = wav[0, : wav.shape[1] // 2400 * 2400].view(-1, 2400).abs()
    eb = (blk.max(dim=1).values - gl["wav_block_absmax"]).abs().max().item()
    em = (blk.mean(dim=1) - gl["wav_block_absmean"]).abs().max().item()
    # row 2: the short golden
    es = (wavs[2][None] - gs["wav"]).abs().max().item()
    print(f"ragged hift {tag} [{mode}] lengths {[x.shape[2] for x in mels]}: long row Linf {e:.2e} blockmax {eb:.2e} blockmean {em:.2e}; short row Linf {es:.2e}")
    assert e < 1e-4 and eb < 1e-4 and em < 1e-4
    assert es < 1e-4
    # f0 of the padded batch, rows 1 and 2 against the goldens
    T = max(x.shape[2] for x in mels)
    pad = torch.stack([F.pad(x[0], (0, T - x.shape[2])) for x in mels])
    f0 = m.f0_predictor(pad.cuda(), lengths=[x.shape[2] for x in mels]).cpu()
    ef = [(f0[1, :frames] - gl["f0"][0]).abs().max().item(), (f0[2, :gs["f0"].shape[1]] - gs["f0"][0]).abs().max().item()]
    print(f"  f0 Linf {ef[0]:.2e} / {ef[1]:.2e} Hz")
    assert max(ef) < 2e-3
    # rows without a golden: their own batch-1 decode on the same object
    for b in (0, 3):
        w1 = m.decode(mels[b].cuda(), srcs[b].cuda())[0].cpu()
        d = (w1 - wavs[b]).abs().max().item()
        print(f"  row {b} vs batch-1 decode: {d:.2e}, bit-identical {torch.equal(w1, wavs[b])}")
        assert d < 1e-6
        # measured bit-identical on MI355X although the padded batch and the single run take different row tiles (128 vs 64 rows): the K
        # loop's order per output element does not depend on the tile
        assert torch.equal(w1, wavs[b])


@pytest.mark.parametrize("mode", ["bf16x3", "exact"])
def test_ragged_rows_vs_reference_golden_tiny(golden_dir, mode):
    cfg = CFGS["tiny"]
    gs = _golden(golden_dir, "tiny")
    mels = [_synth_mel(47, 911), gs["mel"], _synth_mel(13, 912)]
    srcs = [_synth_src(cfg, 47, 913), gs["s"], _synth_src(cfg, 13, 914)]
    m = _gen("tiny", mode=mode)
    wavs = [w.cpu() for w in m.decode_ragged([x.cuda() for x in mels], [s.cuda() for s in srcs])]
    es = (wavs[1][None] - gs["wav"]).abs().max().item()
    print(f"ragged hift tiny [{mode}]: golden row Linf {es:.2e}")
    assert wavs[1].numel() == gs["wav"].shape[1] and es < 1e-4
    T = max(x.shape[2] for x in mels)
    pad = torch.stack([F.pad(x[0], (0, T - x.shape[2])) for x in mels])
    f0 = m.f0_predictor(pad.cuda(), lengths=[x.shape[2] for x in mels]).cpu()
    assert (f0[1, :gs["f0"].shape[1]] - gs["f0"][0]).abs().max().item() < 2e-3


@pytest.mark.parametrize("tag", ["tiny", "v2", "v1"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_ragged_16bit_vs_short_golden(golden_dir, tag, dt):
    cfg = CFGS[tag]
    gs = _golden(golden_dir, tag)
    mels = [_synth_mel(33, 921), gs["mel"]]
    srcs = [_synth_src(cfg, 33, 922), gs["s"]]
    m = _gen(tag, dt=dt)
    wavs = m.decode_ragged([x.cuda() for x in mels], [s.cuda() for s in srcs])
    err = (wavs[1].cpu()[None] - gs["wav"]).abs().max().item()
    print(f"ragged hift {tag} [{dt}]: golden row Linf {err:.2e}")
    assert err < 2e-3


# ----------------------------------------------------------------------------- 2. against batch-1 runs at tile / block edges
# v2: frames -> rows 8 / 40 / 120 (+ 1) per stage; the conv row tiles are 64 and 128 rows, the iSTFT block 64 frames = 256 samples.
#   64 / 8 = 8 frames ends stage-0 tiles (and 8 * 120 = 15 iSTFT blocks exactly): 7, 8, 9;  128 / 8 = 16: 16, 17;  the 128-row tile of
#   stage 1 ends between 3 and 4 frames; 1 and 2 frames are the shortest utterances (one frame = 480 samples > the STFT's 8-sample reflection).
# tiny: rows 4 / 12 (+ 1): 64 / 4 = 16 frames: 15, 16, 17;  64 / 12: 5, 6;  16 * 12 = 3 iSTFT blocks exactly.
EDGE = {"v2": [1, 2, 3, 4, 7, 8, 9, 16, 17, 33], "tiny": [1, 5, 6, 15, 16, 17, 21, 32, 43]}
# measured on MI355X: every row is bit-identical to its batch-1 decode in these configurations (same kernels, same summation order per
# output element) — asserted, as the flow and the speaker embedding assert theirs
BIT_IDENTICAL = {("tiny", "bf16x3"), ("tiny", "exact"), ("v2", "bf16x3"), ("v2", "exact")}


@pytest.mark.parametrize("mode", ["bf16x3", "exact"])
@pytest.mark.parametrize("tag", ["tiny", "v2"])
def test_ragged_rows_equal_batch1_runs_at_tile_edges(tag, mode):
    from oracle import hift as oh
    cfg, sd = CFGS[tag], _sd(tag)
    lens = EDGE[tag]
    mels = [_synth_mel(n, 930 + i) for i, n in enumerate(lens)]
    srcs = [_synth_src(cfg, n, 960 + i) for i, n in enumerate(lens)]
    m = _gen(tag, mode=mode)
    wavs = [w.clone() for w in m.decode_ragged([x.cuda() for x in mels], [s.cuda() for s in srcs])]
    worst, worst_o, equal = 0.0, 0.0, True
    for b, n in enumerate(lens):
        w1 = m.decode(mels[b].cuda(), srcs[b].cuda())[0]
        assert wavs[b].shape == w1.shape == (n * cfg.total_upsample,)
        d = (w1 - wavs[b]).abs().max().item()
        equal = equal and torch.equal(w1, wavs[b])
        ref = oh.decode(sd, cfg, mels[b], srcs[b])[0]
        do = (wavs[b].cpu() - ref).abs().max().item()
        worst, worst_o = max(worst, d), max(worst_o, do)
        assert d < 1e-6, (n, d)
        assert do < 1e-4, (n, do)
    print(f"ragged hift {tag} [{mode}] lengths {lens}: vs batch-1 {worst:.2e} (bit-identical: {equal}), vs CPU oracle {worst_o:.2e}")
    if (tag, mode) in BIT_IDENTICAL:
        assert equal


# ----------------------------------------------------------------------------- 3. padding independence
def _fill_junk(obj, value):
    if isinstance(obj, torch.Tensor):
        if obj.is_floating_point():
            obj.fill_(value)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _fill_junk(o, value)


@pytest.mark.parametrize("tag,mode", [("tiny", "bf16x3"), ("tiny", "exact"), ("v2", "bf16x3")])
def test_padding_independence(tag, mode):
    """The same ragged batch with the padded tail of every input zero, then +-1e4, and the whole workspace overwritten with junk in
    between: the valid part of every output row does not change by a bit.  (Masking only the first layer fails this.)"""
    cfg = CFGS[tag]
    up = cfg.total_upsample
    lens = [9, 40, 23, 1]
    m = _gen(tag, mode=mode)
    m.length_bucket = 8
    T = 40
    outs = []
    for junk in (0.0, 1.0e4, -1.0e4):
        mel = torch.full((len(lens), 80, T), junk)
        src = torch.full((len(lens), 1, T * up), junk)
        for b, n in enumerate(lens):
            mel[b, :, :n] = _synth_mel(n, 940 + b)[0]
            src[b, :, :n * up] = _synth_src(cfg, n, 950 + b)[0]
        # every activation, the staged mel and the source buffer (decode_ragged copies only each row's valid samples into it, so this is
        # what lies behind every row's S_b) hold junk of the opposite sign when the call starts
        for key, val in m._ws.get((len(lens), T), {}).items():
            if not (isinstance(key, tuple) and key[0].startswith("_desc")):
                _fill_junk(val, -junk if junk else 3.0e4)
        wavs = m.decode_ragged(mel.cuda(), src.cuda(), lengths=lens)
        outs.append([w.clone() for w in wavs])
    torch.cuda.synchronize()
    assert len(m._ws) == 1
    for b in range(len(lens)):
        assert outs[0][b].shape == (lens[b] * up,) and torch.isfinite(outs[0][b]).all() and outs[0][b].abs().max().item() > 0
        for k in (1, 2):
            assert torch.equal(outs[0][b], outs[k][b]), (b, k, (outs[0][b] - outs[k][b]).abs().max().item())


# ----------------------------------------------------------------------------- 4. inference_ragged
def test_inference_ragged_vs_oracle():
    from oracle import hift as oh
    cfg, sd = CFGS["v2"], _sd("v2")
    up = cfg.total_upsample
    lens = [100, 37, 64]
    mels = [_synth_mel(n, 970 + i) for i, n in enumerate(lens)]
    rnd = [oh.draw_source_randoms(cfg, 1, n * up, seed=5 + i) for i, n in enumerate(lens)]
    caches = [None, torch.randn(1, 1, 960, generator=torch.Generator().manual_seed(7)) * 0.05, torch.zeros(1, 1, 0)]
    m = _gen("v2")
    wavs, srcs = m.inference_ragged([x.cuda() for x in mels], cache_source=caches, phase_vec=[r[0].cuda() for r in rnd],
                                    noise=[r[1].cuda() for r in rnd])
    wavs, srcs = [w.cpu() for w in wavs], [s.cpu() for s in srcs]
    for b, n in enumerate(lens):
        wav_ref, s_ref = oh.inference(sd, cfg, mels[b], caches[b], rnd[b][0], rnd[b][1], scan_dtype=torch.float64)
        assert wavs[b].shape == (n * up,) and srcs[b].shape == (1, n * up)
        es, ew = (srcs[b] - s_ref[0]).abs().max().item(), (wavs[b] - wav_ref[0]).abs().max().item()
        print(f"inference_ragged row {b} ({n} frames): source {es:.2e} wav {ew:.2e}")
        assert es < 1e-3 and ew < 1e-3
    assert torch.allclose(srcs[1][:, :960], caches[1][0], atol=1e-6)


# ----------------------------------------------------------------------------- 5. one shape, many lengths; the graph form
def test_one_workspace_and_descriptor_serve_every_length_set():
    cfg = CFGS["tiny"]
    m = _gen("tiny")
    m.length_bucket = 32
    utt = {n: (_synth_mel(n, 980 + n).cuda(), _synth_src(cfg, n, 990 + n).cuda()) for n in (20, 31, 9, 5, 27, 32)}
    run = lambda ns: [w.clone() for w in m.decode_ragged([utt[n][0] for n in ns], [utt[n][1] for n in ns])]
    a = run([20, 31, 9])
    ws = m._ws[(3, 32)]
    desc = ws[("_desc_ragged", m.presplit)][0]
    keys = set(ws)
    ptrs = {k: v.data_ptr() for k, v in ws.items() if isinstance(v, torch.Tensor)}
    b = run([5, 27, 32])
    assert len(m._ws) == 1 and m._ws[(3, 32)] is ws and ws[("_desc_ragged", m.presplit)][0] is desc
    assert set(ws) == keys and ptrs == {k: v.data_ptr() for k, v in ws.items() if isinstance(v, torch.Tensor)}   # nothing allocated
    c = run([9, 20, 31])     # the first set, permuted across rows
    assert len(m._ws) == 1
    assert torch.equal(c[0], a[2]) and torch.equal(c[1], a[0]) and torch.equal(c[2], a[1])
    d = run([32, 5, 27])
    assert torch.equal(d[0], b[2]) and torch.equal(d[1], b[0]) and torch.equal(d[2], b[1])


def test_graph_captured_once_replays_any_lengths():
    """cv_hift_decode_graph_create over a ragged descriptor: ONE capture; the device length array is rewritten between replays and every
    replay equals the eager cv_hift_decode_enqueue with the same lengths."""
    from cosyvoice_amd import _lib as L
    from cosyvoice_amd import ops
    cfg = CFGS["tiny"]
    up = cfg.total_upsample
    m = _gen("tiny")
    B, T = 3, 32
    ws = m._workspace(B, T)
    lens_dev = torch.zeros(B, dtype=torch.int32, device="cuda")
    mel = torch.cat([_synth_mel(T, 1000 + b) for b in range(B)]).cuda()
    s = torch.cat([_synth_src(cfg, T, 1010 + b) for b in range(B)]).reshape(B, -1).cuda().contiguous()
    ops.to_channels_last(mel, ws["mel_cl"])
    desc, keep = m.decode_desc(ws, B, T)
    desc.gemm_dtype = L.CV_F32X3
    desc.s, desc.lens = s.data_ptr(), lens_dev.data_ptr()
    g = ops.Graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.check(L.lib().cv_hift_decode_graph_create(C.byref(desc), L.stream_ptr(), C.byref(g.handle)), "cv_hift_decode_graph_create")
    torch.cuda.current_stream().wait_stream(side)
    try:
        assert g.num_launches > 30
        for lens in ([32, 7, 19], [3, 30, 16]):
            lens_dev.copy_(torch.tensor(lens, dtype=torch.int32))
            ws["wav"].fill_(7.0)
            g.launch()
            got = [ws["wav"][b, :n * up].clone() for b, n in enumerate(lens)]
            ws["wav"].fill_(-7.0)
            L.check(L.lib().cv_hift_decode_enqueue(C.byref(desc), L.stream_ptr()), "cv_hift_decode_enqueue")
            for b, n in enumerate(lens):
                eager = ws["wav"][b, :n * up]
                assert torch.isfinite(eager).all() and eager.abs().max().item() <= cfg.audio_limit + 1e-6
                assert torch.equal(got[b], eager), (lens, b)
                w1 = m.decode(mel[b:b + 1, :, :n].contiguous(), s[b:b + 1, :n * up].contiguous())[0]
                assert (w1 - got[b]).abs().max().item() < 1e-6
    finally:
        torch.cuda.synchronize()
        g.destroy()


# ----------------------------------------------------------------------------- 6. ABI level
@pytest.mark.parametrize("mode", GM.MODES)
def test_cv_gemm_ragged_conv(mode):
    """cv_gemm with len_base on a k = 7, dilation 3 conv: two batch rows of different lengths inside one padded buffer whose rows past each
    length hold NaN — against the fp64 conv of each row alone with zero padding, at the bounds of tests/test_gemm_modes_gpu.py.  Row tiles
    that lie wholly past a row's length are skipped: their outputs keep the NaN pre-fill."""
    from cosyvoice_amd import ops
    torch.manual_seed(77)
    B, T, cin, cout, k, dil = 2, 150, 24, 40, 7, 3
    lens = [61, 130]
    pad = dil * (k - 1) // 2
    x = GM.rvals(torch.randn(B, T, cin), mode)
    w = GM.rvals(torch.randn(cout, cin, k) / (cin * k) ** 0.5, mode)
    bias = torch.randn(cout)
    xp = x.clone()
    for b, n in enumerate(lens):
        xp[b, n:] = float("nan")
    xd, wd = GM.dev_op(xp, mode, cin + 8), GM.dev_op(GM.pack_w(w), mode, k * cin + 8)
    o = GM.Outs(mode, B, T, cout)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ops.conv1d_cl(xd, wd, k, dilation=dil, pad_left=pad, bias=bias.cuda(), out_f32=o.o32[:, :T, :cout], out_act=o.oa[:, :T, :cout],
                  lens=ld, a_len=(1, 0), m_len=(1, 0), **GM.gkw(mode))
    torch.cuda.synchronize()
    x3 = mode in ("x3", "x3ps")
    for b, n in enumerate(lens):
        ref, sabs = GM.conv_ref(x[b:b + 1, :n], w, bias, GM.F64, dil=dil, pad=(pad, pad))
        H.check(f"ragged conv [{mode}] row {b} out_f32", o.o32[b:b + 1, :n, :cout].cpu(), ref, H.sum_bound(cin * k + 1, sabs, ref, torch.float32, x3=x3))
        H.check(f"ragged conv [{mode}] row {b} out_act", o.oa[b:b + 1, :n, :cout].cpu(), ref, H.sum_bound(cin * k + 1, sabs, ref, GM.DT[mode], x3=x3))
        skipped = (n + 63) // 64 * 64      # the register-staged tiles this shape gets are 64 rows
        assert bool(torch.isnan(o.o32[b, skipped:T].float()).all()) and bool(torch.isnan(o.oa[b, skipped:T].float()).all()), "a tile past the length ran"
        assert bool(torch.isnan(o.o32[b, T:].float()).all()) and bool(torch.isnan(o.o32[b, :, cout:].float()).all())


@pytest.mark.parametrize("mode", ["bf16x3", "exact"])
def test_null_lens_is_todays_output_and_full_lengths_change_nothing(mode):
    from cosyvoice_amd import _lib as L
    cfg = CFGS["tiny"]
    m = _gen("tiny", mode=mode)
    B, T = 2, 24
    mel = torch.cat([_synth_mel(T, 1020 + b) for b in range(B)]).cuda()
    s = torch.cat([_synth_src(cfg, T, 1030 + b) for b in range(B)]).cuda()
    w0 = m.decode(mel, s).clone()
    ws = m._ws[(B, T)]
    desc = ws[("_desc", m.presplit)][0]
    assert not desc.lens
    desc.lens = None
    ws["wav"].zero_()
    L.check(L.lib().cv_hift_decode_enqueue(C.byref(desc), L.stream_ptr()), "cv_hift_decode_enqueue")
    assert torch.equal(ws["wav"], w0)
    m.length_bucket = T
    full = m.decode_ragged(mel, s, lengths=[T] * B)
    assert len(m._ws) == 1
    assert torch.equal(torch.stack(full), w0)


# ----------------------------------------------------------------------------- 7. orchestrator
def _model(max_batch=4):
    from cosyvoice_amd.flow import CausalMaskedDiffWithXvec
    from cosyvoice_amd.hift import HiFTGenerator
    from cosyvoice_amd.llm import Qwen2LM
    from cosyvoice_amd.model import CosyVoice2Model
    lc, fc, hc = LlmConfig.tiny(), FlowConfig.tiny(), HiftConfig.tiny()
    llm = Qwen2LM(lc, dtype=torch.bfloat16, max_batch=max_batch, ctx_max=256, max_out=256)
    flow = CausalMaskedDiffWithXvec(fc, dtype=torch.float16)
    hift = HiFTGenerator(hc, dtype=torch.float32)
    m = CosyVoice2Model(llm, flow, hift, fp16=False).load_state_dicts(llm_state_dict(lc), flow_state_dict(fc), _sd("tiny"))
    return m, lc, fc, hc


def _inputs(lc, fc, seed=0, n_text=6, n_p=10):
    g = torch.Generator().manual_seed(seed)
    return dict(text=torch.randint(0, lc.vocab_size, (1, n_text), generator=g, dtype=torch.int32),
                prompt_text=torch.randint(0, lc.vocab_size, (1, 4), generator=g, dtype=torch.int32),
                llm_prompt_speech_token=torch.randint(0, lc.speech_token_size, (1, n_p), generator=g, dtype=torch.int32),
                flow_prompt_speech_token=torch.randint(0, lc.speech_token_size, (1, n_p), generator=g, dtype=torch.int32),
                prompt_speech_feat=torch.clamp(torch.randn(1, 2 * n_p, 80, generator=g) * 2 - 6, -11.5, 2.0),
                flow_embedding=torch.randn(1, fc.spk_embed_dim, generator=g))


def _pin_source_randoms(m, hc, monkeypatch):
    """The vocoder draws its source randoms for the shape it runs at, so a padded batch and a batch-1 loop draw different numbers.  Give
    every utterance the same position-indexed phases and noise instead: what remains is the arithmetic."""
    nh, up = hc.nb_harmonics + 1, hc.total_upsample
    g = torch.Generator().manual_seed(123)
    pv = ((torch.rand(1, nh, generator=g) * 2 - 1) * 3.14159).cuda()
    nz = torch.randn(1, nh, 256 * up, generator=g).cuda()
    orig = m.hift.source

    def source(f0, phase_vec=None, noise=None):
        Bq, Tq = f0.shape
        return orig(f0, pv.expand(Bq, -1), nz[:, :, :Tq * up].expand(Bq, -1, -1))
    monkeypatch.setattr(m.hift, "source", source)


def _count_vocoder_calls(monkeypatch):
    from cosyvoice_amd import _lib as L
    real = L.lib().cv_hift_decode_enqueue
    calls = []

    def wrapper(desc, stream):
        calls.append(1)
        return real(desc, stream)
    monkeypatch.setattr(L.lib(), "cv_hift_decode_enqueue", wrapper)
    return calls


def test_tts_batch_ragged_vocoder_equals_per_utterance_loop(monkeypatch):
    m, lc, fc, hc = _model()
    _pin_source_randoms(m, hc, monkeypatch)
    calls = _count_vocoder_calls(monkeypatch)
    ins = [_inputs(lc, fc, seed=s) for s in range(3)]
    shared, B = ins[0], 3
    g = torch.Generator().manual_seed(9)
    forced = [torch.randint(0, lc.speech_token_size, (n,), generator=g).tolist() for n in (14, 9, 17)]
    args = ([i["text"] for i in ins], [shared["prompt_text"]] * B, [shared["llm_prompt_speech_token"]] * B,
            shared["flow_prompt_speech_token"].expand(B, -1), shared["prompt_speech_feat"].expand(B, -1, -1), shared["flow_embedding"].expand(B, -1))
    assert m.ragged_hift
    for to_host in (True, False):
        del calls[:]
        got = m.tts_batch(*args, forced=forced, to_host=to_host)
        assert isinstance(got, list) and len(calls) == 1                # one vocoder launch sequence for the group
        got = [w.cpu().clone() for w in got]
        m.ragged_hift = False
        del calls[:]
        ref = [w.cpu().clone() for w in m.tts_batch(*args, forced=forced, to_host=to_host)]
        m.ragged_hift = True
        assert len(calls) == B
        for w, r, f in zip(got, ref, forced):
            assert w.shape == r.shape == (2 * hc.total_upsample * len(f),)
            assert torch.isfinite(w).all() and w.abs().max().item() > 0
            assert (w - r).abs().max().item() < 1e-6


@pytest.mark.parametrize("cu_slots,fm,to_host,overlap", [(0, 1, True, False), (0, 1, False, False), (8, 1, True, False), (8, 1, False, True),
                                                         (8, 2, True, True), (8, 2, False, False)])
def test_tts_batches_ragged_vocoder_equals_per_utterance_loop(monkeypatch, cu_slots, fm, to_host, overlap):
    m, lc, fc, hc = _model()
    _pin_source_randoms(m, hc, monkeypatch)
    calls = _count_vocoder_calls(monkeypatch)
    B, nb = 2, 4
    shared = _inputs(lc, fc, seed=0)
    all_forced = []

    def batches():
        out = []
        for i in range(nb):
            ins = [_inputs(lc, fc, seed=10 * i + s) for s in range(B)]
            g = torch.Generator().manual_seed(100 + i)
            forced = [torch.randint(0, lc.speech_token_size, (n,), generator=g).tolist() for n in (8 + 3 * i, 15 - 2 * i)]
            all_forced.append(forced)
            out.append(dict(texts=[x["text"].cuda() for x in ins], prompt_texts=[shared["prompt_text"].cuda()] * B,
                            llm_prompt_speech_tokens=[shared["llm_prompt_speech_token"].cuda()] * B,
                            flow_prompt_speech_tokens=shared["flow_prompt_speech_token"].cuda().expand(B, -1),
                            prompt_speech_feats=shared["prompt_speech_feat"].cuda().expand(B, -1, -1),
                            flow_embeddings=shared["flow_embedding"].cuda().expand(B, -1), forced=forced))
        return out

    m.flow_merge, m.overlap_hift = fm, overlap
    run = lambda: [[w.cpu().clone() for w in ws] for ws in m.tts_batches(batches(), to_host=to_host, llm_cu_slots=cu_slots, llm_loops=2)]
    got = run()
    n_ragged = len(calls)
    m.ragged_hift = False
    del calls[:]
    ref = run()
    assert len(got) == len(ref) == nb
    # one vocoder launch sequence per flow group (flow_merge = 1: per batch; merged groups form when tokens are ready: at most one per batch)
    assert (n_ragged == nb) if fm == 1 else (nb // fm <= n_ragged <= nb), n_ragged
    assert len(calls) >= n_ragged * B if fm == 1 else len(calls) > n_ragged
    for i in range(nb):
        assert len(got[i]) == len(ref[i]) == B
        for w, r, f in zip(got[i], ref[i], all_forced[i]):
            assert w.shape == r.shape == (2 * hc.total_upsample * len(f),)
            assert torch.isfinite(w).all() and w.abs().max().item() > 0
            assert (w - r).abs().max().item() < 1e-6
