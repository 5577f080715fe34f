"""GPU: speaker embedding (Kaldi fbank + CAM++) on the device against the CPU restatement (tests/speaker_ref.py), the reference
goldens (tests/golden/campplus_*.npz), torch fp32 per kernel, and its ragged-batch / graph-replay bit-identity contracts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speaker_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from cosyvoice_amd.speaker import CAMPPlus
    from cosyvoice_amd.weights import campplus_state_dict
    return CAMPPlus().load_state_dict(campplus_state_dict())


def _conv(x, T_in, F_in, cin, w, T_out, F_out, B, **kw):
    """cv_spk_conv on contiguous [B][T][F][C] tensors; returns y (B, T_out, F_out, N)."""
    from cosyvoice_amd.speaker import CAMPPlus
    N = w.shape[0]
    y = torch.full((B, T_out, F_out, N), float("nan"), device="cuda")
    CAMPPlus._conv(x, T_in * F_in * cin, cin, T_in, F_in, cin, w, y, T_out * F_out * N, N, T_out, F_out, B, **kw)
    return y


def test_fbank_matches_restatement():
    from cosyvoice_amd.speaker import KaldiFbank
    fb = KaldiFbank()
    lens = (400, 401, 16000, 160000, 480000)
    waves = [R.test_signal(S, seed=i) for i, S in enumerate(lens)]
    for w in waves:
        feat, n = fb(w.unsqueeze(0))
        ref = R.kaldi_fbank(w)
        assert int(n[0]) == ref.shape[0] == feat.shape[1]
        assert (feat[0].cpu().double() - ref).abs().max().item() <= 1e-3
    feat, n = fb([waves[1], waves[3], waves[2]])          # one ragged batch of 3
    for row, w in enumerate([waves[1], waves[3], waves[2]]):
        ref = R.kaldi_fbank(w)
        assert int(n[row]) == ref.shape[0]
        assert (feat[row, :ref.shape[0]].cpu().double() - ref).abs().max().item() <= 1e-3
        assert torch.all(feat[row, ref.shape[0]:] == 0)


@pytest.mark.parametrize("cin,stride,shortcut", [(1, 1, False), (32, 2, False), (32, 1, True), (32, 2, True)])
def test_conv3x3_against_torch(cin, stride, shortcut):
    from cosyvoice_amd.speaker import _pad_k
    g = torch.Generator().manual_seed(cin + stride)
    B, Fi, T = 2, 40, 37
    lens = [37, 21]
    Fo = Fi // stride
    x = torch.randn(B, T, Fi, cin, generator=g)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    w = torch.randn(32, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    bias = torch.randn(32, generator=g) * 0.1
    res = torch.randn(B, T, Fo, 32, generator=g) if shortcut else None
    wp = _pad_k(w.permute(0, 2, 3, 1).reshape(32, 9 * cin)).contiguous()
    L = torch.tensor(lens, dtype=torch.int32).cuda()
    y = _conv(x.cuda(), T, Fi, cin, wp.cuda(), T, Fo, B, k=(3, 3), s=(stride, 1), pad=(1, 1), in_len=L, out_len=L, bias=bias.cuda(),
              res=None if res is None else res.cuda().contiguous(), relu=True).cpu()
    for b, n in enumerate(lens):
        xin = x[b:b + 1, :n].permute(0, 3, 2, 1)                      # (1, cin, F, T)
        ref = F.conv2d(xin, w, bias, stride=(stride, 1), padding=1).permute(0, 3, 2, 1)[0]   # (T, Fo, 32)
        if res is not None:
            ref = ref + res[b, :n]
        ref = F.relu(ref)
        assert (y[b, :n] - ref).abs().max().item() <= 1e-4
        assert torch.all(y[b, n:] == 0)


def test_prologue_bn_gemm_and_partial_sums():
    g = torch.Generator().manual_seed(3)
    B, T, Cb, cin = 3, 203, 192, 160
    lens = [203, 100, 7]
    x = torch.randn(B, T, Cb, generator=g)
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    w = torch.randn(128, cin, generator=g) / cin ** 0.5
    bias = torch.randn(128, generator=g) * 0.1
    L = torch.tensor(lens, dtype=torch.int32).cuda()
    from cosyvoice_amd.speaker import CAMPPlus
    y = torch.full((B, T, 128), float("nan"), device="cuda")
    G = (T + 3) // 4
    ps = torch.full((B, G, 128), float("nan"), device="cuda")
    CAMPPlus._conv(x.cuda(), T * Cb, Cb, T, 1, cin, w.cuda(), y, T * 128, 128, T, 1, B, pre=(sc.cuda(), sh.cuda()), bias=bias.cuda(),
                   relu=True, in_len=L, out_len=L, psum=ps, psum_bs=G * 128)
    y, ps = y.cpu(), ps.cpu()
    for b, n in enumerate(lens):
        ref = F.relu(F.relu(x[b, :n, :cin] * sc + sh) @ w.T + bias)
        assert (y[b, :n] - ref).abs().max().item() <= 1e-4
        assert torch.all(y[b, n:] == 0)
        full = torch.cat([ref, torch.zeros(4 * G - n, 128)]).reshape(G, 4, 128).sum(1)
        assert (ps[b] - full).abs().max().item() <= 1e-4


@pytest.mark.parametrize("T", [57, 100, 250])
def test_cam_gate_and_gated_dilated_conv(T):
    g = torch.Generator().manual_seed(T)
    B = 2
    lens = [T, max(T - 31, 3)]
    h = F.relu(torch.randn(B, T, 128, generator=g))
    for b, n in enumerate(lens):
        h[b, n:] = 0
    G = (T + 3) // 4
    ps = torch.cat([h, torch.zeros(B, 4 * G - T, 128)], 1).reshape(B, G, 4, 128).sum(2)
    w1, b1 = torch.randn(64, 128, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1
    w2, b2 = torch.randn(32, 64, generator=g) * 0.2, torch.randn(32, generator=g) * 0.1
    nseg = (T + 99) // 100
    gate = torch.full((B, nseg, 32), float("nan"), device="cuda")
    L = torch.tensor(lens, dtype=torch.int32).cuda()
    from cosyvoice_amd import _lib as Lb
    d = [t.cuda().contiguous() for t in (ps, w1, b1, w2, b2)]
    st = Lb.stream_ptr()
    Lb.check(Lb.lib().cv_spk_cam_gate(C.c_void_p(d[0].data_ptr()), C.c_int64(G * 128), C.c_void_p(L.data_ptr()), B, T, 100,
                                      *[C.c_void_p(t.data_ptr()) for t in d[1:]], C.c_void_p(gate.data_ptr()), C.c_int64(nseg * 32), st),
             "cv_spk_cam_gate")
    dil = 2
    wl = torch.randn(32, 128, 3, generator=g) / 20
    wp = wl.permute(0, 2, 1).reshape(32, 384).contiguous()
    y = _conv(h.cuda(), T, 1, 128, wp.cuda(), T, 1, B, k=(1, 3), pad=(0, dil), dt=dil, in_len=L, out_len=L, gate=gate,
              gate_bs=nseg * 32)[:, :, 0].cpu()
    for b, n in enumerate(lens):
        hb = h[b:b + 1, :n].transpose(1, 2)                      # (1, 128, n)
        ctx = hb.mean(-1, keepdim=True) + R._seg_mean(hb)
        m = torch.sigmoid(F.conv1d(F.relu(F.conv1d(ctx, w1[:, :, None], b1)), w2[:, :, None], b2))   # (1, 32, n)
        ref = (F.conv1d(hb, wl, padding=dil, dilation=dil) * m)[0].T
        assert (y[b, :n] - ref).abs().max().item() <= 1e-4
        assert torch.all(y[b, n:] == 0)


def test_stats_pool_ragged():
    g = torch.Generator().manual_seed(5)
    B, T, Cc = 3, 131, 512
    lens = [131, 2, 64]
    x = torch.randn(B, T, Cc, generator=g)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    out = torch.full((B, 2 * Cc), float("nan"), device="cuda")
    L = torch.tensor(lens, dtype=torch.int32).cuda()
    from cosyvoice_amd import _lib as Lb
    xd, scd, shd = x.cuda(), sc.cuda(), sh.cuda()
    Lb.check(Lb.lib().cv_spk_stats_pool(C.c_void_p(xd.data_ptr()), C.c_int64(T * Cc), Cc, C.c_void_p(L.data_ptr()), B, T, Cc,
                                        C.c_void_p(scd.data_ptr()), C.c_void_p(shd.data_ptr()), C.c_void_p(out.data_ptr()),
                                        C.c_int64(2 * Cc), Lb.stream_ptr()), "cv_spk_stats_pool")
    out = out.cpu()
    for b, n in enumerate(lens):
        v = F.relu(x[b, :n] * sc + sh)
        ref = torch.cat([v.mean(0), v.std(0, unbiased=True)])
        assert (out[b] - ref).abs().max().item() <= 1e-4


def test_campplus_matches_reference_goldens(model, golden_dir):
    for T in (150, 998):
        z = np.load(os.path.join(golden_dir, f"campplus_t{T}.npz"))
        e = model(torch.from_numpy(z["feat"])).cpu()
        ref = torch.from_numpy(z["embedding"])
        assert (e - ref).abs().max().item() <= 1e-4, T
        assert F.cosine_similarity(e, ref).item() >= 0.99999


def test_extract_spk_embedding_matches_cpu_chain(model):
    from cosyvoice_amd.weights import campplus_state_dict
    from cosyvoice_amd.speaker import extract_spk_embedding
    sd = campplus_state_dict()
    w = R.test_signal(48000, seed=7)
    e = extract_spk_embedding(model, w.unsqueeze(0))
    assert e.shape == (1, 192) and e.is_cuda
    ref = R.extract_spk_embedding(sd, w)
    assert (e.cpu() - ref).abs().max().item() <= 1e-3


def test_ragged_batch_rows_bit_identical_and_graph_equals_eager(model):
    waves = [R.test_signal(S, seed=10 + i) for i, S in enumerate((8000, 48000, 160000, 480000))]
    batch = model.extract_spk_embedding(waves)
    assert batch.shape == (4, 192)
    for i, w in enumerate(waves):
        alone = model.extract_spk_embedding(w)
        assert torch.equal(batch[i:i + 1], alone), i
    eager = model.extract_spk_embedding(waves, graph=False)
    assert torch.equal(eager, batch)
    n = model.num_launches(("wave", 4, 480000))
    assert n is not None and 150 <= n <= 200


def test_reload_changes_results():
    from cosyvoice_amd.speaker import CAMPPlus
    from cosyvoice_amd.weights import campplus_state_dict
    z = torch.from_numpy(np.load(os.path.join(os.path.dirname(__file__), "golden", "campplus_t150.npz"))["feat"])
    m = CAMPPlus().load_state_dict(campplus_state_dict())
    a = m(z).cpu()
    sd2 = campplus_state_dict(seed=7)
    m.load_state_dict(sd2)
    b = m(z).cpu()
    ref2 = R.campplus(sd2, z)
    assert not torch.equal(a, b)
    assert (b - ref2).abs().max().item() <= 1e-4


def test_campplus_session_contract(model, golden_dir):
    from cosyvoice_amd.speaker import CampplusSession
    sess = CampplusSession(model)
    name = sess.get_inputs()[0].name
    z = np.load(os.path.join(golden_dir, "campplus_t150.npz"))
    feat_btf = np.ascontiguousarray(np.concatenate([z["feat"], z["feat"]]).transpose(0, 2, 1))   # (2, T, 80) as the ONNX model takes
    out = sess.run(None, {name: feat_btf})
    assert isinstance(out, list) and len(out) == 1
    assert isinstance(out[0], np.ndarray) and out[0].shape == (2, 192) and out[0].dtype == np.float32
    assert np.abs(out[0] - z["embedding"]).max() <= 1e-4
    emb = torch.tensor([out[0][:1].flatten().tolist()])        # frontend.py:97-99
    assert emb.shape == (1, 192)


def test_too_short_inputs_raise(model):
    with pytest.raises(ValueError):
        model.extract_spk_embedding(torch.zeros(399))
    with pytest.raises(ValueError):
        model.extract_spk_embedding(torch.randn(400 + 160))        # 2 frames -> 1 TDNN frame
    with pytest.raises(ValueError):
        model(torch.randn(1, 80, 2))
