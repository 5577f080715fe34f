"""GPU: cv_attention (flash, head_dim 64) against a plain torch fp32 softmax(QK^T)V reference."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref(q, k, v, scale, klen=None, chunk=0, causal=False, causal_off=0, bias=None):
    # q (B,H,Tq,64) k,v (B,Hkv,Tk,64) fp32
    B, H, Tq, _ = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    rep = H // Hkv
    kk = k.repeat_interleave(rep, 1)
    vv = v.repeat_interleave(rep, 1)
    s = torch.matmul(q, kk.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias
    i = torch.arange(Tq, device=q.device)[:, None]
    j = torch.arange(Tk, device=q.device)[None, :]
    ok = torch.ones(Tq, Tk, dtype=torch.bool, device=q.device)
    if causal:
        ok &= j <= i + causal_off
    if chunk:
        ok &= j < (i // chunk + 1) * chunk
    ok = ok[None, None].expand(B, H, Tq, Tk).clone()
    if klen is not None:
        ok &= (j[None, None] < klen[:, None, None, None])
    s = s.masked_fill(~ok, float("-inf"))
    return torch.matmul(torch.softmax(s, -1), vv)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,Hkv,Tq,Tk,mode", [
    (2, 8, 8, 500, 500, "plain"), (2, 8, 8, 130, 130, "klen"), (1, 8, 8, 200, 200, "chunk"),
    (2, 14, 2, 107, 107, "causal"), (1, 8, 8, 100, 100, "bias"), (1, 4, 4, 1000, 1000, "plain"),
])
@pytest.mark.parametrize("waves", ["4", "2"])
@pytest.mark.parametrize("mfma", ["64", "32", "16"])
def test_attention_vs_torch(dt, B, H, Hkv, Tq, Tk, mode, waves, mfma):
    """Both workgroup shapes (128 queries / 4 waves: the batch-8 grids; 64 queries / 2 waves: grids that would not fill the chip) and
    both MFMA forms (32x32x16: the default; 16x16x32: its cross-check)."""
    from cosyvoice_amd import ops
    torch.manual_seed(0)
    dev = "cuda"
    q = torch.randn(B, Tq, H * 64, device=dev).to(dt)
    k = torch.randn(B, Tk, Hkv * 64, device=dev).to(dt)
    v = torch.randn(B, Tk, Hkv * 64, device=dev).to(dt)
    Tp = (Tk + 63) // 64 * 64
    vt = torch.full((B, Hkv, 64, Tp), float("nan"), device=dev, dtype=dt)  # padding must not leak
    vt[..., :Tk] = v.view(B, Tk, Hkv, 64).permute(0, 2, 3, 1)
    out = torch.zeros(B, Tq, H * 64, device=dev, dtype=dt)
    kw = {}
    rkw = {}
    if mode == "klen":
        kl = torch.tensor([Tk, Tk - 37], device=dev, dtype=torch.int32)
        kw["klen"] = kl
        rkw["klen"] = kl
    if mode == "chunk":
        kw["chunk"] = 50
        rkw["chunk"] = 50
    if mode == "causal":
        kw["causal"] = True
        rkw["causal"] = True
    bias = None
    if mode == "bias":
        raw = torch.randn(B, H, Tq, 2 * Tq - 1, device=dev)
        # rel-shift view (attention.py:225-247): bias[i][j] = raw[i][Tq-1-i+j]
        kw.update(bias=raw.view(-1)[Tq - 1:], bias_bs=H * Tq * (2 * Tq - 1), bias_hs=Tq * (2 * Tq - 1), bias_ld=2 * Tq - 2)
        idx = (Tq - 1 - torch.arange(Tq, device=dev))[:, None] + torch.arange(Tq, device=dev)[None, :]
        rkw["bias"] = torch.gather(raw, 3, idx[None, None].expand(B, H, Tq, Tq))
    scale = 1.0 / math.sqrt(64)
    ops.attention(q, k, vt, out, B=B, H=H, Hkv=Hkv, Tq=Tq, Tk=Tk, scale=scale, q_bs=Tq * H * 64, ldq=H * 64,
                  k_bs=Tk * Hkv * 64, ldk=Hkv * 64, vt_ld=Tp, o_bs=Tq * H * 64, ldo=H * 64, mfma=int(mfma), waves=int(waves), **kw)
    torch.cuda.synchronize()
    ref = _ref(q.float().view(B, Tq, H, 64).transpose(1, 2), k.float().view(B, Tk, Hkv, 64).transpose(1, 2),
               v.float().view(B, Tk, Hkv, 64).transpose(1, 2), scale, **rkw).transpose(1, 2).reshape(B, Tq, H * 64)
    o = out.float()
    if mode == "klen":  # rows of the shorter sequence beyond its length are padding
        pass
    assert torch.isfinite(o).all()
    err = (o - ref).abs().max().item()
    assert err < (3e-2 if dt == torch.bfloat16 else 4e-3), err


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("mfma", ["64", "32", "16"])
def test_fully_masked_query_rows_are_zero(dt, with_bias, mfma):
    """A negative causal_off leaves the first queries without any visible key: those rows must come out as zeros (every masked
    score used to equal the running "max", so exp2(0) = 1 gave them mean(V) of the loaded tiles); the other rows are unaffected."""
    from cosyvoice_amd import ops
    torch.manual_seed(1)
    dev, B, H, T, off = "cuda", 1, 4, 150, -5
    q = torch.randn(B, T, H * 64, device=dev).to(dt)
    k = torch.randn(B, T, H * 64, device=dev).to(dt)
    v = torch.randn(B, T, H * 64, device=dev).to(dt)
    Tp = (T + 63) // 64 * 64
    vt = torch.zeros(B, H, 64, Tp, device=dev, dtype=dt)
    vt[..., :T] = v.view(B, T, H, 64).permute(0, 2, 3, 1)
    out = torch.full((B, T, H * 64), 7.0, device=dev, dtype=dt)
    kw, rkw = {}, {}
    if with_bias:
        bias = torch.randn(B, H, T, T, device=dev)
        kw.update(bias=bias, bias_bs=H * T * T, bias_hs=T * T, bias_ld=T)
        rkw["bias"] = bias
    scale = 0.125
    ops.attention(q, k, vt, out, B=B, H=H, Hkv=H, Tq=T, Tk=T, scale=scale, q_bs=T * H * 64, ldq=H * 64, k_bs=T * H * 64,
                  ldk=H * 64, vt_ld=Tp, o_bs=T * H * 64, ldo=H * 64, causal=True, causal_off=off, mfma=int(mfma), **kw)
    torch.cuda.synchronize()
    o = out.float()
    assert o[:, :-off].abs().max().item() == 0.0
    ref = _ref(q.float().view(B, T, H, 64).transpose(1, 2), k.float().view(B, T, H, 64).transpose(1, 2),
               v.float().view(B, T, H, 64).transpose(1, 2), scale, causal=True, causal_off=off, **rkw).transpose(1, 2).reshape(B, T, H * 64)
    err = (o[:, -off:] - ref[:, -off:]).abs().max().item()
    assert err < (3e-2 if dt == torch.bfloat16 else 4e-3), err


@pytest.mark.parametrize("dt,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("jump", [3.0, 7.5, 8.5, 40.0])
@pytest.mark.parametrize("mfma", ["64", "32", "16"])
def test_online_softmax_rescale_branch(dt, tol, jump, mfma):
    """The tile step rescales its output accumulators only when some query's running max moved (wave-uniform branch).  A rare,
    data-dependent branch needs an input that FORCES it at chosen tiles: one key per tile (3, 6, 9) whose score exceeds everything
    before it by 1, 2, 3 x `jump` log2 units, for one query of a wave only, against an fp64 full-tensor reference.  (A deferred-max form —
    keep the old max while growth stays below 2^8 — passed this test too but bought nothing on this kernel: 57.2 vs 56-58 us.)"""
    from cosyvoice_amd import ops
    torch.manual_seed(4)
    dev, B, H, T = "cuda", 1, 2, 640
    q = torch.randn(B, T, H * 64, device=dev) * 0.5
    k = torch.randn(B, T, H * 64, device=dev) * 0.5
    v = torch.randn(B, T, H * 64, device=dev)
    scale = 0.125
    # spikes: key j of tile (3, 6, 9) lines up with query rows 5, 37, 70 (different q-tiles / waves): score += jump / (scale * log2 e) per step
    for n, (jt, qi) in enumerate(((3, 5), (6, 37), (9, 70))):
        j = jt * 64 + 11
        for h in range(H):
            qv = q[0, qi, h * 64:(h + 1) * 64]
            want = (n + 1) * jump / (scale * 1.4426950408889634) + 6.0 / scale
            k[0, j, h * 64:(h + 1) * 64] = qv * (want / (qv @ qv))
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    vt = torch.zeros(B, H, 64, T, device=dev, dtype=dt)
    vt[:] = v.view(B, T, H, 64).permute(0, 2, 3, 1)
    out = torch.zeros(B, T, H * 64, device=dev, dtype=dt)
    ops.attention(q, k, vt, out, B=B, H=H, Hkv=H, Tq=T, Tk=T, scale=scale, q_bs=T * H * 64, ldq=H * 64, k_bs=T * H * 64, ldk=H * 64,
                  vt_ld=T, o_bs=T * H * 64, ldo=H * 64, mfma=int(mfma))
    torch.cuda.synchronize()
    f = lambda a: a.double().view(B, T, H, 64).permute(0, 2, 1, 3)
    ref = _ref(f(q), f(k), f(v), scale).permute(0, 2, 1, 3).reshape(B, T, H * 64)
    err = (out.double() - ref).abs().max().item()
    assert torch.isfinite(out).all() and err < tol, err
