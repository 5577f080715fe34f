"""GPU: cv_gemm / cv_layernorm through the C ABI against plain torch fp32 references of the same op."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402
from _helpers import unsplit as _unsplit  # noqa: E402

pytestmark = pytest.mark.gpu

DTS = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(1000, 256, 256), (128, 1536, 256), (77, 80, 256), (2256, 4864, 896), (300, 18, 448)])
def test_linear_epilogues(dt, M, N, K):
    from cosyvoice_amd import ops
    torch.manual_seed(0)
    dev = "cuda"
    x = torch.randn(M, K, device=dev).to(dt)
    W = (torch.randn(N, K, device=dev) / K ** 0.5).to(dt)
    bias = torch.randn(N, device=dev)
    res = torch.randn(M, N, device=dev)
    ref = x.float() @ W.float().t() + bias + res
    o32 = torch.empty(M, N, device=dev)
    oa = torch.empty(M, N, device=dev, dtype=dt)
    ops.linear(x, W, bias=bias, res=res, act=ops.ACT_GELU, out_f32=o32, out_act=oa)
    torch.cuda.synchronize()
    assert _rel(o32, ref) < TOL[dt] * 0.5 + 1e-6
    assert _rel(oa, F.gelu(ref)) < TOL[dt]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cin,Cout,k,dil,T", [(256, 256, 3, 1, 500), (64, 64, 11, 5, 3000), (320, 256, 3, 1, 333), (96, 512, 7, 1, 200)])
def test_conv1d_channels_last(dt, Cin, Cout, k, dil, T):
    from cosyvoice_amd import ops
    torch.manual_seed(1)
    dev = "cuda"
    B = 2
    x = torch.randn(B, T, Cin, device=dev).to(dt)
    w = (torch.randn(Cout, Cin, k, device=dev) / (Cin * k) ** 0.5).to(dt)
    bias = torch.randn(Cout, device=dev)
    alpha = torch.rand(Cout, device=dev) + 0.5
    pad = (k * dil - dil) // 2
    ref = F.conv1d(x.float().transpose(1, 2), w.float(), bias, dilation=dil, padding=pad).transpose(1, 2)
    Wp = w.permute(0, 2, 1).reshape(Cout, k * Cin).contiguous()
    o32 = torch.empty(B, T, Cout, device=dev)
    oa = torch.empty(B, T, Cout, device=dev, dtype=dt)
    ops.conv1d_cl(x, Wp, k, dilation=dil, pad_left=pad, bias=bias, act=ops.ACT_SNAKE, act_param=alpha, out_f32=o32, out_act=oa)
    torch.cuda.synchronize()
    assert _rel(o32, ref) < TOL[dt] * 0.5 + 1e-6
    sn = ref + (1.0 / (alpha + 1e-9)) * torch.sin(ref * alpha) ** 2
    assert _rel(oa, sn) < TOL[dt]
    # causal variant (left pad k-1), as CausalConv1d flow/decoder.py:59-85
    refc = F.conv1d(F.pad(x.float().transpose(1, 2), ((k - 1) * dil, 0)), w.float(), bias, dilation=dil).transpose(1, 2)
    ops.conv1d_cl(x, Wp, k, dilation=dil, pad_left=(k - 1) * dil, bias=bias, out_f32=o32)
    torch.cuda.synchronize()
    assert _rel(o32, refc) < TOL[dt] * 0.5 + 1e-6


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_qkv_split_mode(dt):
    from cosyvoice_amd import ops
    torch.manual_seed(2)
    dev = "cuda"
    B, T, C, H = 2, 200, 256, 8
    Tp = 208
    x = torch.randn(B, T, C, device=dev).to(dt)
    W = (torch.randn(3 * H * 64, C, device=dev) / C ** 0.5).to(dt)
    q = torch.zeros(B, T, H * 64, device=dev, dtype=dt)
    k = torch.zeros(B, T, H * 64, device=dev, dtype=dt)
    vt = torch.zeros(B, H, 64, Tp, device=dev, dtype=dt)
    ops.gemm(x, W, T, 3 * H * 64, C, batch=B, a_bs=(T * C, 0), lda=C, out_act=q, oa_bs=(T * H * 64, 0), ldoa=H * 64,
             qkv=dict(q_cols=H * 64, k_cols=H * 64, q_scale=0.125, k_out=k, k_bs=T * H * 64, ldk=H * 64, vt_out=vt,
                      vt_heads=H, vt_ld=Tp))
    torch.cuda.synchronize()
    ref = x.float() @ W.float().t()
    assert _rel(q, ref[..., :512] * 0.125) < TOL[dt]
    assert _rel(k, ref[..., 512:1024]) < TOL[dt]
    vref = ref[..., 1024:].reshape(B, T, H, 64).permute(0, 2, 3, 1)
    assert _rel(vt[..., :T], vref) < TOL[dt]


@pytest.mark.parametrize("odt", DTS)
@pytest.mark.parametrize("rows,dim,rms", [(1000, 256, False), (37, 512, False), (16, 896, True)])
def test_layernorm(odt, rows, dim, rms):
    from cosyvoice_amd import ops
    torch.manual_seed(3)
    dev = "cuda"
    x = torch.randn(rows, dim, device=dev) * 3 + 1
    g = torch.randn(dim, device=dev)
    b = None if rms else torch.randn(dim, device=dev)
    if rms:
        ref = g * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6))
    else:
        ref = F.layer_norm(x, (dim,), g, b, 1e-5)
    o32 = torch.empty(rows, dim, device=dev)
    oa = torch.empty(rows, dim, device=dev, dtype=odt)
    ops.layernorm(x, g, b, 1e-6 if rms else 1e-5, rms=rms, out_f32=o32, out_act=oa)
    torch.cuda.synchronize()
    assert (o32 - ref).abs().max().item() < 2e-5 * ref.abs().max().item() + 1e-5
    assert _rel(oa, ref) < {torch.float32: 1e-6, torch.bfloat16: 5e-3, torch.float16: 6e-4}[odt]


@pytest.mark.parametrize("odt", DTS)
@pytest.mark.parametrize("act", ["NONE", "MISH"])
@pytest.mark.parametrize("rpg", [1, 37])
@pytest.mark.parametrize("dim", [80, 256, 1024])
def test_layernorm_modes(dim, rpg, act, odt):
    """add with rows_per_group 1 and T, act = MISH, out_scale != 1, ldx / add_ld / ldo > dim, rows with a large common offset
    (x = 1000 + N(0, 1)), against F.layer_norm in float64; test_layernorm's bounds.  The kernel adds the group vector AFTER the activation
    (CausalBlock1D's Mish, then the time embedding).  Outputs are pre-filled with NaN; the input's padding columns hold NaN."""
    from cosyvoice_amd import ops
    scale = 0.5
    x, g, b, add, ref = H.layernorm_case(dim, rpg, act, scale, torch.float64)
    rows = x.shape[0]
    xin, addin = H.nan_like((rows + 2, dim + 8), torch.float32), H.nan_like((add.shape[0], dim + 12), torch.float32)
    xin[:rows, :dim], addin[:, :dim] = x.cuda(), add.cuda()
    o32, oa = H.nan_like((rows + 2, dim + 4), torch.float32), H.nan_like((rows + 2, dim + 8), odt)
    ops.layernorm(xin[:rows, :dim], g.cuda(), b.cuda(), 1e-5, add=addin[:, :dim], rows_per_group=rpg, act=getattr(ops, "ACT_" + act),
                  out_scale=scale, out_f32=o32[:rows, :dim], out_act=oa[:rows, :dim])
    torch.cuda.synchronize()
    o32, oa = o32.cpu(), oa.cpu()
    for o in (o32, oa):
        assert bool(torch.isnan(o[rows:].float()).all()) and bool(torch.isnan(o[:, dim:].float()).all()), "layernorm wrote outside (rows, dim)"
    err = (o32[:rows, :dim].double() - ref).abs().max().item()
    assert err < 2e-5 * ref.abs().max().item() + 1e-5, f"max|err| {err:.3e}, max|ref| {ref.abs().max().item():.3e}"
    rel = ((oa[:rows, :dim].double() - ref).norm() / ref.norm()).item()
    assert rel < {torch.float32: 1e-6, torch.bfloat16: 5e-3, torch.float16: 6e-4}[odt], f"relative L2 {rel:.3e}"


@pytest.mark.parametrize("odt", DTS)
@pytest.mark.parametrize("mode", ["ln", "leaky", "rms", "plain"])
@pytest.mark.parametrize("dim", [1028, 2048])
def test_layernorm_wide_leaky_rms_and_null_affine(dim, mode, odt):
    """dim above 1024 (norm_kernel<., 8>: 1028 = 257 float4, one past four per lane, and the limit 2048); CV_ACT_LEAKY, which is ReLU in this
    kernel; RMSNorm with a null beta; LayerNorm with null gamma and beta.  Rows x = 1000 + N(0, 1) for the LayerNorm modes, 3 N(0, 1) + 1 for
    RMS; float64 reference; test_layernorm_modes' bounds, buffers and add (after the activation, one vector per row group)."""
    from cosyvoice_amd import ops
    g_ = torch.Generator().manual_seed(dim + len(mode))
    rows, rpg, scale = 37, 5, 0.5
    rms = mode == "rms"
    x = torch.randn(rows, dim, generator=g_) * 3 + 1 if rms else 1000.0 + torch.randn(rows, dim, generator=g_)
    g = None if mode == "plain" else torch.randn(dim, generator=g_)
    b = None if mode in ("plain", "rms") else torch.randn(dim, generator=g_)
    add = torch.randn((rows + rpg - 1) // rpg, dim, generator=g_)
    xd = x.double()
    if rms:
        y = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + torch.tensor(1e-6, dtype=torch.float32).double()) * g.double()
    else:
        y = F.layer_norm(xd, (dim,), None if g is None else g.double(), None if b is None else b.double(), 1e-5)
    if mode == "leaky":
        y = F.relu(y)
    ref = (y + add.double().repeat_interleave(rpg, 0)[:rows]) * scale
    xin, addin = H.nan_like((rows + 2, dim + 8), torch.float32), H.nan_like((add.shape[0], dim + 12), torch.float32)
    xin[:rows, :dim], addin[:, :dim] = x.cuda(), add.cuda()
    o32, oa = H.nan_like((rows + 2, dim + 4), torch.float32), H.nan_like((rows + 2, dim + 8), odt)
    ops.layernorm(xin[:rows, :dim], None if g is None else g.cuda(), None if b is None else b.cuda(), 1e-6 if rms else 1e-5, rms=rms,
                  add=addin[:, :dim], rows_per_group=rpg, act=ops.ACT_LEAKY if mode == "leaky" else ops.ACT_NONE, out_scale=scale,
                  out_f32=o32[:rows, :dim], out_act=oa[:rows, :dim])
    torch.cuda.synchronize()
    o32, oa = o32.cpu(), oa.cpu()
    for o in (o32, oa):
        assert bool(torch.isnan(o[rows:].float()).all()) and bool(torch.isnan(o[:, dim:].float()).all()), "layernorm wrote outside (rows, dim)"
    err = (o32[:rows, :dim].double() - ref).abs().max().item()
    assert err < 2e-5 * ref.abs().max().item() + 1e-5, f"max|err| {err:.3e}, max|ref| {ref.abs().max().item():.3e}"
    rel = ((oa[:rows, :dim].double() - ref).norm() / ref.norm()).item()
    assert rel < {torch.float32: 1e-6, torch.bfloat16: 5e-3, torch.float16: 6e-4}[odt], f"relative L2 {rel:.3e}"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_tall_gemm_tile_plain_and_swiglu(dt):
    """>= 8192 rows with N, K >= 512 take the 8-wave 128 x 128 tile (the LLM prefill of a 4-batch decode job): plain epilogue with a
    residual, and the SwiGLU epilogue over [gate16 | up16]-interleaved weights (the prefill's gate/up GEMM)."""
    from cosyvoice_amd import ops
    torch.manual_seed(1)
    dev, M, K, I = "cuda", 9024, 896, 1024
    x = (torch.randn(M, K, device=dev) * 0.5).to(dt)
    W = (torch.randn(896, K, device=dev) / K ** 0.5).to(dt)
    res = torch.randn(M, 896, device=dev)
    o32 = torch.empty(M, 896, device=dev)
    ops.linear(x, W, res=res, out_f32=o32)
    g = (torch.randn(I, K, device=dev) / K ** 0.5).to(dt)
    u = (torch.randn(I, K, device=dev) / K ** 0.5).to(dt)
    gu = torch.stack([g.view(I // 16, 16, K), u.view(I // 16, 16, K)], dim=1).reshape(2 * I, K).contiguous()
    h = torch.empty(M, I, device=dev, dtype=dt)
    ops.linear(x, gu, act=ops.ACT_SWIGLU, out_act=h)
    torch.cuda.synchronize()
    assert _rel(o32, x.float() @ W.float().t() + res) < TOL[dt] * 0.5
    assert _rel(h, F.silu(x.float() @ g.float().t()) * (x.float() @ u.float().t())) < TOL[dt]


@pytest.mark.parametrize("shape", ["auto", "4x1", "2x2", "2x1", "1x2", "1x1"])
@pytest.mark.parametrize("Cin,Cout,k,dil,T,B", [(64, 64, 3, 1, 1000, 2), (64, 64, 11, 5, 777, 1), (128, 128, 7, 3, 601, 2),
                                                (256, 256, 11, 5, 500, 1), (256, 256, 3, 1, 130, 3), (128, 64, 7, 1, 70, 2), (64, 192, 3, 3, 257, 1)])
def test_conv_window_kernel_presplit(Cin, Cout, k, dil, T, B, shape):
    """conv_win_kernel (stride-1 bf16x3 convs on pre-split operands: activation window in LDS, weights streamed L2 -> VGPR) against torch
    fp32, and against gemm_kernel on the same launch (the default; the window kernel is opt-in, cv_gemm_params.conv_win): both the fp32 output and the pre-split snake output, every
    workgroup shape, ragged row / column tails, zero padding on both sides, residual + scale epilogue."""
    from cosyvoice_amd import ops, _lib as L
    from cosyvoice_amd.hift import _presplit
    torch.manual_seed(11)
    dev = "cuda"
    x = torch.randn(B, T, Cin)
    w = torch.randn(Cout, Cin, k) / (Cin * k) ** 0.5
    bias = torch.randn(Cout, device=dev)
    alpha = torch.rand(Cout, device=dev) + 0.5
    res = torch.randn(B, T, Cout, device=dev)
    pad = (k * dil - dil) // 2
    xs = _presplit(x.reshape(B * T, Cin)).view(torch.float32).reshape(B, T, Cin).to(dev)
    Wp = w.permute(0, 2, 1).reshape(Cout, k * Cin).contiguous()
    Ws = _presplit(Wp).view(torch.float32).to(dev)
    xv, wv = _unsplit(xs.cpu()).to(dev), _unsplit(Ws.cpu()).to(dev).reshape(Cout, k, Cin).permute(0, 2, 1)
    ref = (F.conv1d(xv.double().transpose(1, 2), wv.double(), bias.double(), dilation=dil, padding=pad).transpose(1, 2) + res.double()) * 0.5
    sn = ref + (1.0 / (alpha.double() + 1e-9)) * torch.sin(ref * alpha.double()) ** 2
    outs = {}
    code = 1 if shape == "auto" else 10 * int(shape[0]) + int(shape[2])   # conv_win: 1 = automatic shape, 10 WM + WN = forced
    for win in ("1", "0"):
        o32 = torch.full((B, T, Cout), float("nan"), device=dev)
        oa = torch.full((B, T, Cout), float("nan"), device=dev)
        ops.conv1d_cl(xs, Ws, k, dilation=dil, pad_left=pad, bias=bias, res=res, out_scale=0.5, act=ops.ACT_SNAKE, act_param=alpha,
                      out_f32=o32, out_act=oa, dtype=L.CV_F32X3, x3_flags=7, conv_win=code if win == "1" else 0)
        torch.cuda.synchronize()
        outs[win] = (o32.clone(), _unsplit(oa.cpu()).to(dev))
        # bf16x3 drops the lo*lo term: relative 2^-16 per product, fp32 accumulation
        assert (o32.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
        assert (outs[win][1].double() - sn).abs().max().item() < 5e-5 * max(1.0, sn.abs().max().item())
    d = (outs["1"][0] - outs["0"][0]).abs().max().item()
    assert d < 2e-6 * max(1.0, ref.abs().max().item())
    if Cin == 64:   # one channel chunk: same summation order as the K-tile loop
        assert torch.equal(outs["1"][0], outs["0"][0]) and torch.equal(outs["1"][1], outs["0"][1])
