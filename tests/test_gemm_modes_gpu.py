"""cv_gemm modes that tests/test_gemm_gpu.py never sets, each against a float64 torch reference of the same operation computed from the
already rounded operands: a_row_stride > 1 (strided conv), out_row_stride / out_row_off / out_rows with tap_step = -1 (ConvTranspose1d as
phase GEMMs, with the M = 1 reflect-pad launch), batch_inner with two-level a_bs / w_bs (rel-pos bias GEMM, odd N = scalar epilogue), res2,
out_scale, every cv_act but SWIGLU, CV_F32X3 with plain operands, x3_flags = 4 alone, K / tap tails and every tile the dispatcher picks.

dtype modes: f32, bf16, f16, x3 (CV_F32X3, plain fp32 operands), x3ps (CV_F32X3, pre-split operands, x3_flags = 3 or 7).
Bounds (tests/_helpers.py), element-wise, no allowance:
  out_f32: (n + 2) 2^-23 sum|terms| + half an fp32 ulp (+ 2^-16 sum|terms| for bf16x3), n = K + the bias / residual terms;
  out_act: the same bound times the activation's Lipschitz constant (GELU 1.13, SiLU 1.1, Mish 1.09, Snake 1 + |sin 2ax| <= 2, others 1)
           + 4 max(e32, 2^-23 |ref|) (e32 = L-inf error of torch's fp32 activation on the same pre-activation) + half an ulp of the
           output type; Snake also meets the cap that follows from sin_cw's 2e-7 claim.
Guards: outputs are pre-filled with NaN and only rows [0, out_rows) x columns [0, N) of each batch may change.  Leaks: NaN sits in guard
rows around every batch's a_rows (a_bs > a_rows * lda), in the columns [cin, lda) / [K, ldw), and in the parts of a shared buffer the
launch must not read.  The ``test_cpu_*`` functions (no gpu mark) check that torch's own fp32 evaluation meets the out_f32 bound."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

gpu = pytest.mark.gpu
MODES = ["f32", "bf16", "f16", "x3", "x3ps"]
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "x3": torch.float32, "x3ps": torch.float32}
F64 = torch.float64
G = 2   # NaN guard rows on each side of a batch's rows


def rvals(x, mode):
    """The values the kernel's operand storage stands for (fp32 tensor): 16-bit rounding, or hi + lo of the pre-split format."""
    x = x.float()
    if mode in ("bf16", "f16"):
        return x.to(DT[mode]).float()
    if mode == "x3ps":
        hi = x.to(torch.bfloat16).float()
        return hi + (x - hi).to(torch.bfloat16).float()
    return x


def dev_op(x, mode, ld):
    """x (..., R, C) fp32 on the CPU -> device view of the same shape in the mode's storage, row stride ld >= C, with G NaN guard rows
    before and after every block of R rows and NaN in the columns [C, ld)."""
    R, Cc = x.shape[-2:]
    shape = (*x.shape[:-2], R + 2 * G, ld)
    if mode == "x3ps":
        buf, st = H.nan_split(shape), H.presplit_f32(x)
    else:
        buf, st = H.nan_like(shape, DT[mode]), x.to(DT[mode])
    view = buf[..., G:G + R, :Cc]
    view.copy_(st.cuda())
    return view


def gkw(mode, out_split=False):
    from cosyvoice_amd import _lib as L
    if mode == "x3":
        return dict(dtype=L.CV_F32X3, x3_flags=4 if out_split else 0)
    if mode == "x3ps":
        return dict(dtype=L.CV_F32X3, x3_flags=7 if out_split else 3)
    return {}


def _ld(n):
    return (n + 7) // 8 * 8 + 8


class Outs:
    """NaN pre-filled out_f32 / out_act buffers (B, rows + G, ld > N) and the keyword arguments that point cv_gemm at them."""

    def __init__(self, mode, B, rows, N, want32=True, wantact=True, out_split=False):
        self.B, self.rows, self.N, self.mode, self.split = B, rows, N, mode, out_split
        self.ld32, self.lda = _ld(N), _ld(N) + 8
        self.o32 = H.nan_like((B, rows + G, self.ld32), torch.float32) if want32 else None
        self.oa = None
        if wantact:
            self.oa = H.nan_split((B, rows + G, self.lda)) if out_split else H.nan_like((B, rows + G, self.lda), DT[mode])

    def kw(self):
        k = {}
        if self.o32 is not None:
            k.update(out_f32=self.o32, o32_bs=(self.o32.stride(0), 0), ldo32=self.ld32)
        if self.oa is not None:
            k.update(out_act=self.oa, oa_bs=(self.oa.stride(0), 0), ldoa=self.lda)
        return k

    def _guards(self, name, t):
        nan = torch.isnan(t.float())
        assert bool(nan[:, self.rows:].all()), f"{name}: rows >= out_rows were written"
        assert bool(nan[:, :, self.N:].all()), f"{name}: columns [N, ld) were written"
        assert not bool(nan[:, :self.rows, :self.N].any()), f"{name}: NaN inside the output (a row was not written, or poison was read)"

    def check(self, name, v_ref, sabs, n, act="NONE", act_param=None, slope=0.0):
        """v_ref, sabs (B, rows, N) float64: the pre-activation value and sum|terms| (bias / residuals included)."""
        x3 = self.mode in ("x3", "x3ps")
        name = f"{name} [{self.mode}]"
        bv = H.sum_bound(n, sabs, v_ref, torch.float32, x3=x3)
        res = {}
        if self.o32 is not None:
            o = self.o32.cpu()
            self._guards(name + " out_f32", o)
            res["f32"] = H.check(name + " out_f32", o[:, :self.rows, :self.N], v_ref, bv)
        if self.oa is not None:
            raw = self.oa.cpu()
            o = H.unsplit(raw) if self.split else raw
            self._guards(name + " out_act", o)
            odt = "split" if self.split else DT[self.mode]
            ref = act64(act, v_ref, act_param, slope)
            if act == "NONE":
                b = H.sum_bound(n, sabs, v_ref, odt, x3=x3)
            else:
                e32 = (act64(act, v_ref.float(), act_param, slope).double() - ref).abs().max()
                b = H.ACT_LIPSCHITZ[act] * bv + H.act_bound(e32, ref, odt)
            res["act"] = H.check(f"{name} out_act{'(split)' if self.split else ''} {act}" + ("" if act == "NONE" else f" (e32 {e32.item():.2e})"), o[:, :self.rows, :self.N], ref, b)
            if act == "SNAKE":
                a = act_param.double()
                cap = 4.1e-7 / (a + 1e-9) + 2.0 ** -22 * torch.maximum(v_ref.abs(), ref.abs()) + 2.0 * bv + 0.5 * H.ulp(ref, odt)
                H.check(name + " out_act Snake cap", o[:, :self.rows, :self.N], ref, cap)
        return res


def act64(act, v, param=None, slope=0.0):
    """The activation in v's own precision (float64 reference, or torch's fp32 for e32)."""
    if act == "NONE":
        return v
    if act == "GELU":
        return F.gelu(v)
    if act == "SILU":
        return F.silu(v)
    if act == "MISH":
        return F.mish(v)
    if act == "LEAKY":
        return torch.where(v > 0, v, v * slope)
    if act == "ELU":
        return F.elu(v)
    if act == "TANH":
        return torch.tanh(v)
    if act == "SNAKE":
        a = param.to(v.dtype)
        return v + (1.0 / (a + 1e-9)) * torch.sin(v * a) ** 2
    raise KeyError(act)


def act_id(act):
    from cosyvoice_amd import ops
    return getattr(ops, "ACT_" + act)


def conv_ref(x, w, bias, dt, stride=1, dil=1, pad=(0, 0)):
    """x (B, T, cin), w (cout, cin, k) values -> (B, T_out, cout) conv and its sum|terms| evaluated in dt."""
    xt, wt = x.to(dt).transpose(1, 2), w.to(dt)
    y = F.conv1d(F.pad(xt, pad), wt, None if bias is None else bias.to(dt), stride=stride, dilation=dil).transpose(1, 2)
    s = F.conv1d(F.pad(xt.abs(), pad), wt.abs(), None if bias is None else bias.to(dt).abs(), stride=stride, dilation=dil).transpose(1, 2)
    return y, s


def pack_w(w):
    """(cout, cin, k) -> (cout, k * cin), k-index = tap * cin + ci."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


# ----------------------------------------------------------------------------- 1. strided conv (a_row_stride > 1)
def _strided_plans():
    from cosyvoice_amd.config import HiftConfig
    from cosyvoice_amd.weights import hift_downsample_plan
    ksp = {(k, s, p) for cfg in (HiftConfig.v2(), HiftConfig.v1()) for (s, k, p) in hift_downsample_plan(cfg)} | {(3, 2, 1)}
    return sorted(ksp)


def _strided_case(k, s, pad, mode):
    torch.manual_seed(k * 100 + s)
    B, cin, cout, T_out = 2, 24, 40, 77
    T = T_out * s + 1                       # not a multiple of the stride (s > 1)
    x = rvals(torch.randn(B, T, cin), mode)
    w = rvals(torch.randn(cout, cin, k) / (cin * k) ** 0.5, mode)
    bias = torch.randn(cout)
    return x, w, bias, T_out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,s,pad", _strided_plans())
def test_cpu_strided_conv_bound_holds_for_torch_fp32(k, s, pad, mode):
    x, w, bias, T_out = _strided_case(k, s, pad, mode)
    ref, sabs = conv_ref(x, w, bias, F64, stride=s, pad=(pad, pad))
    t32, _ = conv_ref(x, w, bias, torch.float32, stride=s, pad=(pad, pad))
    assert ref.shape[1] >= T_out
    H.check("torch fp32 strided conv", t32[:, :T_out], ref[:, :T_out], H.sum_bound(w.shape[1] * k + 1, sabs[:, :T_out], ref[:, :T_out], torch.float32))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,s,pad", _strided_plans())
def test_strided_conv(k, s, pad, mode):
    """ops.conv1d_cl(stride = s) = a_row_stride: the (k, s, pad) of HiFT's source_downs (v2: (30, 15, 7), (6, 3, 1), (1, 1, 0); v1: (16, 8, 4))
    and (3, 2, 1) (the v1 flow's down-sampling), explicit T_out, input length not a multiple of s."""
    from cosyvoice_amd import ops
    x, w, bias, T_out = _strided_case(k, s, pad, mode)
    B, T, cin = x.shape
    cout = w.shape[0]
    ref, sabs = conv_ref(x, w, bias, F64, stride=s, pad=(pad, pad))
    xd, wd = dev_op(x, mode, cin + 8), dev_op(pack_w(w), mode, k * cin + 8)
    o = Outs(mode, B, T_out, cout)
    ops.conv1d_cl(xd, wd, k, pad_left=pad, stride=s, T_out=T_out, bias=bias.cuda(), out_f32=o.o32[:, :T_out, :cout],
                  out_act=o.oa[:, :T_out, :cout], **gkw(mode))
    torch.cuda.synchronize()
    o.check(f"strided conv k={k} s={s}", ref[:, :T_out], sabs[:, :T_out], cin * k + 1)


# ----------------------------------------------------------------------------- 2. ConvTranspose1d as phase GEMMs
def _convt_case(u, k, cin, cout, t_in, off, mode):
    torch.manual_seed(u * 1000 + cin + t_in + off)
    B = 2
    x = rvals(torch.randn(B, t_in, cin), mode)
    w = rvals(torch.randn(cin, cout, k) / (cin * k / u) ** 0.5, mode)
    bias = torch.randn(cout)
    t_out = t_in * u + off
    res = torch.randn(B, t_out, cout)
    return x, w, bias, res, t_out


def _convt_ref(x, w, bias, res, u, k, off, dt):
    xt, wt, b = x.to(dt).transpose(1, 2), w.to(dt), bias.to(dt)
    y = F.conv_transpose1d(xt, wt, b, stride=u, padding=(k - u) // 2)
    s = F.conv_transpose1d(xt.abs(), wt.abs(), b.abs(), stride=u, padding=(k - u) // 2)
    if off:
        y, s = F.pad(y, (1, 0), mode="reflect"), F.pad(s, (1, 0), mode="reflect")
    return y.transpose(1, 2) + res.to(dt), s.transpose(1, 2) + res.to(dt).abs()


# cin / cout are paired (three pairs instead of the 3 x 3 product: the phase arithmetic does not depend on their combination)
CONVT = [(u, k, cin, cout) for (u, k) in ((8, 16), (5, 11), (3, 7), (2, 4)) for (cin, cout) in ((64, 64), (256, 128), (512, 256))]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("u,k,cin,cout", CONVT[::3])
def test_cpu_convtranspose_bound_holds_for_torch_fp32(u, k, cin, cout, off, mode):
    x, w, bias, res, t_out = _convt_case(u, k, cin, cout, 23, off, mode)
    ref, sabs = _convt_ref(x, w, bias, res, u, k, off, F64)
    t32, _ = _convt_ref(x, w, bias, res, u, k, off, torch.float32)
    H.check("torch fp32 conv_transpose1d", t32, ref, H.sum_bound(-(-k // u) * cin + 2, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("t_in", [1, 23, 130])
@pytest.mark.parametrize("u,k,cin,cout", CONVT)
def test_convtranspose_phase_gemms(u, k, cin, cout, t_in, off, mode):
    """The launches of HiFTGenerator._decode_cl_impl: u phase GEMMs with tap_step = -1, out_row_stride = u, out_row_off = r + off, out_rows,
    the fused residual, and for off = 1 the extra M = 1 launch that writes ReflectionPad1d((1, 0))'s row 0 = phase 1 at q = 0."""
    from cosyvoice_amd import ops
    from cosyvoice_amd.hift import _ConvT
    x, w, bias, res, t_out = _convt_case(u, k, cin, cout, t_in, off, mode)
    B = x.shape[0]
    ref, sabs = _convt_ref(x, w, bias, res, u, k, off, F64)
    assert ref.shape[1] == t_out
    up = _ConvT(w, bias, u, (k - u) // 2, DT[mode], "cuda")
    ps = mode == "x3ps"
    xd = dev_op(x, mode, cin + 8)
    ldres = _ld(cout)
    resd = H.nan_like((B, t_out + G, ldres), torch.float32)
    resd[:, :t_out, :cout] = res.cuda()
    o = Outs(mode, B, t_out, cout, wantact=False)
    kw = gkw(mode)

    def phase(r, M, row_off):
        wp, ntaps, cr, wps = up.phases[r]
        ops.gemm(xd, wps.view(torch.float32) if ps else wp, M, cout, ntaps * cin, batch=B, a_bs=(xd.stride(0), 0), lda=xd.stride(1),
                 a_rows=t_in, cin=cin, tap_base=cr, tap_step=-1, bias=up.b, res=resd, res_bs=(resd.stride(0), 0), ldres=ldres,
                 out_row_stride=u, out_row_off=row_off, out_rows=t_out, ldw=ntaps * cin, **o.kw(), **kw)

    for r in range(u):
        phase(r, t_in, r + off)
    if off:
        phase(1, 1, 0)
    torch.cuda.synchronize()
    o.check(f"convT u={u} k={k} off={off}", ref, sabs, -(-k // u) * cin + 2)


# ----------------------------------------------------------------------------- 3. two-level batch (rel-pos bias GEMM)
def _relpos_case(T, mode):
    torch.manual_seed(T)
    R, Hh, D = 2, 8, 512
    q = rvals(torch.randn(R, T, Hh, 64), mode)
    p = rvals(torch.randn(2 * T - 1, Hh, 64) / 8, mode)
    return q, p


def _relpos_ref(q, p, dt):
    y = torch.einsum("rthd,nhd->rhtn", q.to(dt), p.to(dt)) * 0.125
    return y, torch.einsum("rthd,nhd->rhtn", q.to(dt).abs(), p.to(dt).abs()) * 0.125


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [7, 100, 333])
def test_cpu_two_level_batch_bound_holds_for_torch_fp32(T, mode):
    q, p = _relpos_case(T, mode)
    ref, sabs = _relpos_ref(q, p, F64)
    H.check("torch fp32 einsum", _relpos_ref(q, p, torch.float32)[0], ref, H.sum_bound(64, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [7, 100, 333])
def test_two_level_batch_relpos_bias(T, mode):
    """The matrix_bd launch of flow.py's _layer: batch = R * H, batch_inner = H, a_bs = (64, T * 3D), w_bs = (64, 0), K = 64, N = 2T - 1 (odd:
    scalar epilogue), out_scale.  A is the middle third of a (R, T, 3D) buffer whose other two thirds are NaN."""
    from cosyvoice_amd import ops
    q, p = _relpos_case(T, mode)
    R, _, Hh, _ = q.shape
    D, N = Hh * 64, 2 * T - 1
    ref, sabs = _relpos_ref(q, p, F64)
    qkv = torch.full((R, T, 3, D), float("nan"))
    qkv[:, :, 1] = q.reshape(R, T, D)
    if mode == "x3ps":
        qd = H.presplit_f32(torch.nan_to_num(qkv.reshape(R, T, 3 * D), nan=0.0)).cuda()
        bad = H.nan_split((R, T, D))
        qd[:, :, :D], qd[:, :, 2 * D:] = bad, bad
    else:
        qd = qkv.reshape(R, T, 3 * D).to(DT[mode]).cuda()
    pd = dev_op(p.reshape(N, D), mode, D)
    ldb = (N + 3) // 4 * 4
    bd = H.nan_like((R * Hh * T + G, ldb), torch.float32)
    ops.gemm(qd[:, :, D:], pd, T, N, 64, batch=R * Hh, batch_inner=Hh, a_bs=(64, T * 3 * D), lda=3 * D, w_bs=(64, 0), ldw=D,
             out_scale=0.125, out_f32=bd, o32_bs=(T * ldb, Hh * T * ldb), ldo32=ldb, **gkw(mode))
    torch.cuda.synchronize()
    o = bd.cpu()
    assert bool(torch.isnan(o[R * Hh * T:]).all()) and bool(torch.isnan(o[:, N:]).all()), "bias GEMM wrote outside (R, H, T, 2T - 1)"
    H.check(f"rel-pos bias T={T}", o[:R * Hh * T, :N].view(R, Hh, T, N), ref,
            H.sum_bound(64, sabs, ref, torch.float32, x3=mode in ("x3", "x3ps")))


# ----------------------------------------------------------------------------- 4. epilogue matrix
ACTS = [("NONE", 0.0), ("GELU", 0.0), ("SILU", 0.0), ("MISH", 0.0), ("LEAKY", 0.1), ("LEAKY", 0.01), ("ELU", 0.0), ("SNAKE", 0.0), ("TANH", 0.0)]


def _epi_case(N, mode):
    torch.manual_seed(N)
    B, M, K = 2, 77, 72
    x = rvals(torch.randn(B, M, K), mode)
    w = rvals(torch.randn(N, K) * (2.0 / K ** 0.5), mode)
    bias, res, res2 = torch.randn(N), torch.randn(B, M, N), torch.randn(B, M, N)
    alpha = torch.exp(torch.rand(N) * math.log(30 / 0.02) + math.log(0.02))       # per-column Snake alpha in [0.02, 30]
    return x, w, bias, res, res2, alpha


def _epi_ref(x, w, bias, res, res2, extra, dt):
    v, s = x.to(dt) @ w.to(dt).t() + bias.to(dt), x.to(dt).abs() @ w.to(dt).abs().t() + bias.to(dt).abs()
    n, scale = x.shape[-1] + 1, 1.0
    if extra >= 1:
        v, s, n = v + res.to(dt), s + res.to(dt).abs(), n + 1
    if extra >= 2:
        scale = torch.tensor(1.0 / 3.0, dtype=torch.float32).to(dt)
        v, s, n = (v + res2.to(dt)) * scale, (s + res2.to(dt).abs()) * scale, n + 2
    return v, s, n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [64, 80, 18, 1])
def test_cpu_epilogue_bound_holds_for_torch_fp32(N, mode):
    x, w, bias, res, res2, _ = _epi_case(N, mode)
    for extra in (0, 1, 2):
        ref, sabs, n = _epi_ref(x, w, bias, res, res2, extra, F64)
        H.check("torch fp32 linear + epilogue", _epi_ref(x, w, bias, res, res2, extra, torch.float32)[0], ref,
                H.sum_bound(n, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [64, 80, 18, 1])
@pytest.mark.parametrize("act,slope", ACTS)
def test_epilogue_matrix(act, slope, N, mode):
    """Every cv_act but SWIGLU (CV_ACT_NONE / GELU / SILU / MISH / LEAKY with act_slope 0.1 and 0.01 / ELU / SNAKE / TANH) x {out_f32 only, out_act only, both} x {bias, bias + res, bias + res + res2 + out_scale = 1/3}; N = 64 / 80 take
    the vector epilogue, 18 / 1 the scalar one; ldo32 / ldoa / ldres / ldres2 > N; a per-column act_param for Snake on both paths; pre-split
    out_act (x3_flags = 7) where N % 8 == 0."""
    from cosyvoice_amd import ops
    x, w, bias, res, res2, alpha = _epi_case(N, mode)
    B, M, K = x.shape
    xd, wd = dev_op(x, mode, K + 8), dev_op(w, mode, K + 8)
    ldr = _ld(N)
    resd, res2d = H.nan_like((B, M + G, ldr), torch.float32), H.nan_like((B, M + G, ldr + 8), torch.float32)
    resd[:, :M, :N], res2d[:, :M, :N] = res.cuda(), res2.cuda()
    res2d = res2d.view(-1)[:B * (M + G) * ldr].view(B, M + G, ldr)          # res2 shares res's batch stride; its own leading dimension below
    res2d.fill_(float("nan"))
    res2d[:, :M, :N] = res2.cuda()
    slope32 = torch.tensor(slope, dtype=torch.float32).item()
    out_split = mode == "x3ps" and N % 8 == 0
    for want32, wantact in ((True, False), (False, True), (True, True)):
        for extra in (0, 1, 2):
            ref, sabs, n = _epi_ref(x, w, bias, res, res2, extra, F64)
            o = Outs(mode, B, M, N, want32, wantact, out_split and wantact)
            kw = gkw(mode, out_split and wantact)
            if extra >= 1:
                kw.update(res=resd, res_bs=(resd.stride(0), 0), ldres=ldr)
            if extra >= 2:
                kw.update(res2=res2d, ldres2=ldr, out_scale=1.0 / 3.0)
            ops.gemm(xd, wd, M, N, K, batch=B, a_bs=(xd.stride(0), 0), lda=xd.stride(1), ldw=wd.stride(0), bias=bias.cuda(), act=act_id(act),
                     act_param=alpha.cuda() if act == "SNAKE" else None, act_slope=slope, **o.kw(), **kw)
            torch.cuda.synchronize()
            o.check(f"epilogue {act} N={N} extra={extra}", ref, sabs, n, act, alpha if act == "SNAKE" else None, slope32)


# ----------------------------------------------------------------------------- 5. K and tap tails
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [8, 72, 200, 904])
def test_cpu_dense_k_tail_bound_holds_for_torch_fp32(K, mode):
    torch.manual_seed(K)
    x, w = rvals(torch.randn(2, 77, K), mode), rvals(torch.randn(40, K) / K ** 0.5, mode)
    ref, sabs = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    H.check("torch fp32 matmul", x @ w.t(), ref, H.sum_bound(K, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [8, 72, 200, 904])
def test_dense_k_tail(K, mode):
    """K below, across and far past the 128-byte K tile (32 fp32 / 64 16-bit values), never a multiple of it."""
    from cosyvoice_amd import ops
    torch.manual_seed(K)
    B, M, N = 2, 77, 40
    x, w = rvals(torch.randn(B, M, K), mode), rvals(torch.randn(N, K) / K ** 0.5, mode)
    ref, sabs = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    xd, wd = dev_op(x, mode, K + 8), dev_op(w, mode, K + 8)
    o = Outs(mode, B, M, N)
    ops.gemm(xd, wd, M, N, K, batch=B, a_bs=(xd.stride(0), 0), lda=xd.stride(1), ldw=wd.stride(0), **o.kw(), **gkw(mode))
    torch.cuda.synchronize()
    o.check(f"dense K={K}", ref, sabs, K)


TAPS = [(80, 7), (24, 7), (320, 3), (8, 11)]


def _tap_case(cin, k, T, mode):
    torch.manual_seed(cin + k + T)
    x = rvals(torch.randn(2, T, cin), mode)
    w = rvals(torch.randn(40, cin, k) / (cin * k) ** 0.5, mode)
    return x, w, torch.randn(40)


@pytest.mark.parametrize("mode", ["f32", "f16", "x3ps"])
@pytest.mark.parametrize("cin,k", TAPS)
def test_cpu_tap_tail_bound_holds_for_torch_fp32(cin, k, mode):
    for T in (1, 2, 63, 65):
        x, w, bias = _tap_case(cin, k, T, mode)
        for dil in (1, 3, 5):
            for pad in (((k - 1) * dil, 0), ((k * dil - dil) // 2,) * 2):
                ref, sabs = conv_ref(x, w, bias, F64, dil=dil, pad=pad)
                H.check("torch fp32 conv1d", conv_ref(x, w, bias, torch.float32, dil=dil, pad=pad)[0], ref,
                        H.sum_bound(cin * k + 1, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dil", [1, 3, 5])
@pytest.mark.parametrize("cin,k", TAPS)
def test_conv_tap_tails(cin, k, dil, mode):
    """(cin, k) whose per-tap channel run straddles the 128-byte K tile, dilations 1 / 3 / 5, causal (pad_left = (k - 1) d) and symmetric
    padding, T in {1, 2, 63, 65}: the halo exceeds the sequence at the short ones."""
    from cosyvoice_amd import ops
    for T in (1, 2, 63, 65):
        x, w, bias = _tap_case(cin, k, T, mode)
        xd, wd = dev_op(x, mode, cin + 8), dev_op(pack_w(w), mode, k * cin + 8)
        for pad in (((k - 1) * dil, 0), ((k * dil - dil) // 2,) * 2):
            ref, sabs = conv_ref(x, w, bias, F64, dil=dil, pad=pad)
            o = Outs(mode, 2, T, 40)
            ops.conv1d_cl(xd, wd, k, dilation=dil, pad_left=pad[0], bias=bias.cuda(), out_f32=o.o32[:, :T, :40], out_act=o.oa[:, :T, :40],
                          **gkw(mode))
            torch.cuda.synchronize()
            o.check(f"conv cin={cin} k={k} d={dil} T={T} pad={pad}", ref, sabs, cin * k + 1)


# ----------------------------------------------------------------------------- 6. tile variants through the dispatcher
# (batch, M, N, K) and the branch of dispatch<> / dispatch_x3 (csrc/gemm.hip) it selects, t = ceil(M / 128) * ceil(N / 64) * batch:
#   small: K = 256 <= 512                                  -> 64 x 64           (x3 / x3ps: the "small" 64 x 64 bf16x3 tiles)
#   big:   K = 520 > 512, t = 9 * 11 * 8 = 792 >= 768      -> 128 x 64          (x3 / x3ps: the "big" 128 x 64 bf16x3 tiles)
#   tall:  batch 1, M = 9001 >= 8192, N = K = 512          -> 8-wave 128 x 128  (x3 / x3ps: K = 512 is not > 512 -> small)
TILES = {"small": (2, 200, 192, 256), "big": (8, 1100, 704, 520), "tall": (1, 9001, 512, 512)}


def _tile_case(shape, mode):
    B, M, N, K = TILES[shape]
    torch.manual_seed(M)
    return rvals(torch.randn(B, M, K), mode), rvals(torch.randn(N, K) / K ** 0.5, mode), torch.randn(B, M, N)


@pytest.mark.parametrize("shape", ["small", "big"])
def test_cpu_tile_shapes_bound_holds_for_torch_fp32(shape):
    x, w, res = _tile_case(shape, "bf16")
    ref, sabs = x.double() @ w.double().t() + res.double(), x.double().abs() @ w.double().abs().t() + res.double().abs()
    H.check("torch fp32 matmul", x @ w.t() + res, ref, H.sum_bound(x.shape[-1] + 1, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(TILES))
def test_tile_variants(shape, mode):
    from cosyvoice_amd import ops
    x, w, res = _tile_case(shape, mode)
    B, M, N, K = TILES[shape]
    ref, sabs = x.double() @ w.double().t() + res.double(), x.double().abs() @ w.double().abs().t() + res.double().abs()
    xd, wd = dev_op(x, mode, K + 8), dev_op(w, mode, K + 8)
    o = Outs(mode, B, M, N)
    resd = res.cuda()
    ops.gemm(xd, wd, M, N, K, batch=B, a_bs=(xd.stride(0), 0), lda=xd.stride(1), ldw=wd.stride(0), res=resd, res_bs=(M * N, 0), ldres=N,
             **o.kw(), **gkw(mode))
    torch.cuda.synchronize()
    o.check(f"tile {shape}", ref, sabs, K + 1)


# ----------------------------------------------------------------------------- 7. x3_flags = 4 alone
@gpu
@pytest.mark.parametrize("act,slope", [("NONE", 0.0), ("LEAKY", 0.1)])
def test_x3_plain_in_presplit_out(act, slope):
    """HiFT's conv_pre: plain fp32 operands in, pre-split out_act out (x3_flags = 4 alone).  The pre-split activation is bit-identical to
    _presplit of the fp32 output of the same launch (LeakyReLU is one exact fp32 multiply, repeated here in torch)."""
    from cosyvoice_amd import ops
    torch.manual_seed(4)
    B, T, cin, cout, k = 2, 77, 80, 512, 7
    x, w, bias = torch.randn(B, T, cin), torch.randn(cout, cin, k) / (cin * k) ** 0.5, torch.randn(cout)
    ref, sabs = conv_ref(x, w, bias, F64, pad=(3, 3))
    xd, wd = dev_op(x, "x3", cin + 8), dev_op(pack_w(w), "x3", k * cin + 8)
    o = Outs("x3", B, T, cout, out_split=True)
    ops.conv1d_cl(xd, wd, k, pad_left=3, bias=bias.cuda(), act=act_id(act), act_slope=slope, out_f32=o.o32[:, :T, :cout],
                  out_act=o.oa[:, :T, :cout], **gkw("x3", out_split=True))
    torch.cuda.synchronize()
    o.check("conv_pre x3_flags=4", ref, sabs, cin * k + 1, act, None, torch.tensor(slope, dtype=torch.float32).item())
    v = o.o32.cpu()[:, :T, :cout].contiguous()
    a = torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32)) if act == "LEAKY" else v
    got = o.oa.cpu()[:, :T, :cout].contiguous().view(torch.int32)
    assert torch.equal(got, H.presplit_f32(a).view(torch.int32)), "pre-split out_act differs from _presplit(out_f32)"


# ----------------------------------------------------------------------------- cv_layernorm modes (the GPU half is tests/test_gemm_gpu.py::test_layernorm_modes)
@pytest.mark.parametrize("act", ["NONE", "MISH"])
@pytest.mark.parametrize("rpg", [1, 37])
@pytest.mark.parametrize("dim", [80, 256, 1024])
def test_cpu_layernorm_bound_holds_for_torch_fp32(dim, rpg, act):
    """test_layernorm's fp32 bound, 2e-5 max|ref| + 1e-5, at x = 1000 + N(0, 1) is within reach of fp32 arithmetic only when the mean is
    subtracted in two terms: F.layer_norm's own fp32 path carries it as one fp32 and errs by 1.0e-4 .. 1.9e-4 here (as norm_kernel did,
    1.3e-4 .. 1.5e-4 measured on MI355X, before it subtracted the residual mean too).  The fp32 evaluation checked here is therefore the
    plain-tensor restatement with the two-term mean; F.layer_norm's figure is printed next to it."""
    ref = H.layernorm_case(dim, rpg, act, 0.5, F64)[4]
    t32 = H.layernorm_case(dim, rpg, act, 0.5, torch.float32, two_term_mean=True)[4]
    fused = (H.layernorm_case(dim, rpg, act, 0.5, torch.float32)[4].double() - ref).abs().max().item()
    err = (t32.double() - ref).abs().max().item()
    msg = f"fp32 two-term mean: max|err| {err:.3e}; F.layer_norm fp32: {fused:.3e}; max|ref| {ref.abs().max().item():.3e}"
    print(msg)
    assert err < 2e-5 * ref.abs().max().item() + 1e-5, msg
