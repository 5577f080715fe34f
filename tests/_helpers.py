"""Shared helpers of the op-level parity tests: pre-split storage codecs, ulp arithmetic, the element-wise error bounds the tests
assert, and sentinel (guard / leak) buffers.  Plain functions, imported by the test modules (not a conftest)."""
import math

import torch

EPS32 = 2.0 ** -23
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
MIN_EXP = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
ACT_LIPSCHITZ = {"NONE": 1.0, "GELU": 1.13, "SILU": 1.1, "MISH": 1.09, "LEAKY": 1.0, "ELU": 1.0, "SNAKE": 2.0, "TANH": 1.0}


def unsplit(t):
    """pre-split fp32-sized storage (.., C) -> the fp32 values hi + lo it stands for."""
    raw = t.contiguous().view(torch.int16).reshape(*t.shape[:-1], t.shape[-1] // 8, 16)
    hi, lo = raw[..., :8].contiguous().view(torch.bfloat16), raw[..., 8:].contiguous().view(torch.bfloat16)
    return (hi.float() + lo.float()).reshape(t.shape)


def presplit_f32(x):
    """fp32 (.., C), C % 8 == 0 -> the same shape of fp32-sized PRE-SPLIT storage ([8 x bf16 hi | 8 x bf16 lo] per 8 values)."""
    from cosyvoice_amd.hift import _presplit
    x = x.float().cpu().contiguous()
    return _presplit(x.reshape(-1, x.shape[-1])).view(torch.float32).reshape(x.shape)


def ulp(ref, dt):
    """Spacing of ``dt`` (a torch dtype, or "split" for the hi + lo bf16 pair) at |ref|, float64."""
    ref = ref.double().abs()
    if dt == "split":       # hi = bf16(v) leaves |v - hi| <= 2^-8 |v|; lo = bf16(v - hi) leaves 2^-8 of that: half an "ulp" = 2^-16 |v|
        return ref * 2.0 ** -15
    e = torch.frexp(ref)[1].double() - 1                       # |ref| = m * 2^(e+1), m in [0.5, 1)
    e = torch.clamp(e, min=MIN_EXP[dt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dt])


def sum_bound(n, sabs, ref, dt, x3=False):
    """Rule 2: forward bound of an n-term sum of products accumulated in fp32, (n + 2) 2^-23 sum|terms| + half an ulp of the output
    type; bf16x3 products add the dropped lo * lo term, 2^-16 sum|terms|."""
    b = (n + 2) * EPS32 * sabs.double() + 0.5 * ulp(ref, dt)
    if x3:
        b = b + 2.0 ** -16 * sabs.double()
    return b


def act_bound(e32, ref, dt=torch.float32):
    """Rule 3: a transcendental evaluated in fp32 with fast intrinsics may err by 4 x max(torch's own fp32 error, 2^-23 |ref|), plus the
    rounding to the output type."""
    return 4.0 * torch.maximum(e32.double(), EPS32 * ref.double().abs()) + 0.5 * ulp(ref, dt)


def check(name, got, ref, bound):
    """Element-wise |got - ref| <= bound, no exceptions; the message carries the measured figures."""
    got, ref, bound = got.double().cpu(), ref.double().cpu(), bound.double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    msg = f"{name}: max|err| {err.max().item():.3e}, max err/bound {ratio:.3f}, max|ref| {ref.abs().max().item():.3e}"
    print(msg)          # shown by pytest -s / on failure: the figures of DESIGN.md §2 come from these lines
    assert bool((err <= bound).all()), msg
    return err.max().item(), ratio


def nan_like(shape, dt, device="cuda"):
    """A buffer of NaN: the sentinel an op must leave where it does not write, and the poison it must not read."""
    return torch.full(shape, float("nan"), dtype=dt, device=device)


def nan_split(shape, device="cuda"):
    """fp32-sized pre-split storage whose every bf16 half is NaN."""
    return torch.full((*shape[:-1], shape[-1] * 2), 0x7FC0, dtype=torch.int16, device=device).view(torch.float32)


def layernorm_case(dim, rows_per_group, act, scale, dt, groups=3, T=37, two_term_mean=False):
    """cv_layernorm with a per-group add: rows with a large common offset (x = 1000 + N(0, 1)); returns x, gamma, beta, add and
    (act(LayerNorm(x)) + add[row // rows_per_group]) * scale evaluated in ``dt`` by F.layer_norm, or (two_term_mean) by plain tensor
    operations that subtract the mean in two terms, mean and the mean of the residual x - mean, as norm_kernel does."""
    import torch.nn.functional as F
    g_ = torch.Generator().manual_seed(dim + rows_per_group)
    rows = groups * T
    x = 1000.0 + torch.randn(rows, dim, generator=g_)
    g, b = torch.randn(dim, generator=g_), torch.randn(dim, generator=g_)
    add = torch.randn(rows // rows_per_group, dim, generator=g_)
    if two_term_mean:
        d = x.to(dt) - x.to(dt).mean(-1, keepdim=True)
        d = d - d.mean(-1, keepdim=True)
        y = d * torch.rsqrt((d * d).mean(-1, keepdim=True) + 1e-5) * g.to(dt) + b.to(dt)
    else:
        y = F.layer_norm(x.to(dt), (dim,), g.to(dt), b.to(dt), 1e-5)
    if act == "MISH":
        y = F.mish(y)
    y = (y + add.to(dt).repeat_interleave(rows_per_group, 0)) * scale
    return x, g, b, add, y


def source_ref64(f0, pv, noise, lin_w, lin_b, up, sr, amp, sigma, vthr):
    """sine_gen(scan_dtype=float64) -> linear -> tanh of oracle/hift.py with every step after F_mat in float64 (F_mat itself formed in fp32,
    generator.py:145)."""
    nh = pv.shape[1]
    f0u = f0.repeat_interleave(up, dim=1)[:, None]                                                  # (B, 1, S)
    Fm = (f0u * torch.arange(1, nh + 1, dtype=torch.float32).reshape(1, nh, 1) / sr).double()
    theta = 2 * math.pi * (torch.cumsum(Fm, -1) % 1)
    p = pv.double().clone()
    p[:, 0] = 0
    uv = (f0u > vthr).double()
    sw = amp * torch.sin(theta + p) * uv + (uv * sigma + (1 - uv) * amp / 3) * noise.double()
    return torch.tanh((sw * lin_w.double().reshape(1, nh, 1)).sum(1) + lin_b.double())


def scan_drift_bound(cfg, f0_up, nh=None):
    """2 pi sine_amp ulp32(C_max): one ulp of the largest value the fp32 cumulative sum reaches (f0_up (B, 1, S), top harmonic).  An fp32
    running sum is off by about half an ulp of itself (measured: exactly that, over four seeds), times 2 pi for the phase, times the
    amplitude of the sine; one ulp leaves a factor 2."""
    nh = cfg.nb_harmonics + 1 if nh is None else nh
    F_top = f0_up * torch.tensor(float(nh)) / cfg.sampling_rate
    c_max = torch.cumsum(F_top, dim=-1).max()
    return 2 * math.pi * cfg.nsf_alpha * ulp(c_max, torch.float32).item(), c_max.item()
