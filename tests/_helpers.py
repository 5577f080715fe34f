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


# ----------------------------------------------------------------------------- attention (cv_attention, cv_decode_attention)
LOG2E32 = 1.4426950408889634
NEG_BIG = -1e30
ATTN_CS = 136           # score term of attn_bound, see its docstring
ATTN_C = 10             # constant term of attn_bound
DECODE_MERGE_C = 10     # the 8-wave log-sum-exp merge of cv_decode_attention


def attn_mask(B, Tq, Tk, klen=None, chunk=0, causal=False, causal_off=0, q_off=0):
    """(B, Tq, Tk) bool, True = visible, as include/cosyvoice_amd.h states the masks: j < min(klen[b], Tk); chunk: j < ((i + q_off) / chunk
    + 1) * chunk; causal: j <= i + causal_off."""
    i = torch.arange(Tq)[:, None]
    j = torch.arange(Tk)[None, :]
    ok = torch.ones(Tq, Tk, dtype=torch.bool)
    if causal:
        ok &= j <= i + causal_off
    if chunk:
        ok &= j < ((i + q_off) // chunk + 1) * chunk
    ok = ok[None].expand(B, Tq, Tk).clone()
    if klen is not None:
        kl = torch.as_tensor(klen, dtype=torch.long).clamp(max=Tk)
        ok &= j[None] < kl[:, None, None]
    return ok


def attn_ref64(q, k, v, scale, ok, bias=None):
    """float64 softmax(scale q k^T + bias) v over the visible keys, from the already rounded operands.  q (B, H, Tq, 64), k / v (B, Hkv, Tk, 64),
    ok (B, Tq, Tk) bool, bias (B, H, Tq, Tk) or None (its masked entries may hold anything, NaN included).  Rows without a visible key are zero.
    Returns ref, A = sum_j p |v|, S = max over the visible keys of scale sum_d |q k| + |bias| (B, H, Tq), and sub = sum_j [p / max p < 2^-14]
    p |v| (the part of A carried by probabilities that are subnormal in fp16)."""
    q, k, v = q.double(), k.double(), v.double()
    rep = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    okh = ok[:, None]
    s = scale * (q @ k.transpose(-1, -2))
    sa = scale * (q.abs() @ k.abs().transpose(-1, -2))
    if bias is not None:
        bz = torch.where(okh, bias.double(), torch.zeros((), dtype=torch.float64))
        s, sa = s + bz, sa + bz.abs()
    s = s.masked_fill(~okh, float("-inf"))
    live = okh.any(-1, keepdim=True)
    m = torch.where(live, s.max(-1, keepdim=True).values, torch.zeros((), dtype=torch.float64))
    e = torch.exp(s - m)                                                   # 1 at the row maximum, 0 at masked keys
    p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    S = torch.where(live[..., 0], sa.masked_fill(~okh, 0.0).max(-1).values, torch.zeros((), dtype=torch.float64))
    return p @ v, p @ v.abs(), S, (p * (e < 2.0 ** -14)) @ v.abs()


def attn_bound(ref, A, S, sub, Tk, dt, merge=0):
    """Element-wise bound of the flash kernels against attn_ref64 (derivation: module docstring of tests/test_attention_ops_gpu.py):
    (u_P + ATTN_CS 2^-23 S_i + (Tk + 2 ceil(Tk / 64) + ATTN_C + merge) 2^-23) A_id + half an ulp of the output (+ sub for fp16).  Tk: the
    number of keys a row may see, an int or an integer tensor that broadcasts against A."""
    n = Tk + 2 * ((Tk + 63) // 64) + ATTN_C + merge
    b = (2.0 ** -(MANT[dt] + 1) + ATTN_CS * EPS32 * S[..., None] + n * EPS32) * A + 0.5 * ulp(ref, dt)
    return b + sub if dt == torch.float16 else b


def attn_emulate(q, k, v, scale, ok, dt, bias=None, waves=1, flush=False):
    """Plain torch emulation of the kernels' arithmetic (no library code): fp32 scores, scale * log2(e) folded into one fp32 factor, masked
    scores = -1e30, 64-key online softmax with exp2, the denominator from the unrounded fp32 P, the numerator from P rounded to ``dt``
    (flush: fp16-subnormal P flushed to zero instead of rounded gradually), fp32 accumulation, rows without a visible key zero; ``waves``
    > 1: tile t belongs to wave t % waves and the waves are merged by log-sum-exp (cv_decode_attention).  Returns (B, H, Tq, 64) ``dt``."""
    f32 = torch.float32
    rep = q.shape[1] // k.shape[1]
    qf, kf, vf = q.to(f32), k.to(f32).repeat_interleave(rep, 1), v.to(f32).repeat_interleave(rep, 1)
    Tk = kf.shape[2]
    sc = (torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E32, dtype=f32)).item()
    t = (qf @ kf.transpose(-1, -2)) * sc
    okh = ok[:, None].expand_as(t)
    if bias is not None:
        t = t + torch.where(okh, bias.to(f32), torch.zeros((), dtype=f32)) * torch.tensor(LOG2E32, dtype=f32)
    t = torch.where(okh, t, torch.full((), NEG_BIG, dtype=f32))
    shape = t.shape[:-1]
    parts = []
    for w in range(waves):
        m, l, o = torch.full(shape, NEG_BIG, dtype=f32), torch.zeros(shape, dtype=f32), torch.zeros(*shape, 64, dtype=f32)
        for j0 in range(64 * w, Tk, 64 * waves):
            tt = t[..., j0:j0 + 64]
            mnew = torch.maximum(m, tt.max(-1).values)
            p = torch.exp2(tt - mnew[..., None])
            p = torch.where((mnew <= 0.5 * NEG_BIG)[..., None], torch.zeros((), dtype=f32), p)
            alpha = torch.exp2(m - mnew)
            l = l * alpha + p.sum(-1)
            pr = p.to(dt)
            if flush and dt == torch.float16:
                pr = torch.where(p < 2.0 ** -14, torch.zeros((), dtype=dt), pr)
            o = o * alpha[..., None] + pr.to(f32) @ vf[..., j0:j0 + 64, :]
            m = mnew
        parts.append((m, l, o))
    if waves > 1:
        mm = torch.stack([p_[0] for p_ in parts]).max(0).values
        l, o = torch.zeros(shape, dtype=f32), torch.zeros(*shape, 64, dtype=f32)
        for m_, l_, o_ in parts:
            ww = torch.exp2(m_ - mm)
            l, o = l + l_ * ww, o + o_ * ww[..., None]
    inv = torch.where(l > 0, 1.0 / l.clamp_min(1e-38), torch.zeros((), dtype=f32))
    return (o * inv[..., None]).to(dt)


def kv_tile_index(key, d, v=False):
    """Vectorised index map of the fragment-tiled KV cache as include/cosyvoice_amd.h documents it (cv_kv_retile), written from the header's
    formulas, not from ops.kv_tile_index: element offset of (key, d) inside one (sequence, kv head) cache; key, d integer tensors."""
    t, r = key // 64, key % 64
    if not v:       # ((kt*2 + f)*64 + lq + 16*lg)*8 + e : key 16*kt + lq, d = 32*f + 8*lg + e
        kt, lq, f, lg, e = r // 16, r % 16, d // 32, (d % 32) // 8, d % 8
        i = ((kt * 2 + f) * 64 + lq + 16 * lg) * 8 + e
    else:           # ((dt*2 + s2)*64 + lq + 16*lg)*8 + e : key 32*s2 + 16*(e >> 2) + 4*lg + (e & 3), d = 16*dt + lq
        dt_, lq, s2, r32 = d // 16, d % 16, r // 32, r % 32
        e = 4 * (r32 // 16) + r32 % 4
        lg = (r32 % 16) // 4
        i = ((dt_ * 2 + s2) * 64 + lq + 16 * lg) * 8 + e
    return t * 4096 + i


# ----------------------------------------------------------------------------- LLM decode ops
def rope_ref64(x, ang32):
    """HF rotate_half RoPE of x (.., 64) in float64 with the angle given in fp32 (.., 32) (the single fp32 product pos * inv_freq[d], or a table
    entry): returns ref, sum|terms| and torch's own fp32 evaluation of the same expression."""
    x1, x2 = x[..., :32].double(), x[..., 32:].double()
    c, s = torch.cos(ang32.double()), torch.sin(ang32.double())
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    sabs = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    c32, s32 = torch.cos(ang32), torch.sin(ang32)
    t32 = torch.cat([x[..., :32] * c32 - x[..., 32:] * s32, x[..., 32:] * c32 + x[..., :32] * s32], -1)
    return ref, sabs, t32


def rope_table_ref64(x, c32, s32):
    """The same rotation with cos / sin given as fp32 numbers (a table row), taken as exact: ref and sum|terms|."""
    x1, x2, c, s = x[..., :32].double(), x[..., 32:].double(), c32.double(), s32.double()
    return (torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1),
            torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1))


def rope_bound(ref, sabs, t32, dt):
    """Rule 2 with n = 2 (two products, one sum) + rule 3 for sincosf (4 x max(e32, 2^-23 |ref|), e32 from torch's fp32 evaluation) + half an
    ulp of the 16-bit output (inside sum_bound)."""
    e32 = (t32.double() - ref).abs().max()
    return sum_bound(2, sabs, ref, dt) + 4.0 * torch.maximum(e32, EPS32 * ref.abs())


def rmsnorm_ref64(v, gamma, eps, dt):
    """rmsnorm(v) * gamma in float64 from fp32 v (rows, dim), and its bound: the sum of dim squares in fp32 errs by <= (dim + 2) 2^-23 of
    itself (all terms >= 0), / dim and + eps add two roundings; through rsqrt (d x^-1/2 = -x^-3/2 dx / 2) that is (dim + 4) / 2 x 2^-23
    relative, rsqrtf itself <= 2 ulp, the two products v * rstd * gamma one more: (dim / 2 + 5) 2^-23 |ref| + half an ulp of the output."""
    v, g = v.double(), gamma.double()
    dim = v.shape[-1]
    ref = v * torch.rsqrt((v * v).mean(-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32).double()) * g
    return ref, (dim / 2 + 5) * EPS32 * ref.abs() + 0.5 * ulp(ref, dt)


# ----------------------------------------------------------------------------- flow estimator row-block kernels (csrc/flowblock.hip)
AS_ERFC_CAP = 1.5e-7    # Abramowitz-Stegun 7.1.26, the |error| the kernel's gelu_erf comment states for its erfc polynomial
ROW_KINDS = ("x30", "offset", "const", "zero")


def flow_rows(R, T, width, g):
    """(R, T, width) fp32 activations: ordinary rows 2 N(0, 1) + 0.3, and in every sequence r the four special rows ROW_KINDS[(r + j) % 4] at
    rows (T - 1, 0, T // 2, 1)[j] (a position that repeats keeps its first kind: T = 1 holds x30 / offset / const in its three sequences):
    x30 = an ordinary row times 30, offset = an ordinary row + 100, const = c + 1e-3 N(0, 1) with c = 0.5 + 0.25 r (variance 1e-6: eps = 1e-5
    dominates), zero = all zeros.  The last row of a sequence and the first of the next are therefore always of different kinds."""
    x = torch.randn(R, T, width, generator=g) * 2 + 0.3
    for r in range(R):
        seen = set()
        for j, t in enumerate((T - 1, 0, T // 2, 1)):
            if t in seen or t >= T:
                continue
            seen.add(t)
            kind = ROW_KINDS[(r + j) % 4]
            if kind == "x30":
                x[r, t] *= 30.0
            elif kind == "offset":
                x[r, t] += 100.0
            elif kind == "const":
                x[r, t] = (0.5 + 0.25 * r) + 1e-3 * torch.randn(width, generator=g)
            else:
                x[r, t] = 0.0
    return x


def bits(t):
    """The tensor's storage as integers: equality that tells NaN payloads and signed zeros apart."""
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def window_only(name, buf, rows, c0, c1):
    """buf (rows + guard, ld) was NaN everywhere before the op: after it only [0, rows) x [c0, c1) may hold anything else."""
    m = torch.isnan(buf.float())
    assert bool(m[rows:].all()), f"{name}: guard rows past the last sequence were written"
    assert bool(m[:rows, :c0].all()) and bool(m[:rows, c1:].all()), f"{name}: pitch slack outside columns [{c0}, {c1}) was written"


def carry16(y, b, dt):
    """Interval of a 16-bit intermediate carried UNROUNDED in float64: its fp32 error bound b plus half an ulp of ``dt`` at the largest value
    the kernel may have rounded (|y| + b)."""
    return b + 0.5 * ulp(y.abs() + b, dt)


def ln_ref64(x, dx, gamma, beta, eps):
    """LayerNorm over the last dimension in float64 and the fp32 bound of flowblock.hip's arithmetic (one fp32 mean, then centred squares; derived
    in the module docstring of tests/test_flowblock_ops_gpu.py).  x: the rows as the kernel holds them up to the element-wise interval dx (None:
    rows read from memory, exact).  Returns y (unrounded) and its bound (without the rounding to a 16-bit type: carry16)."""
    x, g, b = x.double(), gamma.double(), beta.double()
    n = x.shape[-1]
    dx = torch.zeros_like(x) if dx is None else dx.double()
    eps64 = torch.tensor(eps, dtype=torch.float32).double()
    s = x.sum(-1, keepdim=True)
    d = x - s / n
    q = (d * d).sum(-1, keepdim=True)
    v = q / n + eps64
    rstd = torch.rsqrt(v)
    y = d * rstd * g + b
    dmu = sum_bound(n, x.abs().sum(-1, keepdim=True), s, torch.float32) / n               # rule 2 on the row sum: ~ (n + 2) 2^-23 mean|x_row|
    dd = dmu + dx + dx.mean(-1, keepdim=True) + 0.5 * ulp(d, torch.float32)               # x_i - mean: both errors and one rounding
    dq = sum_bound(n, q, q, torch.float32) + 2.0 * (d.abs() * dd).sum(-1, keepdim=True)   # rule 2 on the squares + d(d^2) = 2 |d| dd
    rel = 0.5 * (dq / n + 0.5 * EPS32 * v) / v + 2.0 * EPS32                              # through v^-1/2; + eps rounds once; rsqrtf <= 2 ulp
    first = g.abs() * rstd * (dd + d.abs() * rel) + 1.5 * EPS32 * ((d * rstd * g).abs() + b.abs())   # the last: two products and one sum
    return y, 2.0 * first


def ln_emulate(x, gamma, beta, eps, stats_from=None):
    """fp32 torch: one mean, centred squares, rsqrt, (x - mean) rstd gamma + beta; stats_from: rows whose statistics are used instead."""
    xs = x if stats_from is None else stats_from
    n = x.shape[-1]
    mean = xs.sum(-1, keepdim=True) * (1.0 / n)
    ds = xs - mean
    rstd = torch.rsqrt((ds * ds).sum(-1, keepdim=True) * (1.0 / n) + eps)
    return (x - mean) * rstd * gamma + beta


def gelu_ref64(x):
    return 0.5 * x * torch.erfc(-x * 0.7071067811865476)       # x Phi(x) without the 1 - erf cancellation of the negative side


def gelu_bound(pre, bpre, dt):
    """exact-erf GELU of a pre-activation known to the element-wise interval bpre, rounded to ``dt``: ACT_LIPSCHITZ x bpre + rule 3 + the erfc
    polynomial's stated cap 0.5 |x| 1.5e-7 (``b32``), + half an ulp; fp16: a value the kernel may hold below 2^-14 may be flushed to zero instead
    of rounded gradually (+ |g| there).  Returns g (unrounded float64), the bound, and e32."""
    import torch.nn.functional as F
    g = gelu_ref64(pre)
    p32 = pre.float()
    e32 = (F.gelu(p32).double() - gelu_ref64(p32.double())).abs().max()
    b32 = ACT_LIPSCHITZ["GELU"] * bpre + 4.0 * torch.maximum(e32, EPS32 * g.abs()) + 0.5 * pre.abs() * AS_ERFC_CAP
    b = carry16(g, b32, dt)
    if dt == torch.float16:
        b = b + torch.where(g.abs() - b32 < 2.0 ** -14, g.abs(), torch.zeros_like(g))
    return g, b, e32.item()


def gelu_emulate(x):
    """The kernel's gelu_erf in fp32 torch: relu(x) - 0.5 |x| erfc(|x| / sqrt 2), erfc by the A-S 7.1.26 polynomial, exp through exp2."""
    ax = x.abs()
    t = 1.0 / (ax * (0.3275911 * 0.70710678118654752) + 1.0)
    e = torch.exp2(x * x * (-0.5 * 1.4426950408889634))
    pl = 1.061405429 * t - 1.453152027
    pl = pl * t + 1.421413741
    pl = pl * t - 0.284496736
    pl = pl * t + 0.254829592
    return (-0.5 * ax) * (pl * t * e) + torch.clamp(x, min=0)


def mish_ref64(x):
    import torch.nn.functional as F
    return x * torch.tanh(F.softplus(x, threshold=700.0))


def mish_bound(y, by):
    """Mish of a value known to the interval by, evaluated in fp32: ACT_LIPSCHITZ x by + rule 3.  Returns m (float64), the bound, e32."""
    import torch.nn.functional as F
    m = mish_ref64(y)
    y32 = y.float()
    e32 = (F.mish(y32).double() - mish_ref64(y32.double())).abs().max()
    return m, ACT_LIPSCHITZ["MISH"] * by + 4.0 * torch.maximum(e32, EPS32 * m.abs()), e32.item()


def mish_emulate(x):
    """The kernel's mish_fast in fp32 torch: x w / (w + 2), w = e^x (e^x + 2), e^x = exp2(min(x, 20) log2 e)."""
    n = torch.exp2(torch.clamp(x, max=20.0) * 1.4426950408889634)
    w = n * (n + 2.0)
    return x * w / (w + 2.0)


def causal_conv3_64(a, w):
    """Causal k = 3 conv (left padding 2) of channels-last a (R, T, Ci) with w (Co, Ci, 3) in a's dtype (float64 for the references)."""
    import torch.nn.functional as F
    return F.conv1d(F.pad(a.transpose(1, 2), (2, 0)), w).transpose(1, 2)


def worst_ratio(got, ref, bound):
    """max err / bound, a non-finite output counting as infinite: by how much an injected fault misses."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()


# ----------------------------------------------------------------------------- GroupNorm over channels-last (csrc/norm.hip: cv_groupnorm_cl)
GN_ROWS = 32            # rows per chunk of gn_stats_kernel / gn_apply_kernel
GN_KINDS = ("ordinary", "x30", "offset100", "offset1000", "const", "zero")


def gn_units(B, T, C, G, g, start=0, order=GN_KINDS):
    """(B, T, C) fp32 with one kind per (batch, group) unit — the statistics span the unit, so the kinds of flow_rows are given to whole units:
    order[(start + b G + g) % len(order)] (order: GN_KINDS unless given): ordinary 2 N(0, 1) + 0.3, that x 30, + 100, + 1000, near-constant c + 1e-3 N(0, 1) (variance 1e-6 against
    eps 1e-5) and zero.  Returns x and the kind of every unit."""
    cpg = C // G
    x = (torch.randn(B, T, G, cpg, generator=g) * 2 + 0.3)
    kinds = []
    for b in range(B):
        for gi in range(G):
            kind = order[(start + b * G + gi) % len(order)]
            kinds.append(kind)
            if kind == "x30":
                x[b, :, gi] *= 30.0
            elif kind == "offset100":
                x[b, :, gi] += 100.0
            elif kind == "offset1000":
                x[b, :, gi] += 1000.0
            elif kind == "const":
                x[b, :, gi] = (0.5 + 0.25 * gi) + 1e-3 * torch.randn(T, cpg, generator=g)
            elif kind == "zero":
                x[b, :, gi] = 0.0
    return x.reshape(B, T, C).contiguous(), kinds


def gn_chain(T, cpg):
    """The longest chain of fp32 additions an element's contribution passes through in the fixed summation order of cv_groupnorm_cl: the strided
    adds of one of 256 threads over a 32-row chunk, the 6-step butterfly, the 3 adds of the wave sums, and 4 operations per merged chunk (the
    difference, the weight, the product and the sum of Chan's update).  The n of rule 2: a sum evaluated as a tree errs by its depth, not by its
    number of leaves."""
    return -(-min(GN_ROWS, T) * cpg // 256) + 6 + 3 + 4 * (-(-T // GN_ROWS))


def gn_ref64(x, G, gamma, beta, eps):
    """GroupNorm of channels-last x (B, T, C) in float64 and a SHIFT-INVARIANT fp32 bound built from the centred values only (derivation: module
    docstring of tests/test_norm_act_ops_gpu.py).  Returns y = (x - mu) r gamma + beta (unrounded) and its bound (before Mish / add / the rounding
    to the output type)."""
    B, T, C = x.shape
    cpg = C // G
    n = T * cpg
    nc = gn_chain(T, cpg)
    xg = x.double().reshape(B, T, G, cpg)
    g = (torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()).reshape(1, 1, G, cpg)
    b = (torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()).reshape(1, 1, G, cpg)
    eps64 = torch.tensor(eps, dtype=torch.float32).double()
    red = lambda t: t.sum((1, 3), keepdim=True)
    d = xg - red(xg) / n
    q = red(d * d)
    v = q / n + eps64
    r = torch.rsqrt(v)
    y = d * r * g + b
    dmax = d.abs().amax((1, 3), keepdim=True)
    dmu = (nc + 2) * EPS32 * red(d.abs()) / n                                  # rule 2 on the centred sum (chain of nc additions), / n
    dd = dmu + 0.5 * EPS32 * (d.abs() + dmax) + 0.5 * ulp(d, torch.float32)    # + the rounding of x - pilot (|x - p| <= |d| + max|d|) and of - mean
    dq = (nc + 2) * EPS32 * q + 2.0 * red(d.abs() * dd)                        # rule 2 on the squares + d(d^2) = 2 |d| dd
    rel = 0.5 * (dq / n + 0.5 * EPS32 * v) / v + 2.0 * EPS32                   # through v^-1/2; + eps rounds once; rsqrtf <= 2 ulp
    first = g.abs() * r * (dd + d.abs() * rel) + 1.5 * EPS32 * ((d * r * g).abs() + b.abs())
    return y.reshape(B, T, C), (2.0 * first).reshape(B, T, C)


def _gn_block_sum(v, n):
    """block_sum of norm.hip over the first n entries of v (.., n) fp32: thread i adds entries i, i + 256, .. in order, each wave reduces by the
    xor butterfly (offsets 32 .. 1), the four wave sums are added left to right."""
    k = (n + 255) // 256
    pad = torch.zeros(*v.shape[:-1], k * 256, dtype=torch.float32)
    pad[..., :n] = v
    pad = pad.reshape(*v.shape[:-1], k, 256)
    s = pad[..., 0, :].clone()
    for j in range(1, k):
        s = s + pad[..., j, :]
    s = s.reshape(*v.shape[:-1], 4, 64)
    lane = torch.arange(64)
    o = 32
    while o:
        s = s + s[..., lane ^ o]
        o >>= 1
    w = s[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def gn_emulate(x, G, eps, pilot, fault=None):
    """fp32 torch emulation of gn_stats_kernel / gn_apply_kernel in their own summation order (32-row chunks, _gn_block_sum, two-pass inside the
    chunk, Chan's merge over the chunks in order).  pilot False: the arithmetic before the fix (chunk means of x itself, one fp32 each); True: every
    value is first centred on the unit's own first element, x[b, 0, g cpg].  fault "full_count": the last, partial chunk is merged with the count
    of a full one.  Returns (x - mean) rstd (B, T, C) fp32."""
    B, T, C = x.shape
    cpg = C // G
    xg = x.float().reshape(B, T, G, cpg).permute(0, 2, 1, 3).contiguous()       # (B, G, T, cpg)
    if pilot:
        xg = xg - xg[:, :, :1, :1]
    mean = torch.zeros(B, G)
    m2 = torch.zeros(B, G)
    cnt = 0.0
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    for t0 in range(0, T, GN_ROWS):
        nr = min(GN_ROWS, T - t0)
        n = nr * cpg
        c = xg[:, :, t0:t0 + nr].reshape(B, G, n)
        mb = _gn_block_sum(c, n) / f32(float(n))
        dc = c - mb[..., None]
        qb = _gn_block_sum(dc * dc, n)
        nb = float(GN_ROWS * cpg if fault == "full_count" else n)
        tot = cnt + nb
        dlt = mb - mean
        mean = mean + dlt * (f32(nb) / f32(tot))
        m2 = m2 + (qb + dlt * dlt * (f32(cnt) * f32(nb) / f32(tot)))
        cnt = tot
    rstd = torch.rsqrt(m2 / f32(cnt) + f32(eps))
    y = (xg - mean[..., None, None]) * rstd[..., None, None]
    return y.permute(0, 2, 1, 3).reshape(B, T, C)


# ----------------------------------------------------------------------------- speaker encoder kernels (csrc/speaker.hip)
FLT_EPSILON = 2.0 ** -23


def _spk_gather(A, ti, fi, in_len, fill=None):
    """A (B, T_in, F_in, cin) -> (B, T_out, F_out, cin): the rows (ti[t], fi[f]); positions outside [0, in_len[b]) x [0, F_in) give 0 (or
    ``fill`` (cin,)), whatever A holds there or at the clamped index (NaN included)."""
    B, T_in, F_in, _ = A.shape
    okt = (ti >= 0)[None] & (ti[None] < in_len[:, None])
    okf = (fi >= 0) & (fi < F_in)
    g = A[:, ti.clamp(0, T_in - 1)][:, :, fi.clamp(0, F_in - 1)]
    ok = okt[:, :, None, None] & okf[None, None, :, None]
    other = torch.zeros((), dtype=A.dtype) if fill is None else fill.to(A.dtype)
    return torch.where(ok, g, other)


def _spk_taps(c):
    tt, ff = torch.arange(c["T_out"]), torch.arange(c["F_out"])
    kf, kt = c["k"]
    for i_f in range(kf):
        for i_t in range(kt):
            yield i_f, i_t, tt * c["s"][1] + i_t * c["dt"] - c["pad"][1], ff * c["s"][0] + i_f - c["pad"][0]


def spk_conv_ref64(c, x, w, in_len, out_len, pre=None, bias=None, res=None, gate=None):
    """cv_spk_conv as include/cosyvoice_amd.h states it, float64, from the fp32 operands.  c: dict(T_out, F_out, k (kf, kt), s (sf, st), pad (pf,
    pt), dt, relu, gate_seg); x (B, T_in, F_in, cin) (rows at and past in_len may hold anything), w (N, kf, kt, cin), in_len / out_len (B,) long,
    pre (scale, shift), bias (N,), res (B, T_out, F_out, N) (rows past out_len may hold anything), gate (B, segments, N).  Returns ref (B, T_out,
    F_out, N), rows >= out_len zero, and its bound: rule 2 with n = kf kt cin, plus one term each for the prologue fma, the bias, the residual
    and the gate product."""
    f64 = torch.float64
    B = x.shape[0]
    kf, kt = c["k"]
    cin, N = x.shape[-1], w.shape[0]
    A = x.double()
    extras = 0
    if pre is not None:
        A = torch.clamp(A * pre[0].double() + pre[1].double(), min=0)
        extras += 1
    acc = torch.zeros(B, c["T_out"], c["F_out"], N, dtype=f64)
    sabs = torch.zeros_like(acc)
    for i_f, i_t, ti, fi in _spk_taps(c):
        g = _spk_gather(A, ti, fi, in_len)
        wt = w[:, i_f, i_t].double()
        acc += g @ wt.t()
        sabs += g.abs() @ wt.abs().t()
    live = (torch.arange(c["T_out"])[None] < out_len[:, None])[:, :, None, None]
    if bias is not None:
        acc, sabs, extras = acc + bias.double(), sabs + bias.double().abs(), extras + 1
    if res is not None:
        r = torch.where(live, res.double(), torch.zeros((), dtype=f64))
        acc, sabs, extras = acc + r, sabs + r.abs(), extras + 1
    if c.get("relu"):
        acc = torch.clamp(acc, min=0)
    if gate is not None:
        seg = torch.arange(c["T_out"]) // c["gate_seg"]
        gg = torch.where(live, gate.double()[:, seg][:, :, None, :], torch.zeros((), dtype=f64))
        acc, sabs, extras = acc * gg, sabs * gg.abs(), extras + 1
    ref = torch.where(live, acc, torch.zeros((), dtype=f64))
    assert bool(torch.isfinite(ref).all())
    bound = torch.where(live, sum_bound(kf * kt * cin + extras, sabs, ref, torch.float32), torch.zeros((), dtype=f64))
    return ref, bound


def spk_conv_emulate(c, x, w, in_len, out_len, pre=None, bias=None, res=None, gate=None, fault=None):
    """fp32 torch emulation of spk_conv_kernel: the prologue as one fma, K in the kernel's order (taps outer, 16 channels per step; cin = 1: all
    taps in one step), then bias, residual, ReLU, gate, rows >= out_len zero; psum = ((v0 + v1) + v2) + v3 of the stored rows.  Returns y, psum
    (B, ceil(T_out / 4), N) (F_out == 1) or None.  Faults: "pre_on_pad" (padded taps contribute relu(shift)), "past_len" (rows >= in_len read),
    "no_dilation", "sf_on_time" (the frequency stride applied to time and the time stride to frequency), "gate_shift" (segment index of frame
    t + 1), "psum_all_rows" (psum counts rows >= out_len)."""
    f32 = torch.float32
    B, T_in = x.shape[0], x.shape[1]
    kf, kt = c["k"]
    cin, N = x.shape[-1], w.shape[0]
    c = dict(c)
    if fault == "no_dilation":
        c["dt"] = 1
    if fault == "sf_on_time":
        c["s"] = (c["s"][1], c["s"][0])
    if fault == "past_len":
        in_len = torch.full_like(in_len, T_in)
    A, fill = x.float(), None
    if pre is not None:
        A = torch.clamp((A.double() * pre[0].double() + pre[1].double()).float(), min=0)
        if fault == "pre_on_pad":
            fill = torch.clamp(pre[1].float(), min=0)
    acc = torch.zeros(B, c["T_out"], c["F_out"], N, dtype=f32)
    if cin == 1:
        G = torch.cat([_spk_gather(A, ti, fi, in_len, fill) for _, _, ti, fi in _spk_taps(c)], -1)
        acc = acc + G @ w.reshape(N, kf * kt).t()
    else:
        for i_f, i_t, ti, fi in _spk_taps(c):
            g = _spk_gather(A, ti, fi, in_len, fill)
            for c0 in range(0, cin, 16):
                acc = acc + g[..., c0:c0 + 16] @ w[:, i_f, i_t, c0:c0 + 16].t()
    tt = torch.arange(c["T_out"])
    live = (tt[None] < out_len[:, None])[:, :, None, None]
    v = acc
    if bias is not None:
        v = v + bias
    if res is not None:
        v = v + torch.where(live, res.float(), torch.zeros(()))
    if c.get("relu"):
        v = torch.clamp(v, min=0)
    if gate is not None:
        seg = ((tt + 1 if fault == "gate_shift" else tt) // c["gate_seg"]).clamp(max=gate.shape[1] - 1)
        v = v * torch.where(live, gate.float()[:, seg][:, :, None, :], torch.zeros(()))
    y = torch.where(live, v, torch.zeros(()))
    psum = None
    if c["F_out"] == 1:
        src = v if fault == "psum_all_rows" else y
        G4 = (c["T_out"] + 3) // 4
        p = torch.zeros(B, 4 * G4, N)
        p[:, :c["T_out"]] = src[:, :, 0]
        p = p.reshape(B, G4, 4, N)
        psum = ((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]) + p[:, :, 3]
    return y, psum


def spk_psum_ref64(y):
    """The 4-row group sums of the rows a launch stored (y (B, T_out, N)), float64, and rule 2 with n = 4 on them."""
    B, T, N = y.shape
    G4 = (T + 3) // 4
    p = torch.zeros(B, 4 * G4, N, dtype=torch.float64)
    p[:, :T] = y.double()
    p = p.reshape(B, G4, 4, N)
    ref = p.sum(2)
    return ref, sum_bound(4, p.abs().sum(2), ref, torch.float32)


def spk_gate_ref64(ps, lens, T, seg_len, w1, b1, w2, b2):
    """cv_spk_cam_gate in float64 from the group sums ps (B, groups, 128) (groups at and past ceil(len / 4) may hold anything).  Returns gate
    (B, ceil(T / seg_len), 32) — segments at and past a length zero — its bound, and e32 of the sigmoid.  Bound: rule 2 on the two group sums
    (n = the groups each spans) and the two divisions, pushed through |w1|, rule 2 with n = 128 + 1, through |w2|, rule 2 with n = 64 + 1, then
    the sigmoid: Lipschitz 1 / 4 and rule 3 (expf and the reciprocal)."""
    f64 = torch.float64
    B = ps.shape[0]
    nseg = (T + seg_len - 1) // seg_len
    ref, bound = torch.zeros(B, nseg, 32, dtype=f64), torch.zeros(B, nseg, 32, dtype=f64)
    W1, W2 = w1.double(), w2.double()
    vs, live = [], []
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        groups = (n + 3) // 4
        p = ps[b, :groups].double()
        for s in range(nseg):
            if s * seg_len >= n:
                continue
            g0, g1 = s * (seg_len // 4), min(groups, (s + 1) * (seg_len // 4))
            cnt = min(seg_len, n - s * seg_len)
            tot, seg = p.sum(0), p[g0:g1].sum(0)
            ctx = tot / n + seg / cnt
            bctx = ((groups + 2) * EPS32 * p.abs().sum(0) / n + (g1 - g0 + 2) * EPS32 * p[g0:g1].abs().sum(0) / cnt
                    + EPS32 * ((tot / n).abs() + (seg / cnt).abs()) + 0.5 * EPS32 * ctx.abs())
            pre = W1 @ ctx + b1.double()
            bh = W1.abs() @ bctx + sum_bound(129, W1.abs() @ (ctx.abs() + bctx) + b1.double().abs(), pre, torch.float32)
            hid = torch.clamp(pre, min=0)
            v = W2 @ hid + b2.double()
            bv = W2.abs() @ bh + sum_bound(65, W2.abs() @ (hid + bh) + b2.double().abs(), v, torch.float32)
            ref[b, s], bound[b, s] = torch.sigmoid(v), 0.25 * bv
            vs.append(v)
            live.append((b, s))
    e32 = torch.zeros((), dtype=f64)
    if vs:
        v = torch.stack(vs)
        e32 = (torch.sigmoid(v.float()).double() - torch.sigmoid(v.float().double())).abs().max()
        for (b, s) in live:
            bound[b, s] += act_bound(e32, ref[b, s])
    return ref, bound, e32.item()


def spk_gate_emulate(ps, lens, T, seg_len, w1, b1, w2, b2, fault=None):
    """fp32 torch emulation of spk_cam_gate_kernel: group sums in 4 slices (groups i = slice mod 4, in order) added in slice order, the hidden
    layer in 8 slices of 16 channels, the output in 8 slices of 8, partials added to the bias in slice order, 1 / (1 + exp(-v)).  fault "seg_len":
    the last segment is divided by seg_len instead of its valid frames."""
    B = ps.shape[0]
    nseg = (T + seg_len - 1) // seg_len
    out = torch.zeros(B, nseg, 32)

    def sliced(p):
        parts = []
        for ph in range(4):
            a = torch.zeros(128)
            for i in range(ph, p.shape[0], 4):
                a = a + p[i]
            parts.append(a)
        return ((parts[0] + parts[1]) + parts[2]) + parts[3]
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        groups = (n + 3) // 4
        p = ps[b, :groups].float()
        for s in range(nseg):
            if s * seg_len >= n:
                continue
            g0, g1 = s * (seg_len // 4), min(groups, (s + 1) * (seg_len // 4))
            cnt = seg_len if fault == "seg_len" else min(seg_len, n - s * seg_len)
            ctx = sliced(p) / float(n) + sliced(p[g0:g1]) / float(cnt)
            h = b1.float().clone()
            for sl in range(8):
                h = h + w1[:, sl * 16:(sl + 1) * 16].float() @ ctx[sl * 16:(sl + 1) * 16]
            hid = torch.clamp(h, min=0)
            v = b2.float().clone()
            for sl in range(8):
                v = v + w2[:, sl * 8:(sl + 1) * 8].float() @ hid[sl * 8:(sl + 1) * 8]
            out[b, s] = 1.0 / (1.0 + torch.exp(-v))
    return out


def spk_pool_ref64(x, lens, pre=None):
    """cv_spk_stats_pool in float64: [mean | unbiased std] over t < len of a = relu(x scale + shift) (x itself without pre); x (B, T, C), every
    len >= 2.  Returns ref (B, 2 C), its first-order bound (derivation: module docstring of tests/test_speaker_ops_gpu.py) and e32 of sqrt."""
    f64 = torch.float64
    B, T, Cc = x.shape
    ref, bound = torch.zeros(B, 2 * Cc, dtype=f64), torch.zeros(B, 2 * Cc, dtype=f64)
    stds = []
    for b in range(B):
        n = int(lens[b])
        a = x[b, :n].double()
        da = torch.zeros_like(a)
        if pre is not None:
            a = torch.clamp(a * pre[0].double() + pre[1].double(), min=0)
            da = 0.5 * EPS32 * a
        mu = a.sum(0) / n
        d = a - mu
        q = (d * d).sum(0)
        var = q / (n - 1)
        std = torch.sqrt(var)
        dmu = ((n + 2) * EPS32 * a.abs().sum(0) + da.sum(0)) / n + 0.5 * EPS32 * mu.abs()
        dd = dmu + da + 0.5 * ulp(d, torch.float32)
        dq = (n + 2) * EPS32 * q + 2.0 * (d.abs() * dd).sum(0)
        dvar = 2.0 * (dq / (n - 1) + 0.5 * EPS32 * var)
        dstd = torch.minimum(dvar / (2.0 * std).clamp_min(1e-300), torch.sqrt(dvar))
        ref[b] = torch.cat([mu, std])
        bound[b] = torch.cat([2.0 * dmu, dstd])
        stds.append(var)
    v32 = torch.stack(stds).float()
    e32 = (torch.sqrt(v32).double() - torch.sqrt(v32.double())).abs().max()
    bound[:, Cc:] += act_bound(e32, ref[:, Cc:])
    return ref, bound, e32.item()


def spk_pool_emulate(x, lens, pre=None, fault=None):
    """fp32 torch emulation of spk_stats_kernel: 4 row phases (t = phase mod 4, in order) added in phase order, two passes, sqrt(q / (n - 1)).
    fault "biased": q / n."""
    B, T, Cc = x.shape
    out = torch.zeros(B, 2 * Cc)

    def phased(a):
        parts = []
        for ph in range(4):
            s = torch.zeros(Cc)
            for t in range(ph, a.shape[0], 4):
                s = s + a[t]
            parts.append(s)
        return ((parts[0] + parts[1]) + parts[2]) + parts[3]
    for b in range(B):
        n = int(lens[b])
        a = x[b, :n].float()
        if pre is not None:
            a = torch.clamp((a.double() * pre[0].double() + pre[1].double()).float(), min=0)
        mean = phased(a) / float(n)
        d = a - mean
        out[b] = torch.cat([mean, torch.sqrt(phased(d * d) / float(n if fault == "biased" else n - 1))])
    return out


def spk_log_cmn_ref64(mel, lens, cmn):
    """cv_spk_log_cmn in float64: log(max(mel, FLT_EPSILON)) (- its mean over t < len when cmn), rows >= len zero; mel (B, T, n_mels) (rows at and
    past a length may hold anything).  Bound: rule 3 for logf, rule 2 (n = len terms) + the division for the mean, one rounding for the
    difference.  Returns ref, bound, e32."""
    f64 = torch.float64
    B, T, nm = mel.shape
    ref, bound = torch.zeros(B, T, nm, dtype=f64), torch.zeros(B, T, nm, dtype=f64)
    m32 = torch.clamp(torch.nan_to_num(mel.float(), nan=1.0), min=FLT_EPSILON)
    e32 = (torch.log(m32).double() - torch.log(m32.double())).abs().max()
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        if n == 0:
            continue
        l = torch.log(torch.clamp(mel[b, :n].double(), min=FLT_EPSILON))
        bl = 4.0 * torch.maximum(e32, EPS32 * l.abs())
        if cmn:
            mean = l.sum(0) / n
            bmean = ((n + 2) * EPS32 * l.abs().sum(0) + bl.sum(0)) / n + 0.5 * EPS32 * mean.abs()
            ref[b, :n] = l - mean
            bound[b, :n] = bl + bmean + 0.5 * ulp(ref[b, :n], torch.float32)
        else:
            ref[b, :n], bound[b, :n] = l, bl
    return ref, bound, e32.item()


def spk_log_cmn_emulate(mel, lens, cmn, fault=None):
    """fp32 torch emulation of spk_log_cmn_kernel: P = 1024 / n_mels row phases summed in order, partials added in phase order.  fault "mean_T":
    the mean runs over all T rows."""
    B, T, nm = mel.shape
    P = 1024 // nm
    out = torch.zeros(B, T, nm)
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        if n == 0:
            continue
        l = torch.log(torch.fmax(mel[b].float(), torch.tensor(FLT_EPSILON)))            # fmaxf: a NaN operand gives the other one
        if cmn:
            rows = T if fault == "mean_T" else n
            a = torch.zeros(nm)
            for ph in range(min(P, rows)):
                s = torch.zeros(nm)
                for t in range(ph, rows, P):
                    s = s + l[t]
                a = a + s
            l = l - a / float(max(rows, 1))
        out[b, :n] = l[:n]
    return out
