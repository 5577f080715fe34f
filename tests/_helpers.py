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
