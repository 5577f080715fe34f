"""Op-level parity of the helper kernels (csrc/hift.hip, flow.hip, frontend.hip, llm.hip: cv_relpos_append) through the C ABI against
plain float64 torch references of the same operation, computed from the already rounded operands.

Every test pre-fills its outputs with NaN and checks that what the op must not write still holds it (guards), and poisons every input
location the op must not read with NaN (leaks).  Bounds (tests/_helpers.py):
  rule 1  data movement: bit-exact against the float64 reference cast to the output type;
  rule 2  fp32 sums of products: (n + 2) 2^-23 sum|terms| + half an ulp of the output type, element-wise;
  rule 3  transcendentals: 4 x max(e32, 2^-23 |ref|) element-wise, e32 = the L-inf error of torch's own fp32 CPU evaluation of the same
          inputs against float64 (one figure per case: an element-wise e32 is zero by chance where another rounding order is not), plus
          the project's stated hard caps (waveform 1e-4, Snake from sin_cw's 2e-7 claim).
The ``test_cpu_*`` functions carry no gpu mark: they check that torch's fp32 evaluation of every rule-2 case meets the same bound, so a
miss on the device is the kernel's."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

gpu = pytest.mark.gpu
DTS = [torch.float32, torch.bfloat16, torch.float16]
F64 = torch.float64


def _guarded(rows, ld, dt, guard=3):
    """(rows + guard, ld) NaN buffer and its first ``rows`` rows."""
    buf = H.nan_like((rows + guard, ld), dt)
    return buf, buf[:rows]


def _tail_is_nan(name, buf, rows):
    assert bool(torch.isnan(buf[rows:].float()).all()), f"{name}: rows past the end were written"


# ----------------------------------------------------------------------------- 1. layout changes
CL_SHAPES = [(1, 80, 1), (2, 80, 33), (3, 31, 64), (2, 513, 95), (1, 18, 2401)]


@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("B,Cc,T", CL_SHAPES)
def test_to_channels_last(B, Cc, T, wide, dt):
    from cosyvoice_amd import ops
    torch.manual_seed(B * 1000 + Cc + T)
    ldo = (Cc + 15) // 16 * 16 + 16 if wide else Cc
    x = torch.randn(B, Cc, T)
    buf, out = _guarded(B * T, ldo, dt)
    ops.to_channels_last(x.cuda(), out.view(B, T, ldo))
    torch.cuda.synchronize()
    o = out.view(B, T, ldo).cpu()
    ref = x.double().transpose(1, 2).to(dt)
    assert torch.equal(o[..., :Cc], ref), f"max|err| {(o[..., :Cc].double() - ref.double()).abs().max().item():.3e}"
    assert bool((o[..., Cc:] == 0).all()), "pad columns [C, ldo) must be zero"
    _tail_is_nan("to_channels_last", buf, B * T)


@gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("B,Cc,T", CL_SHAPES)
def test_to_channels_first(B, Cc, T, wide):
    from cosyvoice_amd import ops
    torch.manual_seed(B * 1000 + Cc + T + 1)
    ldx = (Cc + 15) // 16 * 16 + 16 if wide else Cc
    x = torch.randn(B, T, Cc)
    xin = H.nan_like((B, T, ldx), torch.float32)
    xin[..., :Cc] = x.cuda()
    buf, out = _guarded(B * Cc, T, torch.float32)
    ops.to_channels_first(xin, out.view(B, Cc, T))
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, Cc, T).cpu(), x.transpose(1, 2).contiguous())
    _tail_is_nan("to_channels_first", buf, B * Cc)
    # round trip cf(cl(x)) == x
    x_cf = out.view(B, Cc, T)
    cl, rt = H.nan_like((B, T, ldx), torch.float32), H.nan_like((B, Cc, T), torch.float32)
    ops.to_channels_last(x_cf, cl)
    ops.to_channels_first(cl, rt)
    torch.cuda.synchronize()
    assert torch.equal(rt.cpu(), x_cf.cpu())


# ----------------------------------------------------------------------------- 2. multi-alpha Snake
def _snake_inputs(rows, Cc, n, seed):
    """x (rows, C) fp32 and n alpha vectors: alpha log-uniform in [0.02, 30] (channel 3: alpha = 0 in every vector); y = x * alpha_max
    sweeps |y| log-spaced over [1e-6, 1e3] with both signs, points within 1e-3 of multiples of pi/2 up to 1e3, and x = 0."""
    g = torch.Generator().manual_seed(seed)
    alphas = [torch.exp(torch.rand(Cc, generator=g, dtype=F64) * math.log(30 / 0.02) + math.log(0.02)).float() for _ in range(n)]
    for a in alphas:
        a[3] = 0.0
        a[0], a[1] = 0.02, 30.0
    amax = torch.stack(alphas).max(0).values.double()
    N = rows * Cc
    i = torch.arange(N, dtype=F64)
    mag = 10 ** (-6 + 9 * ((i * 0.6180339887) % 1.0))                                   # log-spaced 1e-6 .. 1e3
    sign = torch.where((i.long() & 1) == 0, 1.0, -1.0).double()
    y = mag * sign
    k = torch.randint(-636, 637, (N,), generator=g).double()                           # |k pi/2| < 1e3
    near = k * (math.pi / 2) + (torch.rand(N, generator=g, dtype=F64) * 2 - 1) * 1e-3
    kind = torch.randint(0, 8, (N,), generator=g)
    y = torch.where(kind >= 5, near, y)
    y = torch.where(kind == 4, torch.zeros_like(y), y)
    y = y.reshape(rows, Cc)
    x = torch.where(amax > 0, y / amax.clamp_min(1e-30), y).float()
    x[:, 3] = y[:, 3].float().clamp(-50, 50)                                           # alpha = 0: any x, result exactly x
    return x, alphas


def _snake_ref(x, a):
    x, a = x.double(), a.double()
    return x + (1.0 / (a + 1e-9)) * torch.sin(x * a) ** 2


def _snake_cap(x, a, ref):
    """|err| <= 4.1e-7 / (alpha + 1e-9) + 2^-22 max(|x|, |ref|): sin_cw's 2e-7 absolute claim through s^2 / alpha, plus the roundings of
    x * alpha and of the sum."""
    return 4.1e-7 / (a.double() + 1e-9) + 2.0 ** -22 * torch.maximum(x.double().abs(), ref.abs())


@gpu
@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16", "split"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("Cc", [8, 64, 136])
@pytest.mark.parametrize("rows", [1, 7, 4097])
def test_snake_multi(rows, Cc, n, fmt):
    from cosyvoice_amd import ops
    x, alphas = _snake_inputs(rows, Cc, n, seed=rows * 7 + Cc + n)
    ldx, ldo = Cc + 8, Cc + 16
    xin = H.nan_like((rows, ldx), torch.float32)
    xin[:, :Cc] = x.cuda()
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "split": torch.float32}[fmt]
    bufs = [H.nan_split((rows + 2, ldo)) if fmt == "split" else H.nan_like((rows + 2, ldo), dt) for _ in range(n)]
    ops.snake_multi(xin[:, :Cc], [a.cuda() for a in alphas], [b[:rows, :Cc] for b in bufs], split=(fmt == "split"))
    torch.cuda.synchronize()
    odt = "split" if fmt == "split" else dt
    for k in range(n):
        raw = bufs[k].cpu()
        o = (H.unsplit(raw) if fmt == "split" else raw)
        ref = _snake_ref(x, alphas[k])
        t32 = x + (1.0 / (alphas[k] + 1e-9)) * torch.sin(x * alphas[k]) ** 2
        e32 = (t32.double() - ref).abs().max()
        half = 0.5 * H.ulp(ref, odt)
        H.check(f"snake_multi[{k}] [{fmt}] rule 3 (e32 {e32.item():.2e})", o[:rows, :Cc], ref, H.act_bound(e32, ref, odt))
        H.check(f"snake_multi[{k}] [{fmt}] sin_cw cap", o[:rows, :Cc], ref, _snake_cap(x, alphas[k], ref) + half)
        zero = alphas[k] == 0
        xz = x[:, zero]
        if fmt == "split":
            hi = xz.to(torch.bfloat16).float()
            xz = hi + (xz - hi).to(torch.bfloat16).float()
        assert torch.equal(o[:rows, :Cc][:, zero].float(), xz.to(dt).float()), "alpha = 0 must give exactly x"
        assert bool(torch.isnan(o[:rows, Cc:]).all()) and bool(torch.isnan(o[rows:]).all()), "snake_multi wrote outside [rows, C)"


# ----------------------------------------------------------------------------- 3. STFT
def _stft_case(S, B, sig):
    g = torch.Generator().manual_seed(S + B)
    if sig == "randn":
        s = torch.randn(B, S, generator=g)
    else:                                    # non-zero only in the first and last 8 samples: only the reflect branches contribute
        s = torch.zeros(B, S)
        s[:, :8] = torch.randn(B, 8, generator=g)
        s[:, -8:] = torch.randn(B, 8, generator=g)
    n = torch.arange(16, dtype=F64)
    win = 0.5 - 0.5 * torch.cos(2 * math.pi * n / 16)
    sp = torch.stft(s.double(), 16, 4, 16, window=win, center=True, pad_mode="reflect", return_complex=True)   # (B, 9, F)
    ref = torch.cat([sp.real, sp.imag], 1).transpose(1, 2).contiguous()                                       # (B, F, 18)
    fr = F.pad(s.double().abs()[:, None], (8, 8), mode="reflect")[:, 0].unfold(1, 16, 4) * win                # (B, F, 16) |w x|
    ang = 2 * math.pi * torch.outer(n, torch.arange(9, dtype=F64)) / 16
    sabs = torch.cat([fr @ torch.cos(ang).abs(), fr @ torch.sin(ang).abs()], -1)
    sp32 = torch.stft(s, 16, 4, 16, window=win.float(), center=True, pad_mode="reflect", return_complex=True)
    t32 = torch.cat([sp32.real, sp32.imag], 1).transpose(1, 2).contiguous()
    return s, ref, sabs, t32


STFT_S = [16, 20, 480, 9604, 240000]


@pytest.mark.parametrize("sig", ["randn", "edges"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", STFT_S)
def test_cpu_stft16_bound_holds_for_torch_fp32(S, B, sig):
    s, ref, sabs, t32 = _stft_case(S, B, sig)
    H.check("torch fp32 stft", t32, ref, H.sum_bound(16, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ldo", [18, 24, 32])
@pytest.mark.parametrize("sig", ["randn", "edges"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", STFT_S)
def test_stft16(S, B, sig, ldo, dt):
    from cosyvoice_amd import ops
    s, ref, sabs, _ = _stft_case(S, B, sig)
    Fr = S // 4 + 1
    buf, out = _guarded(B * Fr, ldo, dt)
    ops.stft16(s.cuda(), out.view(B, Fr, ldo))
    torch.cuda.synchronize()
    o = out.view(B, Fr, ldo).cpu()
    H.check(f"stft16 S={S} [{dt}]", o[..., :18], ref, H.sum_bound(16, sabs, ref, dt))
    assert bool((o[..., 18:] == 0).all()), "pad columns [18, ldo) must be zero"
    _tail_is_nan("stft16", buf, B * Fr)


# ----------------------------------------------------------------------------- 4. iSTFT
def _istft_ref(y, limit, dt):
    """oracle/hift.py::istft + the exp / sin front of decode() and the output clamp, evaluated in ``dt``."""
    y = y.to(dt)
    mag = torch.clip(torch.exp(y[..., :9]), max=1e2).transpose(1, 2)
    ph = torch.sin(y[..., 9:18]).transpose(1, 2)
    n = torch.arange(16, dtype=F64)
    win = (0.5 - 0.5 * torch.cos(2 * math.pi * n / 16)).to(dt)
    w = torch.istft(torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)), 16, 4, 16, window=win)
    return torch.clamp(w, -limit, limit)


@gpu
@pytest.mark.parametrize("limit", [0.99, 0.05])
@pytest.mark.parametrize("ldy", [18, 32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Fr", [2, 3, 64, 65, 66, 129, 60001])
def test_istft16(Fr, B, ldy, limit):
    from cosyvoice_amd import ops
    g = torch.Generator().manual_seed(Fr + B)
    y = torch.cat([torch.rand(B, Fr, 9, generator=g) * 14 - 8, torch.rand(B, Fr, 9, generator=g) * 20 - 10], -1)   # log-mag, phase pre-act
    assert bool((y[..., :9] > math.log(100)).any()) or Fr < 3
    yin = H.nan_like((B, Fr, ldy), torch.float32)
    yin[..., :18] = y.cuda()
    Lw = (Fr - 1) * 4
    buf, out = _guarded(B, Lw, torch.float32)
    ops.istft16(yin, out, limit)
    torch.cuda.synchronize()
    lim32 = torch.tensor(limit, dtype=torch.float32).item()
    ref = _istft_ref(y, lim32, F64)
    # e32 is taken BEFORE the clamp: the clamp is exact and 1-Lipschitz, so the error in front of it bounds the error behind it, while behind
    # it most samples are pinned to the limit and the few that are left make the maximum a matter of chance (at limit 0.05, 3 x 252 samples)
    big = float("inf")
    e32 = (_istft_ref(y, big, torch.float32).double() - _istft_ref(y, big, F64)).abs().max()
    o = out.cpu()
    assert bool((ref.abs() == lim32).any()) or limit > 0.5 or Fr < 64, "the output clamp must be active at the low limit"
    H.check(f"istft16 rule 3 (e32 {e32.item():.2e})", o, ref, H.act_bound(e32, ref))
    H.check("istft16 waveform cap 1e-4", o, ref, torch.full_like(ref, 1e-4))
    _tail_is_nan("istft16", buf, B)


# ----------------------------------------------------------------------------- 5. harmonic source
VTHR = 10.0


def _f0_track(kind, B, T, g):
    if kind == "const220":
        return torch.full((B, T), 220.0)
    if kind == "uniform":
        return torch.rand(B, T, generator=g) * 320 + 80
    if kind == "hi800":
        return torch.full((B, T), 800.0)
    f0 = torch.rand(B, T, generator=g) * 320 + 80                       # mixed voiced / unvoiced
    f0[torch.rand(B, T, generator=g) < 0.3] = 0.0
    thr = torch.tensor(VTHR)
    edge = torch.stack([thr, torch.nextafter(thr, torch.tensor(0.0)), torch.nextafter(thr, torch.tensor(100.0))])
    idx = torch.arange(T) % 7 == 3
    f0[:, idx] = edge[torch.arange(int(idx.sum())) % 3]
    return f0


@gpu
@pytest.mark.parametrize("nh", [1, 9, 16])
@pytest.mark.parametrize("up", [256, 480])
@pytest.mark.parametrize("T", [1, 20, 500, 1000])
@pytest.mark.parametrize("B", [1, 3])
def test_hift_source(B, T, up, nh):
    import dataclasses
    from cosyvoice_amd import ops
    from cosyvoice_amd.config import HiftConfig
    from oracle import hift as oh
    cfg = dataclasses.replace(HiftConfig.v2(), nb_harmonics=nh - 1, nsf_voiced_threshold=VTHR)
    sr, amp, sigma = float(cfg.sampling_rate), cfg.nsf_alpha, cfg.nsf_sigma
    S = T * up
    g = torch.Generator().manual_seed(B * 31 + T + up + nh)
    lin_w = torch.randn(1, nh, generator=g) / nh ** 0.5
    lin_b = torch.randn(1, generator=g) * 0.1
    sd = {"m_source.l_linear.weight": lin_w, "m_source.l_linear.bias": lin_b}
    for kind in ("const220", "uniform", "mixed", "hi800"):
        f0 = _f0_track(kind, B, T, g)
        pv = (torch.rand(B, nh, 1, generator=g) * 2 - 1) * math.pi          # a different phase vector per batch row
        noise = torch.randn(B, nh, S, generator=g)
        pv_dev = pv.clone()
        pv_dev[:, 0] = 1.0e4                                                  # harmonic 0 of phase_vec is ignored (generator.py:150)
        ref = H.source_ref64(f0, pv, noise, lin_w, lin_b, up, sr, amp, sigma, VTHR)
        f0u = f0.repeat_interleave(up, dim=1)[:, :, None]
        t32 = oh.source_module(sd, cfg, f0u, pv, noise, scan_dtype=F64)[..., 0]
        e32 = (t32.double() - ref).abs().max()
        work = torch.empty(B, nh, T, device="cuda", dtype=F64)
        buf, out = _guarded(B, S, torch.float32)
        ops.hift_source(f0.cuda(), pv_dev.reshape(B, nh).cuda(), noise.cuda(), lin_w.reshape(nh).cuda(), lin_b.cuda(), work, out, up, sr, amp,
                        sigma, VTHR)
        torch.cuda.synchronize()
        H.check(f"hift_source {kind} rule 3 (e32 {e32.item():.2e})", out.cpu(), ref, H.act_bound(e32, ref))
        _tail_is_nan("hift_source", buf, B)


# ----------------------------------------------------------------------------- 6. CFM helpers
@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 50, 1001])
@pytest.mark.parametrize("B", [1, 3])
def test_est_pack(B, T, dt):
    """[x | mu | spks | cond] rows of the conditional CFG pass and [x | 0 | 0 | 0] rows of the unconditional one (exact zeros: nothing of
    mu / spks / cond may reach them)."""
    from cosyvoice_amd import ops
    Cc = 80
    torch.manual_seed(B + T)
    x, mu, cond, spks = torch.randn(B, T, Cc), torch.randn(B, T, Cc), torch.randn(B, T, Cc), torch.randn(B, Cc)
    buf, out = _guarded(2 * B * T, 4 * Cc, dt)
    ops.est_pack(x.cuda(), mu.cuda(), spks.cuda(), cond.cuda(), out.view(2 * B, T, 4 * Cc))
    torch.cuda.synchronize()
    ref = torch.zeros(B, 2, T, 4, Cc, dtype=F64)
    for seg, src in enumerate((x, mu, spks[:, None].expand(B, T, Cc), cond)):
        ref[:, 0, :, seg] = src.double()
    ref[:, 1, :, 0] = x.double()                                     # unconditional CFG row: x only, mu / spks / cond zeroed
    assert torch.equal(out.cpu().view(B, 2, T, 4, Cc), ref.to(dt))
    _tail_is_nan("est_pack", buf, 2 * B * T)


def _cfm_case(B, T, dt_step, w):
    Cc = 80
    torch.manual_seed(B + T)
    x, v = torch.randn(B, T, Cc), torch.randn(2 * B, T, Cc)
    d, w = torch.tensor(dt_step, dtype=torch.float32), torch.tensor(w, dtype=torch.float32)
    vc, vu = v.view(B, 2, T, Cc)[:, 0], v.view(B, 2, T, Cc)[:, 1]
    ref = x.double() + d.double() * ((1 + w.double()) * vc.double() - w.double() * vu.double())
    sabs = x.double().abs() + d.double().abs() * ((1 + w.double()).abs() * vc.double().abs() + w.double().abs() * vu.double().abs())
    t32 = x + d * ((1 + w) * vc - w * vu)
    return x, v, ref, sabs, t32


CFM = [(r, d) for r in (0.0, 0.7) for d in (0.1, -0.0625)]


@pytest.mark.parametrize("w,dt_step", CFM)
@pytest.mark.parametrize("T", [1, 50, 1001])
@pytest.mark.parametrize("B", [1, 3])
def test_cpu_cfm_update_bound_holds_for_torch_fp32(B, T, w, dt_step):
    x, v, ref, sabs, t32 = _cfm_case(B, T, dt_step, w)
    H.check("torch fp32 cfm_update", t32, ref, H.sum_bound(3, sabs, ref, torch.float32))


@gpu
@pytest.mark.parametrize("w,dt_step", CFM)
@pytest.mark.parametrize("T", [1, 50, 1001])
@pytest.mark.parametrize("B", [1, 3])
def test_cfm_update(B, T, w, dt_step):
    from cosyvoice_amd import ops
    x, v, ref, sabs, _ = _cfm_case(B, T, dt_step, w)
    buf, xd = _guarded(B * T, 80, torch.float32)
    xd.copy_(x.view(B * T, 80))
    ops.cfm_update(xd.view(B, T, 80), v.cuda(), dt_step, w)
    torch.cuda.synchronize()
    H.check("cfm_update", xd.cpu().view(B, T, 80), ref, H.sum_bound(3, sabs, ref, torch.float32))
    _tail_is_nan("cfm_update", buf, B * T)


# ----------------------------------------------------------------------------- 7. embedding gather
@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("V,dim,ldo", [(100, 80, 96), (6561, 512, 520)])
def test_embedding(V, dim, ldo, dt):
    from cosyvoice_amd import ops
    torch.manual_seed(V)
    table = torch.randn(V, dim)
    idx = torch.tensor([0, V - 1, -1, -2, 5, -2, -1, V - 1, 0, 17, -2] * 13 + [V // 2], dtype=torch.int32)
    rows = idx.numel()
    buf, out = _guarded(rows, ldo, dt)
    ops.embedding(table.cuda(), idx.cuda(), out)
    torch.cuda.synchronize()
    o = out.cpu()
    il = idx.long()
    assert torch.equal(o[il >= 0][:, :dim], table[il[il >= 0]].double().to(dt)), "gathered rows"
    assert bool((o[il == -1][:, :dim] == 0).all()), "-1 rows are zero"
    assert bool(torch.isnan(o[il == -2].float()).all()), "-2 rows stay untouched"
    assert bool(torch.isnan(o[:, dim:].float()).all()), "pad columns [dim, ldo) stay untouched"
    _tail_is_nan("embedding", buf, rows)


# ----------------------------------------------------------------------------- 8. linear interpolation along T
def _interp_case(Ti, To, Cc):
    torch.manual_seed(Ti * 1000 + To + Cc)
    x = torch.randn(Ti, Cc)
    ref = F.interpolate(x.double().t()[None], size=To, mode="linear", align_corners=False)[0].t().contiguous()
    t32 = F.interpolate(x.t()[None], size=To, mode="linear", align_corners=False)[0].t().contiguous()
    src = ((torch.arange(To, dtype=F64) + 0.5) * Ti / To - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(Ti - 1)
    i1 = (i0 + 1).clamp_max(Ti - 1)
    l1 = (src - i0.double())[:, None]
    x0, x1 = x.double()[i0], x.double()[i1]
    sabs = (1 - l1) * x0.abs() + l1 * x1.abs()
    widx = (x1 - x0).abs() * (Ti + To) * 2.0 ** -22      # the source index is formed in fp32: the weight is off by <= (T_in + T_out) 2^-23
    return x, ref, t32, sabs, widx


INTERP = [(1, 5), (50, 100), (50, 173), (173, 50), (250, 250), (2, 1)]


@pytest.mark.parametrize("Cc", [80, 512])
@pytest.mark.parametrize("Ti,To", INTERP)
def test_cpu_interp_bound_holds_for_torch_fp32(Ti, To, Cc):
    x, ref, t32, sabs, widx = _interp_case(Ti, To, Cc)
    H.check("torch fp32 interpolate", t32, ref, H.sum_bound(2, sabs, ref, torch.float32) + widx)


@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cc", [80, 512])
@pytest.mark.parametrize("Ti,To", INTERP)
def test_interp_linear_cl(Ti, To, Cc, dt):
    from cosyvoice_amd import ops
    x, ref, t32, sabs, widx = _interp_case(Ti, To, Cc)
    xin = H.nan_like((Ti + 2, Cc + 8), torch.float32)
    xin[:Ti, :Cc] = x.cuda()
    buf = H.nan_like((To + 2, Cc + 24), dt)
    ops.interp_linear_cl(xin[:Ti, :Cc], buf[:To, :Cc])
    torch.cuda.synchronize()
    o = buf.cpu()
    H.check(f"interp_linear_cl [{dt}] vs float64", o[:To, :Cc], ref, H.sum_bound(2, sabs, ref, dt) + widx)
    H.check(f"interp_linear_cl [{dt}] vs torch fp32 (same index arithmetic)", o[:To, :Cc], t32, H.sum_bound(2, sabs, t32, dt))
    assert bool(torch.isnan(o[:, Cc:].float()).all()) and bool(torch.isnan(o[To:].float()).all()), "interp wrote outside (T_out, C)"


# ----------------------------------------------------------------------------- 9. prompt-feature front half
def _mag_case(rows):
    torch.manual_seed(rows)
    nb = 961
    spec = torch.randn(rows, 2 * nb) * torch.logspace(-6, 2, 2 * nb)
    spec[0, :4] = 0.0
    spec[0, nb:nb + 4] = 0.0                                           # re = im = 0: sqrt(eps)
    eps = torch.tensor(1e-9, dtype=torch.float32)
    s = spec.double()[:, :nb] ** 2 + spec.double()[:, nb:] ** 2 + eps.double()
    ref = s.sqrt()
    t32 = torch.sqrt(spec[:, :nb] * spec[:, :nb] + spec[:, nb:] * spec[:, nb:] + eps)
    # rule 2 through the square root: the three-term sum s = re^2 + im^2 + eps (all >= 0) errs by <= 5 * 2^-23 s; d sqrt(s) = ds / (2 sqrt(s))
    # = 2.5 * 2^-23 ref; sqrtf itself <= 1 ulp = 2^-23 ref: (n + 2) 2^-23 ref + half an ulp of the output covers both
    bound = 5 * H.EPS32 * ref + 0.5 * H.ulp(ref, torch.float32)
    return spec, ref, t32, bound


@pytest.mark.parametrize("rows", [1, 300, 3001])
def test_cpu_stft_magnitude_bound_holds_for_torch_fp32(rows):
    spec, ref, t32, bound = _mag_case(rows)
    H.check("torch fp32 magnitude", t32, ref, bound)


@gpu
@pytest.mark.parametrize("ld_mag", [961, 992])
@pytest.mark.parametrize("rows", [1, 300, 3001])
def test_stft_magnitude(rows, ld_mag):
    from cosyvoice_amd import _lib as L
    spec, ref, _, bound = _mag_case(rows)
    nb, ld_spec = 961, 1928
    sin = H.nan_like((rows, ld_spec), torch.float32)
    sin[:, :2 * nb] = spec.cuda()
    buf, out = _guarded(rows, ld_mag, torch.float32)
    L.check(L.lib().cv_stft_magnitude(C.c_void_p(sin.data_ptr()), ld_spec, C.c_void_p(out.data_ptr()), ld_mag, rows, nb, C.c_float(1e-9),
                                      L.stream_ptr()), "cv_stft_magnitude")
    torch.cuda.synchronize()
    o = out.cpu()
    H.check("stft_magnitude", o[:, :nb], ref, bound)
    assert bool((o[:, nb:] == 0).all()), "pad columns [nbins, ld_mag) are documented as zero"
    _tail_is_nan("stft_magnitude", buf, rows)


@gpu
@pytest.mark.parametrize("ld", [80, 88])
@pytest.mark.parametrize("B,T,n_mels", [(1, 1, 80), (3, 95, 80), (2, 1500, 80)])
def test_log_clamp_channels_first(B, T, n_mels, ld):
    from cosyvoice_amd import _lib as L
    torch.manual_seed(B + T)
    clip = torch.tensor(1e-5, dtype=torch.float32)
    mel = torch.exp(torch.randn(B, T, n_mels) * 6 - 8)                 # spans far below and far above clip
    mel.view(-1)[::7] = clip                                           # exactly at clip
    mel.view(-1)[1::7] = torch.nextafter(clip, torch.tensor(0.0))      # just below
    mel.view(-1)[2::7] = torch.nextafter(clip, torch.tensor(1.0))      # just above
    mel.view(-1)[3::49] = 0.0
    min_ = H.nan_like((B, T, ld), torch.float32)
    min_[..., :n_mels] = mel.cuda()
    buf, out = _guarded(B * n_mels, T, torch.float32)
    L.check(L.lib().cv_log_clamp_channels_first(C.c_void_p(min_.data_ptr()), ld, C.c_void_p(out.data_ptr()), B, T, n_mels, C.c_float(1e-5),
                                                L.stream_ptr()), "cv_log_clamp_channels_first")
    torch.cuda.synchronize()
    ref = torch.log(torch.clamp(mel.double(), min=clip.double())).transpose(1, 2)
    e32 = (torch.log(torch.clamp(mel, min=clip)).transpose(1, 2).double() - ref).abs().max()
    H.check(f"log_clamp rule 3 (e32 {e32.item():.2e})", out.view(B, n_mels, T).cpu(), ref, H.act_bound(e32, ref))
    _tail_is_nan("log_clamp_channels_first", buf, B * n_mels)


# ----------------------------------------------------------------------------- 10. v1 LM cache append
@gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("t", [0, 5, 71])
@pytest.mark.parametrize("D", [512, 1024])
def test_relpos_append(D, t, dt):
    from cosyvoice_amd import _lib as L
    ctx = 72
    torch.manual_seed(D + t)
    qkv = torch.randn(4 * D)
    qin = H.nan_like((4 * D + 64,), torch.float32)
    qin[:4 * D] = qkv.cuda()
    qq, kc, vtc = H.nan_like((2 * D + 32,), dt), H.nan_like((ctx, D), dt), H.nan_like((D, ctx), dt)
    L.check(L.lib().cv_relpos_append(C.c_void_p(qin.data_ptr()), C.c_void_p(qq.data_ptr()), C.c_void_p(kc.data_ptr()),
                                     C.c_void_p(vtc.data_ptr()), L.TORCH_DT[dt], D, t, ctx, L.stream_ptr()), "cv_relpos_append")
    torch.cuda.synchronize()
    r = qkv.double().to(dt)
    qq, kc, vtc = qq.cpu(), kc.cpu(), vtc.cpu()
    assert torch.equal(qq[:2 * D], r[:2 * D]) and bool(torch.isnan(qq[2 * D:].float()).all()), "query pair"
    assert torch.equal(kc[t], r[2 * D:3 * D]), "K cache row t"
    assert torch.equal(vtc[:, t], r[3 * D:]), "V^T cache column t"
    other = torch.ones(ctx, dtype=torch.bool)
    other[t] = False
    assert bool(torch.isnan(kc[other].float()).all()) and bool(torch.isnan(vtc[:, other].float()).all()), "the rest of the caches is untouched"
