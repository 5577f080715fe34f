"""Op-level parity of cv_groupnorm_cl (csrc/norm.hip) and cv_anti_alias_act / cv_anti_alias_act_cl (csrc/bigvgan.hip) through the C ABI against
float64 references computed on the CPU from the operands as stored (16-bit inputs rounded first), element-wise (H.check: no element is left
out), by the rules stated at the top of tests/test_helper_kernels_gpu.py.  Every pitch and batch stride has slack and guard rows follow every
batch; all of it is NaN before the launch, in inputs (what must not be read) and outputs (what must not be written); read-only inputs are
compared bit for bit afterwards.

GroupNorm (H.gn_units, H.gn_ref64).  The statistics span a (batch, group) unit of n = T C / G values, so the row kinds of H.flow_rows are given
to whole units: ordinary, x 30, common offset 100, common offset 1000, near-constant (variance 1e-6 against eps 1e-5), zero.
  The bound is SHIFT-INVARIANT: it is built from the centred values d = x - mu only and holds no term proportional to a common offset.  That is
  achievable in fp32 because the inputs are exact fp32 numbers: x - p for a datum p of the unit is exact where the offset dominates (Sterbenz)
  and otherwise rounds relative to |d| + max|d|.  With q = sum d^2, v = q / n + eps, r = v^-1/2, y = d r gamma + beta:
        dmu  = (nc + 2) 2^-23 sum|d| / n                     rule 2 on the centred sum
        dd_i = dmu + 2^-24 (|d_i| + max|d|) + half an ulp of d_i        (x - p) - mean: the centring and the subtraction round once each
        dq   = (nc + 2) 2^-23 q + 2 sum |d_i| dd_i           rule 2 on the squares + d(d^2) = 2 |d| dd
        dr / r = (dq / n + 2^-24 v) / (2 v) + 2 x 2^-23      as the LayerNorm bound of tests/test_flowblock_ops_gpu.py
        dy_i = |gamma_i| r (dd_i + |d_i| dr / r) + 1.5 x 2^-23 (|d_i r gamma_i| + |beta_i|)
  to first order; the bound is 2 dy.  nc (H.gn_chain) is the n of rule 2: the sums are evaluated in a FIXED tree (the header promises a fixed
  order: 256 strided partial sums per 32-row chunk, a 6-step butterfly, 4 wave sums, Chan's merge over the chunks), and a tree errs by its depth
  — the longest chain of additions, ceil(32 cpg / 256) + 9 + 4 per chunk — not by its n leaves; with n = T cpg (16000 at T = 500) rule 2 would
  allow 1.5e-3 and could not tell a mean carried in one fp32 (1e-4 at offset 1000) from a correct one.
  Then Mish by H.mish_bound (ACT_LIPSCHITZ x the interval + rule 3), one rounding for the add, half an ulp of a 16-bit output.
  The kernel before this module carried every chunk mean as one fp32 of x itself: H.gn_emulate(pilot=False) reproduces that arithmetic in its
  own summation order and test_cpu_groupnorm_old_arithmetic_misses asserts that it MISSES on the offset-1000 units; pilot=True, the arithmetic
  of the kernel as it is now (all sums of x - x[b, 0, g cpg]), meets the bound on every case.
  Faults (test_cpu_groupnorm_faults_miss): the last, partial chunk merged with the count of a full one; add before Mish.

Anti-aliased SnakeBeta (_aa_ref64: UpSample1d(2) -> SnakeBeta -> DownSample1d(2) with the replicate pads of oracle/bigvgan.py, float64, checked
once against the oracle and tests/golden/bigvgan_act.npz on the CPU).  alpha_log / beta_log sweep [-3, 3] per channel in opposite directions, so
1 / beta reaches 20 where alpha is 20.  With u the up-sampled signal, s = u + sin^2(u alpha) / beta:
        b_up = rule 2, n = 6, on 2 sum|x f|                                  (the x 2 is exact)
        b_s  = (1 + alpha / beta) b_up                                       |ds / du| = |1 + (alpha / beta) sin(2 u alpha)|
             + |u| dalpha / beta + sin^2 dinvb                               alpha = expf(alpha_log), 1 / (expf(beta_log) + 1e-9): rule 3 each
             + rule 3 on s (e32: torch's fp32 Snake at the fp32 u against float64)
        b_y  = sum_k |f_k| b_s + rule 2, n = 12, on sum|f_k s| + half an ulp of the output type
  Rows: N(0, 2), a constant row (channel 0 of batch 0) and a +-1 alternation (the last channel of batch 0): the two replicate clamps show
  most clearly on those.  The two layouts are also compared with each other: same data, |y_cf - y_cl| <= the sum of their bounds.
  Faults (test_cpu_anti_alias_faults_miss): zero padding instead of replicate; the halo one sample short at a tile boundary; the x 2 gain of
  the transposed conv dropped.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

gpu = pytest.mark.gpu
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
EPS = 1e-5

# ============================================================================= GroupNorm
GN_CASES = [(3, 1, 64, 4), (2, 31, 80, 1), (2, 32, 256, 8), (1, 33, 256, 8), (2, 65, 64, 64), (1, 500, 256, 8)]
GN_IDS = ["-".join(map(str, c)) for c in GN_CASES]
# name: (affine, mish, add: None / "C" / "BC", fp32 output, out_act dtype or None, in place)
GN_VARIANTS = {
    "f32-affine-mish-addC": (True, True, "C", True, None, False),
    "bf16+f32-affine-mish-addBC": (True, True, "BC", True, BF16, False),
    "f16-plain": (False, False, None, False, F16, False),
    "f32act-affine-addBC": (True, False, "BC", False, F32, False),
    "inplace-affine": (True, False, None, True, None, True),
}
GN_GUARD = 2


@functools.lru_cache(maxsize=None)
def _gn_data(ci):
    B, T, Cc, G = GN_CASES[ci]
    g = torch.Generator().manual_seed(40 + ci)
    # the kinds rotate from GN_KINDS[ci]: case 1 has two units only (x30, offset100), every other case holds every kind
    x, kinds = H.gn_units(B, T, Cc, G, g, start=ci)
    gamma, beta = 1 + 0.3 * torch.randn(Cc, generator=g), 0.5 * torch.randn(Cc, generator=g)
    add = torch.randn(B, Cc, generator=g)
    return x, kinds, gamma, beta, add


@functools.lru_cache(maxsize=None)
def _gn_expect(ci, vname):
    """ref and bound of the fp32 output and of the out_act output (None where the variant has none)."""
    affine, mish, add, _, adt, _ = GN_VARIANTS[vname]
    x, _, gamma, beta, addv = _gn_data(ci)
    y, by = H.gn_ref64(x, GN_CASES[ci][3], gamma if affine else None, beta if affine else None, EPS)
    if mish:
        y, by, _ = H.mish_bound(y, by)
    if add:
        a = (addv if add == "BC" else addv[:1]).double()[:, None, :]
        y = y + a
        by = by + 0.5 * H.ulp(y, F32)
    return y, by + 0.5 * H.ulp(y, F32), (None if adt is None else by + 0.5 * H.ulp(y, adt))


def _gn_mish32(y):
    """act_mish of cv_device.h in fp32 torch: x tanh(softplus(x)), softplus threshold 20."""
    return y * torch.tanh(torch.where(y > 20.0, y, torch.log1p(torch.exp(torch.clamp(y, max=20.0)))))


def _gn_emulated(ci, vname, pilot, fault=None):
    affine, mish, add, _, adt, _ = GN_VARIANTS[vname]
    x, _, gamma, beta, addv = _gn_data(ci)
    y = H.gn_emulate(x, GN_CASES[ci][3], EPS, pilot, fault="full_count" if fault == "full_count" else None)
    if affine:
        y = y * gamma + beta
    a = None if not add else (addv if add == "BC" else addv[:1])[:, None, :]
    if fault == "add_first" and a is not None:
        y = y + a
    if mish:
        y = _gn_mish32(y)
    if fault != "add_first" and a is not None:
        y = y + a
    return y, (None if adt is None else y.to(adt))


def _gn_checks(who, ci, vname, o32, oa):
    ref, b32, ba = _gn_expect(ci, vname)
    worst = 0.0
    if o32 is not None:
        worst = max(worst, H.check(f"{who} groupnorm {GN_IDS[ci]} {vname} fp32", o32, ref, b32)[1])
    if oa is not None:
        worst = max(worst, H.check(f"{who} groupnorm {GN_IDS[ci]} {vname} out_act", oa, ref, ba)[1])
    return worst


def _gn_unit_ratio(ci, got, ref, bound):
    """worst err / bound per (batch, group) unit, with the unit's kind."""
    B, T, Cc, G = GN_CASES[ci]
    r = ((got.double() - ref).abs() / bound).reshape(B, T, G, Cc // G).amax((1, 3)).reshape(-1)
    return list(zip(_gn_data(ci)[1], r.tolist()))


@gpu
@pytest.mark.parametrize("vname", list(GN_VARIANTS))
@pytest.mark.parametrize("ci", range(len(GN_CASES)), ids=GN_IDS)
def test_groupnorm_cl(ci, vname):
    from cosyvoice_amd import ops
    B, T, Cc, G = GN_CASES[ci]
    affine, mish, add, want32, adt, inplace = GN_VARIANTS[vname]
    x, _, gamma, beta, addv = _gn_data(ci)
    ldx, ld32, lda = Cc + 8, Cc + 4, Cc + 8
    xin = H.nan_like((B, T + GN_GUARD, ldx), F32)
    xin[:, :T, :Cc] = x.cuda()
    x0 = xin.clone()
    gd, bd = (gamma.cuda(), beta.cuda()) if affine else (None, None)
    addbuf = None
    if add:                                                       # (C,): one vector, add_ld 0; (B, C): rows of a wider NaN-padded buffer
        addbuf = H.nan_like((B, Cc + 12), F32)
        addbuf[:, :Cc] = addv.cuda()
        addarg = addbuf[:, :Cc] if add == "BC" else addbuf[0, :Cc]
    else:
        addarg = None
    o32 = xin if inplace else (H.nan_like((B, T + GN_GUARD, ld32), F32) if want32 else None)
    oa = H.nan_like((B, T + GN_GUARD, lda), adt) if adt is not None else None
    part = ops.groupnorm_workspace(B, T, G, "cuda")
    ops.groupnorm_cl(xin[:, :T, :Cc], G, gd, bd, EPS, part, act=ops.ACT_MISH if mish else ops.ACT_NONE, add=addarg,
                     out_f32=None if o32 is None else o32[:, :T, :Cc], out_act=None if oa is None else oa[:, :T, :Cc])
    torch.cuda.synchronize()
    for name, o in (("out_f32", o32), ("out_act", oa)):
        if o is None:
            continue
        m = torch.isnan(o.float())
        assert bool(m[:, T:].all()) and bool(m[:, :, Cc:].all()), f"{name}: written outside [B][T][C]"
    if not inplace:
        assert torch.equal(H.bits(xin), H.bits(x0)), "x was modified"
    if affine:
        assert torch.equal(gd.cpu(), gamma) and torch.equal(bd.cpu(), beta)
    if add:
        assert torch.equal(H.bits(addbuf[:, :Cc]).cpu(), H.bits(addv)) and bool(torch.isnan(addbuf[:, Cc:]).all())
    _gn_checks("MI355X", ci, vname, None if o32 is None else o32[:, :T, :Cc].cpu(), None if oa is None else oa[:, :T, :Cc].cpu())


@gpu
def test_groupnorm_cl_independent_of_batch_and_pitch():
    """A unit's result depends on nothing but its own values: each batch entry run alone, from a dense buffer, gives the same bits."""
    from cosyvoice_amd import ops
    ci = 4
    B, T, Cc, G = GN_CASES[ci]
    x, _, gamma, beta, _ = _gn_data(ci)
    xin = H.nan_like((B, T + GN_GUARD, Cc + 8), F32)
    xin[:, :T, :Cc] = x.cuda()
    full = H.nan_like((B, T, Cc), F32)
    ops.groupnorm_cl(xin[:, :T, :Cc], G, gamma.cuda(), beta.cuda(), EPS, ops.groupnorm_workspace(B, T, G, "cuda"), act=ops.ACT_MISH, out_f32=full)
    for b in range(B):
        one = H.nan_like((1, T, Cc), F32)
        ops.groupnorm_cl(x[b:b + 1].cuda(), G, gamma.cuda(), beta.cuda(), EPS, ops.groupnorm_workspace(1, T, G, "cuda"), act=ops.ACT_MISH,
                         out_f32=one)
        torch.cuda.synchronize()
        assert torch.equal(H.bits(one[0]), H.bits(full[b])), f"batch entry {b} alone differs"


@pytest.mark.parametrize("vname", list(GN_VARIANTS))
@pytest.mark.parametrize("ci", range(len(GN_CASES)), ids=GN_IDS)
def test_cpu_groupnorm_emulation_meets_bounds(ci, vname):
    o32, oa = _gn_emulated(ci, vname, pilot=True)
    want32 = GN_VARIANTS[vname][3]
    assert _gn_checks("fp32 emulation", ci, vname, o32 if want32 else None, oa) <= 1.0


def test_cpu_groupnorm_old_arithmetic_misses():
    """The arithmetic cv_groupnorm_cl had before (chunk means of x itself, one fp32 each), emulated in its own summation order, against the
    shift-invariant bound, per kind of unit.  It meets the bound on the ordinary, x30, offset-100 and zero units and MISSES on the units whose
    common offset is 500 or more times their spread: the offset-1000 units wherever the unit has at most three chunks, and the near-constant
    units (0.5 .. 16 + 1e-3 N(0, 1)) in every case.  Measured worst err / bound, offset-1000 | near-constant: 3-1-64-4: 3.3 | 10.6,
    2-32-256-8: 5.2 | 33, 1-33-256-8: 5.4 | 50, 2-65-64-64: 7.2 | 200, 1-500-256-8: 0.92 | 4.5.  In the 16-chunk case nc = 77 and the bound
    at d = 0 is 1.5e-5, which the offset-1000 unit's 5e-5 error of the mean, spread over gamma and Mish, just meets: there the miss is the
    near-constant unit's.  The centred arithmetic stays below 0.05 on every unit."""
    for ci in range(len(GN_CASES)):
        B, T, Cc, G = GN_CASES[ci]
        x, kinds, _, _, _ = _gn_data(ci)
        y, by = H.gn_ref64(x, G, None, None, EPS)
        per = _gn_unit_ratio(ci, H.gn_emulate(x, G, EPS, pilot=False), y, by)
        new = _gn_unit_ratio(ci, H.gn_emulate(x, G, EPS, pilot=True), y, by)
        worst = {k: max(r for kk, r in per if kk == k) for k in set(kinds)}
        print(f"groupnorm {GN_IDS[ci]}: one-fp32 chunk means, worst err / bound per kind", {k: round(v, 2) for k, v in worst.items()},
              "| centred:", round(max(r for _, r in new), 3))
        assert all(worst[k] <= 1.0 for k in ("ordinary", "x30", "offset100", "zero") if k in worst), worst
        assert all(r <= 1.0 for _, r in new)
        if "const" in worst:
            assert worst["const"] > 1.0, (GN_IDS[ci], worst)
        if "offset1000" in worst and T <= 3 * H.GN_ROWS:
            assert worst["offset1000"] > 1.0, (GN_IDS[ci], worst)
    for ci in (0, 2, 3, 4, 5):                                                     # and through the affine, Mish and the add
        vname = "f32-affine-mish-addC"
        assert H.worst_ratio(_gn_emulated(ci, vname, pilot=False)[0], *_gn_expect(ci, vname)[:2]) > 1.0, GN_IDS[ci]


def test_cpu_groupnorm_faults_miss():
    r1 = {GN_IDS[ci]: H.worst_ratio(_gn_emulated(ci, "f32-affine-mish-addC", True, "full_count")[0], *_gn_expect(ci, "f32-affine-mish-addC")[:2])
          for ci in range(len(GN_CASES))}
    r2 = {GN_IDS[ci]: H.worst_ratio(_gn_emulated(ci, "f32-affine-mish-addC", True, "add_first")[0], *_gn_expect(ci, "f32-affine-mish-addC")[:2])
          for ci in range(len(GN_CASES))}
    print("groupnorm fault full_count misses by", r1)
    print("groupnorm fault add_first misses by", r2)
    for cid in ("2-31-80-1", "1-33-256-8", "2-65-64-64", "1-500-256-8"):          # every case with a partial last chunk after a full one
        assert r1[cid] > 1.0, (cid, r1[cid])
    assert all(v > 1.0 for v in r2.values()), r2


# ============================================================================= anti-aliased SnakeBeta
AA_TT, AA_CT = 256, 32           # outputs per workgroup of the channels-first / channels-last kernel
AA_CF_T = [1, 2, 5, 6, 7, 255, 256, 257, 519]
AA_CF_C = [1, 3]
AA_CL_T = [1, 5, 31, 32, 33, 71]
AA_CL_C = [1, 63, 64, 65, 70]
AA_CL_DT = [(F32, F32), (F32, BF16), (F16, F16), (BF16, F32)]
AA_B = 2


def _filter12():
    from cosyvoice_amd.bigvgan import kaiser_sinc_filter12
    return kaiser_sinc_filter12()


@functools.lru_cache(maxsize=None)
def _aa_data(Cc, T, idt):
    g = torch.Generator().manual_seed(7000 + 31 * Cc + T)
    x = torch.randn(AA_B, Cc, T, generator=g) * 2
    x[0, 0] = 1.7                                                                # a constant row
    x[0, Cc - 1] = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0)              # +-1 alternation (C = 1: this one wins)
    sweep = torch.linspace(-3, 3, Cc) if Cc > 1 else torch.tensor([3.0])
    return x.to(idt).float(), sweep.clone(), (-sweep).clone()                    # alpha up, beta down: 1 / beta = 20 where alpha = 20


def _aa_pipeline(x, f, alpha, inv_beta, dt):
    """UpSample1d(2) -> x + inv_beta sin^2(x alpha) -> DownSample1d(2) in ``dt`` with torch's conv functions and the oracle's pads; returns u, s, y."""
    Cc = x.shape[1]
    fk = f.to(dt).view(1, 1, 12).expand(Cc, -1, -1)
    u = 2 * F.conv_transpose1d(F.pad(x.to(dt), (5, 5), mode="replicate"), fk, stride=2, groups=Cc)[..., 15:-15]
    sn = torch.sin(u * alpha.to(dt)[None, :, None])
    s = u + inv_beta.to(dt)[None, :, None] * sn * sn
    return u, s, F.conv1d(F.pad(s, (5, 6), mode="replicate"), fk, stride=2, groups=Cc)


@functools.lru_cache(maxsize=None)
def _aa_expect(Cc, T, idt, odt):
    """float64 reference (B, C, T) and its bound (module docstring)."""
    x, alog, blog = _aa_data(Cc, T, idt)
    f = _filter12()
    a64, ib64 = torch.exp(alog.double()), 1.0 / (torch.exp(blog.double()) + 1e-9)
    u, s, y = _aa_pipeline(x, f, a64, ib64, F64)
    fa = f.double().abs().view(1, 1, 12).expand(Cc, -1, -1)
    up_abs = 2 * F.conv_transpose1d(F.pad(x.double().abs(), (5, 5), mode="replicate"), fa, stride=2, groups=Cc)[..., 15:-15]
    b_up = (6 + 2) * H.EPS32 * up_abs
    a32, ib32 = torch.exp(alog), 1.0 / (torch.exp(blog) + 1e-9)
    da = 4.0 * torch.maximum((a32.double() - a64).abs().max(), H.EPS32 * a64)
    dib = 4.0 * torch.maximum((ib32.double() - ib64).abs().max(), H.EPS32 * ib64)
    u32 = u.float()
    sn32 = torch.sin(u32 * a64.float()[None, :, None])
    s32 = u32 + ib64.float()[None, :, None] * sn32 * sn32
    sn64 = torch.sin(u32.double() * a64.float().double()[None, :, None])
    e32 = (s32.double() - (u32.double() + ib64.float().double()[None, :, None] * sn64 * sn64)).abs().max()
    A, IB = a64[None, :, None], ib64[None, :, None]
    b_s = (1 + A * IB) * b_up + u.abs() * da[None, :, None] * IB + torch.sin(u * A) ** 2 * dib[None, :, None] \
        + 4.0 * torch.maximum(e32, H.EPS32 * s.abs())
    pad = lambda t: F.pad(t, (5, 6), mode="replicate")
    b_y = F.conv1d(pad(b_s), fa, stride=2, groups=Cc) + H.sum_bound(12, F.conv1d(pad(s.abs() + b_s), fa, stride=2, groups=Cc), y, odt)
    return y, b_y, e32.item()


def _aa_emulate(x, f, alog, blog, tile, fault=None):
    """fp32 torch, written from the definition as a gather: up[n] = 2 sum_i xp[i] f[n + 15 - 2 i] over the six i with a tap in range, xp[i] =
    x[clamp(i - 5)]; y[t] = sum_k s[clamp(2 t - 5 + k)] f[k].  Faults: "zero_pad" (both pads zero instead of replicate), "short_halo" (the
    last output of every ``tile`` reads its last tap one sample short), "no_gain" (the x 2 dropped)."""
    B, Cc, T = x.shape
    f = f.float()
    alpha, inv_beta = torch.exp(alog)[None, :, None], (1.0 / (torch.exp(blog) + 1e-9))[None, :, None]
    n = torch.arange(2 * T)
    ilo = (n + 5) >> 1
    acc = torch.zeros(B, Cc, 2 * T)
    for q in range(6):
        i = ilo + q
        k = n + 15 - 2 * i
        xi = i - 5
        v = x[..., xi.clamp(0, T - 1)]
        if fault == "zero_pad":
            v = torch.where((xi >= 0) & (xi < T), v, torch.zeros(()))
        acc = acc + v * f[k]
    u = acc if fault == "no_gain" else 2.0 * acc
    sn = torch.sin(u * alpha)
    s = u + inv_beta * sn * sn
    t = torch.arange(T)
    y = torch.zeros(B, Cc, T)
    for k in range(12):
        j = 2 * t - 5 + k
        if fault == "short_halo" and k == 11:
            j = torch.where(t % tile == tile - 1, j - 1, j)
        v = s[..., j.clamp(0, 2 * T - 1)]
        if fault == "zero_pad":
            v = torch.where((j >= 0) & (j < 2 * T), v, torch.zeros(()))
        y = y + v * f[k]
    return y


def _aa_check(who, Cc, T, idt, odt, y):
    ref, bound, e32 = _aa_expect(Cc, T, idt, odt)
    return H.check(f"{who} anti_alias C {Cc} T {T} {idt}->{odt} (e32 {e32:.2e})", y, ref, bound)[1]


def _aa_run_cf(Cc, T, dt):
    from cosyvoice_amd import _lib as L
    x, alog, blog = _aa_data(Cc, T, dt)
    f = _filter12().cuda()
    guard = 16
    xin = H.nan_like((AA_B * Cc * T + guard,), dt)                 # B C T dense (the form has no pitch): guards after the last row
    xin[:AA_B * Cc * T] = x.to(dt).reshape(-1).cuda()
    x0 = xin.clone()
    y = H.nan_like((AA_B * Cc * T + guard,), dt)
    a, b = alog.cuda(), blog.cuda()
    L.check(L.lib().cv_anti_alias_act(C.c_void_p(xin.data_ptr()), C.c_void_p(y.data_ptr()), L.TORCH_DT[dt], AA_B, Cc, T, C.c_void_p(f.data_ptr()),
                                      C.c_void_p(f.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), L.stream_ptr()),
            "cv_anti_alias_act")
    torch.cuda.synchronize()
    assert torch.equal(H.bits(xin), H.bits(x0)), "x was modified"
    assert bool(torch.isnan(y[AA_B * Cc * T:].float()).all()), "written past the last row"
    return y[:AA_B * Cc * T].reshape(AA_B, Cc, T).float().cpu()


def _aa_run_cl(Cc, T, idt, odt):
    from cosyvoice_amd.bigvgan import anti_alias_act_cl
    x, alog, blog = _aa_data(Cc, T, idt)
    f = _filter12().cuda()
    ldx, ldy, guard = Cc + 5, Cc + 3, 2
    xin = H.nan_like((AA_B * T + guard, ldx), idt)
    xin[:AA_B * T, :Cc] = x.transpose(1, 2).reshape(AA_B * T, Cc).to(idt).cuda()
    x0 = xin.clone()
    y = H.nan_like((AA_B * T + guard, ldy), odt)
    anti_alias_act_cl(xin[:AA_B * T].view(AA_B, T, ldx), y[:AA_B * T].view(AA_B, T, ldy), Cc, f, f.clone(), alog.cuda(), blog.cuda())
    torch.cuda.synchronize()
    assert torch.equal(H.bits(xin), H.bits(x0)), "x was modified"
    H.window_only("anti_alias_act_cl", y, AA_B * T, 0, Cc)
    return y[:AA_B * T, :Cc].reshape(AA_B, T, Cc).transpose(1, 2).float().cpu()


@gpu
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("Cc", AA_CF_C)
@pytest.mark.parametrize("T", AA_CF_T)
def test_anti_alias_act(T, Cc, dt):
    _aa_check("MI355X cf", Cc, T, dt, dt, _aa_run_cf(Cc, T, dt))


@gpu
@pytest.mark.parametrize("idt,odt", AA_CL_DT, ids=["f32-f32", "f32-bf16", "f16-f16", "bf16-f32"])
@pytest.mark.parametrize("Cc", AA_CL_C)
@pytest.mark.parametrize("T", AA_CL_T)
def test_anti_alias_act_cl(T, Cc, idt, odt):
    _aa_check("MI355X cl", Cc, T, idt, odt, _aa_run_cl(Cc, T, idt, odt))


@gpu
@pytest.mark.parametrize("dt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("Cc,T", [(3, 5), (3, 257), (65, 33), (1, 256)])
def test_anti_alias_layouts_agree(Cc, T, dt):
    """The two layouts on the same data differ by no more than the sum of their bounds (equal here: same types)."""
    ycf, ycl = _aa_run_cf(Cc, T, dt), _aa_run_cl(Cc, T, dt, dt)
    _, bound, _ = _aa_expect(Cc, T, dt, dt)
    H.check(f"anti_alias cf vs cl C {Cc} T {T} {dt}", ycf, ycl, 2.0 * bound)


def test_cpu_anti_alias_reference_matches_oracle_and_golden(golden_dir):
    from oracle import bigvgan as ob
    for Cc, T in [(3, 1), (3, 5), (3, 7), (3, 257), (65, 33)]:
        x, alog, blog = _aa_data(Cc, T, F32)
        ref, bound, _ = _aa_expect(Cc, T, F32, F32)
        H.check(f"oracle vs float64 reference C {Cc} T {T}", ob.anti_alias_activation(x, alog, blog), ref, bound)
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "bigvgan_act.npz")).items()}
    a64, ib64 = torch.exp(g["alpha_log"].double()), 1.0 / (torch.exp(g["beta_log"].double()) + 1e-9)
    y = _aa_pipeline(g["x"], _filter12(), a64, ib64, F64)[2]
    err = (y - g["y"].double()).abs().max().item()
    print(f"golden bigvgan_act vs float64 reference: max|err| {err:.3e}, max|y| {g['y'].abs().max().item():.3e}")
    assert err <= 2e-5                                                              # the tolerance test_bigvgan_gpu.py holds the kernel to


def _aa_all_cases():
    cases = [(Cc, T, dt, dt, AA_TT) for T in AA_CF_T for Cc in AA_CF_C for dt in (F32, BF16, F16)]
    return cases + [(Cc, T, i, o, AA_CT) for T in AA_CL_T for Cc in AA_CL_C for i, o in AA_CL_DT]


def test_cpu_anti_alias_emulation_meets_bounds():
    worst = 0.0
    for Cc, T, idt, odt, tile in _aa_all_cases():
        x, alog, blog = _aa_data(Cc, T, idt)
        y = _aa_emulate(x, _filter12(), alog, blog, tile).to(odt)
        worst = max(worst, H.worst_ratio(y, *_aa_expect(Cc, T, idt, odt)[:2]))
        assert worst <= 1.0, (Cc, T, idt, odt, worst)
    print(f"anti_alias fp32 emulation: worst err / bound over {len(_aa_all_cases())} cases {worst:.3f}")


def test_cpu_anti_alias_faults_miss():
    for fault in ("zero_pad", "short_halo", "no_gain"):
        miss = {}
        for Cc, T, idt, odt, tile in _aa_all_cases():
            if idt != F32 or odt != F32:
                continue
            x, alog, blog = _aa_data(Cc, T, idt)
            r = H.worst_ratio(_aa_emulate(x, _filter12(), alog, blog, tile, fault), *_aa_expect(Cc, T, idt, odt)[:2])
            miss[(Cc, T, tile)] = r
        print(f"anti_alias fault {fault}: misses by", {k: f"{v:.3g}" for k, v in miss.items() if v > 1.0})
        if fault == "short_halo":      # shows where a tile's last output has its last tap, sample 2 tile + 4, inside the signal: T >= tile + 3
            assert all((v > 1.0) == (T >= tile + 3) for (Cc, T, tile), v in miss.items()), (fault, miss)
            assert any(T >= tile + 3 for (Cc, T, tile) in miss if tile == AA_TT) and any(T >= tile + 3 for (Cc, T, tile) in miss if tile == AA_CT)
        else:
            assert all(v > 1.0 for v in miss.values()), (fault, miss)
