"""GPU: cv_lora_shrink / cv_lora_expand (include/cosyvoice_amd_lora.h) against float64 references formed from the 16-bit-rounded operands.

Written from the header's contract.  Bounds (tests/_helpers.py, no hand-tuned tolerance):

  shrink   u[row][j] = sum_k A_a[j][k] x[row][k], fp32 accumulation of K products, fp32 output:
               b_u = sum_bound(K, sum_k |A x|, u, fp32)                                                   (rule 2, n = K)
  expand   d = s_a sum_j B_a[n][j] u[j]; the reference uses the float64 u, the kernel its own, which is off by at most b_u: r products,
           then the multiply by s_a and (ADD) the sum with y count as one more term, and the error of u passes through |s_a| |B|:
               b_y = sum_bound(r + 1, |s_a| sum_j |B u| (+ |y0|), ref, fp32) + |s_a| sum_j |B[n][j]| b_u[j]      (rule 2, n = r + 1)
  SWIGLU   g' = g + d_gate and up' = up + d_up carry b_g, b_up as above (ADD).  h = silu(g') up' rounded to the 16-bit type:
               b_silu = ACT_LIPSCHITZ["SILU"] b_g + act_bound(e32, silu(g'))          (rule 3; e32: torch's own fp32 error of silu)
               b_h    = b_silu (|up'| + b_up) + |silu(g')| b_up + 2^-23 |h| + ulp16(h) / 2

Rows with adapter -1: shrink writes zeros, STORE writes zeros, ADD leaves the row bit-unchanged, SWIGLU applies no term.  Every output
buffer is NaN-filled with guard rows and pitch slack; the bank has four slots, the one no row names holds NaN (so does its scale); x has
NaN pitch slack.  Row independence: every row of a 33-row launch is bit-equal to the same row launched alone."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _helpers import ACT_LIPSCHITZ, EPS32, act_bound, bits, check, nan_like, sum_bound, ulp, window_only

pytestmark = pytest.mark.gpu

SLOT_PATTERN = (0, 2, -1, 2, 1)
N_SLOTS = 4
SCALES = (1.0, 2.0, 0.5, float("nan"))


def _segments(kind, r):
    """(N, segments, ldo) of the column layouts the LM uses."""
    if kind == "n128":
        return 128, [(0, 128, 0)], 128
    if kind == "qkv":            # q 896 | k 128 | v 128 of the full-size LM, one launch
        return 1152, [(0, 896, 0), (896, 1024, r), (1024, 1152, 2 * r)], 1152
    if kind == "head":           # the 6564-way head in its 16-padded pitch
        return 6564, [(0, 6564, 0)], 6576
    if kind == "swiglu":
        return 1024, [(0, 512, 0), (512, 1024, r)], 1024
    raise ValueError(kind)


def _case(K, r, kind, rows, rps, dt, seed=0):
    g = torch.Generator().manual_seed(1000 * K + 10 * r + rows + seed)
    N, segs, ldo = _segments(kind, r)
    R_tot = len(segs) * r
    n_seq = (rows + rps - 1) // rps
    adapters = torch.tensor([SLOT_PATTERN[i % len(SLOT_PATTERN)] for i in range(n_seq)], dtype=torch.int32)
    x = torch.randn(rows, K, generator=g).to(dt)
    A = (torch.randn(N_SLOTS, R_tot, K, generator=g) / K ** 0.5).to(dt)
    B = (torch.randn(N_SLOTS, N, r, generator=g) / r ** 0.5).to(dt)
    A[3], B[3] = float("nan"), float("nan")          # the slot no row names is never read
    y0 = torch.randn(rows, N, generator=g)
    return dict(K=K, r=r, N=N, segs=segs, ldo=ldo, R_tot=R_tot, rows=rows, rps=rps, adapters=adapters, x=x, A=A, B=B,
                s=torch.tensor(SCALES, dtype=torch.float32), y0=y0, dt=dt)


def _row_slots(c):
    return c["adapters"][torch.arange(c["rows"]) // c["rps"]].long()


def _ref_shrink(c):
    """u (rows, R_tot) float64 and its bound; zeros for base-only rows."""
    a = _row_slots(c)
    live = a >= 0
    Aa = c["A"].double()[a.clamp_min(0)]                                   # (rows, R_tot, K)
    xd = c["x"].double()
    u = torch.einsum("rjk,rk->rj", Aa, xd)
    sabs = torch.einsum("rjk,rk->rj", Aa.abs(), xd.abs())
    u, sabs = torch.where(live[:, None], u, torch.zeros_like(u)), torch.where(live[:, None], sabs, torch.zeros_like(sabs))
    return u, sum_bound(c["K"], sabs, u, torch.float32)


def _ref_delta(c, u, bu):
    """d (rows, N) float64 = s_a B_a u over the segments, sum|terms| and the part of the bound that u's own error contributes."""
    a = _row_slots(c)
    live = (a >= 0)[:, None]
    Ba = c["B"].double()[a.clamp_min(0)]                                   # (rows, N, r)
    sa = c["s"].double()[a.clamp_min(0)].abs()[:, None]
    sgn = c["s"].double()[a.clamp_min(0)][:, None]
    d, sabs, prop = [torch.zeros(c["rows"], c["N"], dtype=torch.float64) for _ in range(3)]
    r = c["r"]
    for b, e, off in c["segs"]:
        d[:, b:e] = torch.einsum("rnj,rj->rn", Ba[:, b:e], u[:, off:off + r])
        sabs[:, b:e] = torch.einsum("rnj,rj->rn", Ba[:, b:e].abs(), u[:, off:off + r].abs())
        prop[:, b:e] = torch.einsum("rnj,rj->rn", Ba[:, b:e].abs(), bu[:, off:off + r])
    z = torch.zeros_like(d)
    return torch.where(live, sgn * d, z), torch.where(live, sa * sabs, z), torch.where(live, sa * prop, z)


def _run_shrink(c, rows=None, row0=0):
    """Launch over rows [row0, row0 + rows) of the case (whole sequences when rps > 1); returns the u buffer with guards."""
    from cosyvoice_amd import ops
    rows = c["rows"] if rows is None else rows
    xb = nan_like((rows, c["K"] + 8), c["dt"])
    xb[:, :c["K"]] = c["x"][row0:row0 + rows].cuda()
    ub = nan_like((rows + 2, c["R_tot"] + 4), torch.float32)
    ra = c["adapters"][row0 // c["rps"]:].contiguous().cuda()
    ops.lora_shrink(xb, c["A"].cuda(), ra, ub, rows, c["rps"])
    return ub, ra


def _run_expand(c, ub, ra, mode, rows=None, row0=0):
    from cosyvoice_amd import _lib as L, ops
    rows = c["rows"] if rows is None else rows
    Bd, sd = c["B"].cuda(), c["s"].cuda()
    if mode == L.LORA_SWIGLU:
        I = c["N"] // 2
        gu = c["y0"][row0:row0 + rows].cuda().contiguous()
        gu0 = gu.clone()
        hb = nan_like((rows + 2, I + 8), c["dt"])
        ops.lora_expand(ub, Bd, sd, ra, gu, rows, c["rps"], mode=mode, segments=c["segs"], h=hb)
        assert torch.equal(bits(gu), bits(gu0)), "SWIGLU wrote its fp32 input"
        return hb
    yb = nan_like((rows + 2, c["ldo"]), torch.float32)
    if mode == L.LORA_ADD:
        yb[:rows, :c["N"]] = c["y0"][row0:row0 + rows].cuda()
    ops.lora_expand(ub, Bd, sd, ra, yb, rows, c["rps"], mode=mode, segments=c["segs"])
    return yb


def _check_chain(c, mode, name):
    from cosyvoice_amd import _lib as L
    rows, N, R_tot = c["rows"], c["N"], c["R_tot"]
    live = _row_slots(c) >= 0
    ub, ra = _run_shrink(c)
    out = _run_expand(c, ub, ra, mode)
    torch.cuda.synchronize()
    u_ref, bu = _ref_shrink(c)
    window_only(name + " u", ub, rows, 0, R_tot)
    ug = ub[:rows, :R_tot].cpu()
    check(name + " shrink", ug, u_ref, bu)
    assert bool((ug[~live] == 0).all()), "shrink: a base-only row is not zero"
    d, dabs, prop = _ref_delta(c, u_ref, bu)
    if mode == L.LORA_SWIGLU:
        I = N // 2
        window_only(name + " h", out, rows, 0, I)
        y0 = c["y0"].double().view(rows, I // 16, 2, 16)
        g0, up0 = y0[:, :, 0].reshape(rows, I), y0[:, :, 1].reshape(rows, I)
        g, up = g0 + d[:, :I], up0 + d[:, I:]
        bg = sum_bound(c["r"] + 1, dabs[:, :I] + g0.abs(), g, torch.float32) + prop[:, :I]
        bup = sum_bound(c["r"] + 1, dabs[:, I:] + up0.abs(), up, torch.float32) + prop[:, I:]
        bg, bup = torch.where(live[:, None], bg, torch.zeros_like(bg)), torch.where(live[:, None], bup, torch.zeros_like(bup))
        silu = g * torch.sigmoid(g)
        e32 = (torch.nn.functional.silu(g.float()).double() - silu).abs()
        bs = ACT_LIPSCHITZ["SILU"] * bg + act_bound(e32, silu)
        h = silu * up
        bh = bs * (up.abs() + bup) + silu.abs() * bup + EPS32 * h.abs() + 0.5 * ulp(h, c["dt"])
        check(name + " swiglu", out[:rows, :I].float().cpu(), h, bh)
        return
    window_only(name + " y", out, rows, 0, N)
    yg = out[:rows, :N].cpu()
    if mode == L.LORA_ADD:
        ref = c["y0"].double() + d
        bound = sum_bound(c["r"] + 1, dabs + c["y0"].double().abs(), ref, torch.float32) + prop
        assert torch.equal(bits(yg[~live]), bits(c["y0"][~live])), "ADD changed a base-only row"
        if live.any():
            check(name + " add", yg[live], ref[live], bound[live])
    else:
        bound = sum_bound(c["r"] + 1, dabs, d, torch.float32) + prop
        assert bool((yg[~live] == 0).all()), "STORE: a base-only row is not zero"
        check(name + " store", yg, d, bound)


CASES = [  # K, r, column layout, rows, rows_per_seq, mode
    (256, 8, "n128", 1, 1, "ADD"),
    (896, 16, "qkv", 5, 1, "ADD"),
    (896, 16, "head", 16, 1, "ADD"),
    (4864, 32, "n128", 17, 1, "STORE"),
    (896, 16, "swiglu", 33, 1, "SWIGLU"),
    (896, 32, "qkv", 21, 7, "ADD"),
    (4864, 16, "n128", 33, 1, "STORE"),
    (256, 8, "swiglu", 21, 7, "SWIGLU"),
    (896, 8, "head", 33, 1, "ADD"),
    (4864, 16, "n128", 21, 7, "ADD"),
]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,r,kind,rows,rps,mode", CASES)
def test_cv_lora_shrink_expand_parity(K, r, kind, rows, rps, mode, dt):
    from cosyvoice_amd import _lib as L
    c = _case(K, r, kind, rows, rps, dt)
    _check_chain(c, getattr(L, "LORA_" + mode), f"K{K} r{r} {kind} rows{rows}/{rps} {mode}")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind,mode", [("qkv", "ADD"), ("n128", "STORE"), ("swiglu", "SWIGLU")])
def test_cv_lora_row_is_bit_identical_alone(kind, mode, dt):
    """Every row of a 33-row launch equals, bit for bit, the same row launched alone with its own adapter."""
    from cosyvoice_amd import _lib as L
    m = getattr(L, "LORA_" + mode)
    c = _case(896, 16, kind, 33, 1, dt, seed=5)
    ub, ra = _run_shrink(c)
    out = _run_expand(c, ub, ra, m)
    cols = c["N"] // 2 if mode == "SWIGLU" else c["N"]
    for row in range(33):
        u1, ra1 = _run_shrink(c, rows=1, row0=row)
        o1 = _run_expand(c, u1, ra1, m, rows=1, row0=row)
        assert torch.equal(bits(u1[0, :c["R_tot"]]), bits(ub[row, :c["R_tot"]])), f"shrink row {row}"
        assert torch.equal(bits(o1[0, :cols]), bits(out[row, :cols])), f"expand row {row}"


def test_cv_lora_rejects_what_the_header_excludes():
    """Unsupported shapes are refused by the wrappers' entry points before a launch (negative cv_status -> RuntimeError)."""
    from cosyvoice_amd import ops
    dt = torch.float16
    ra = torch.zeros(1, dtype=torch.int32, device="cuda")
    u = torch.zeros(1, 96, device="cuda")
    with pytest.raises(RuntimeError):      # K % 32
        ops.lora_shrink(torch.zeros(1, 48, dtype=dt, device="cuda"), torch.zeros(1, 16, 48, dtype=dt, device="cuda"), ra, u, 1)
    with pytest.raises(RuntimeError):      # r = 12
        ops.lora_expand(u, torch.zeros(1, 64, 12, dtype=dt, device="cuda"), torch.ones(1, device="cuda"), ra,
                        torch.zeros(1, 64, device="cuda"), 1)
    with pytest.raises(ValueError):        # four segments
        ops.lora_expand(u, torch.zeros(1, 64, 8, dtype=dt, device="cuda"), torch.ones(1, device="cuda"), ra,
                        torch.zeros(1, 64, device="cuda"), 1, segments=[(0, 16, 0), (16, 32, 0), (32, 48, 0), (48, 64, 0)])
