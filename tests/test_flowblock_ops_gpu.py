"""Op-level parity of the estimator's row-block kernels (csrc/flowblock.hip: cv_tblock_head, cv_tblock_tail, cv_tblock_tail_head,
cv_resblock_conv1 / conv2) through the C ABI against float64 references computed on the CPU from the operands already rounded to the 16-bit
type, element-wise (H.check: no element, row or case is left out), by the rules stated at the top of tests/test_helper_kernels_gpu.py.

Buffers.  Every pitch has slack (ldx 264, ldqk 1032, vt_ld round_up(T, 8) + 8, ldao 520, out_act at column 8 of a 264-wide buffer, lda cin + 8
and, for cin = 256, 512 = the first half of the estimator's ``cat``, ldh1 264, ldo 260) and GUARD rows follow the last sequence; all of it is
NaN before the launch, in inputs (what must not be read) and outputs (what must not be written: after the launch everything outside
[R][T][width], and the V^T columns [T, vt_ld), still holds NaN).  Read-only inputs are compared bit for bit after the launch.

Rows (H.flow_rows).  Every x / ao / a tensor holds ordinary rows 2 N(0, 1) + 0.3 and, in every sequence, one row x 30, one with a common offset
of 100, one near-constant row (c + 1e-3 N(0, 1): eps = 1e-5 dominates the variance) and one all-zero row, at rows T - 1, 0, T // 2 and 1 with
the kinds rotated per sequence, so the rows on both sides of a sequence boundary always differ in kind.  T = 1 has three rows in all: they are
the x 30, the offset and the near-constant row.

Bounds (nothing is fitted to the kernels: the constants are those of rules 2 and 3, H.ACT_LIPSCHITZ, the Abramowitz-Stegun figure 1.5e-7 that
gelu_erf states, and the factor 2 on first-order terms).
  16-bit intermediates (LayerNorm output, GELU output, h1 inside one launch) are carried UNROUNDED in float64 with an element-wise interval
      b_A = (fp32 bound of the value) + half an ulp of the operand type (H.carry16) and pushed through the next product as b_A |W|^T plus rule 2
      with n = K on (|A| + b_A) |W|^T: the reference never decides which way a value on a rounding boundary falls.
  Each launch is held to the float64 evaluation of ITS OWN inputs as the launch before stored them: conv2 from the h1 conv1 wrote, the head
      half of cv_tblock_tail_head from the x it stored (the kernel normalises its accumulators, which are that x bit for bit).
  LayerNorm over n = 256 (H.ln_ref64; ln_rows_to_lds and ln_acc: one fp32 mean, then centred squares).  With S = sum x, mu = S / n, d = x - mu,
      q = sum d^2, v = q / n + eps, r = v^-1/2, y = d r gamma + beta, and the input known to dx (0 for rows read from memory, the rule-2 bound of
      the accumulator where the rows are accumulators):
        dmu  = rule 2 (n terms) on S, / n            ~ (n + 2) 2^-23 mean|x_row|: rows with a common offset pay for it here
        dd_i = dmu + dx_i + mean(dx) + half an ulp of d_i
        dq   = rule 2 (n terms) on q + 2 sum |d_i| dd_i
        dr / r = (dq / n + 2^-24 v) / (2 v) + 2 x 2^-23      (d v^-1/2 = -v^-3/2 dv / 2; the eps sum rounds once; rsqrtf <= 2 ulp)
        dy_i = |gamma_i| r (dd_i + |d_i| dr / r) + 1.5 x 2^-23 (|d_i r gamma_i| + |beta_i|)      (two products and one sum, half an ulp each)
      to first order; the bound is 2 dy, the factor 2 covering the higher orders as in the RMSNorm prologue bound of test_llm_ops_gpu.py.
  GELU  H.gelu_bound: ACT_LIPSCHITZ["GELU"] x the pre-activation interval + rule 3 + 0.5 |x| 1.5e-7 + half an ulp; fp16 values the kernel may
      hold below 2^-14 may be rounded gradually or flushed (+ |g| there, as the ``sub`` term of H.attn_bound).
  Mish  H.mish_bound: ACT_LIPSCHITZ["MISH"] x the interval + rule 3; then one fp32 rounding for the time term (conv1) or two for the bias and
      the sum of the 1x1 conv (conv2: fl(fl(mish + br) + acc)), + half an ulp of the output type.
  Dense sums  rule 2 with n = 256 (head), 512 + 2 (out-projection + residual + bias), 256 + 1 (hidden layer), 1024 + 2 (FFN output + residual
      + bias), 3 cin + 1 (k3 conv), cin + 1 (1x1 conv).
  The tail's 16-bit copy out_act is the same accumulators rounded once: bit-identical to T(x as stored).

Isolation (zero tolerance).  At every explicit mt each sequence of the R = 3 batch is also run alone (R = 1): same instantiation, same per-row
arithmetic, so the outputs are bit-identical or data crossed a sequence or tile boundary.
Across mt.  Reading flowblock.hip: a row's LayerNorm is summed by the 16 lanes (ln_rows_to_lds) or the 4 lane groups x 8 waves (ln_acc) that own
that row, and every MFMA chain runs over the k-steps in the same order, whatever MT is — MT only sets how many 16-row tiles a workgroup carries.
No sum order depends on MT, so test_*_identical_across_mt ASSERTS that mt = 1 .. 4 give bit-identical outputs (and prints it).

CPU twins (``test_cpu_*``, no gpu mark): a plain-torch fp32 emulation of each kernel's arithmetic (``_emu_*``: fp32 LayerNorm with one mean,
rounding to dt where the kernel rounds, fp32 products, the erfc-polynomial GELU and the w / (w + 2) Mish of the kernel comments; the fused form
takes its statistics from the fp32 block output it holds) meets every bound on every GPU case, through the same ``_*_checks`` as the GPU tests.
test_cpu_injected_fault_misses: each fault misses a bound (both dtypes unless noted) in the case named:
  1 clamp0      causal conv reads the clamped row 0 instead of zeros before the start        resblock cin 256, T 5: h1
  2 prev_seq    conv of sequence r > 0 reads the last rows of sequence r - 1                  resblock cin 256, T 5: h1
  3 no_bo       bo omitted when ao is given                                                    tail ao, T 17: x
  4 tadd_first  time term added before Mish                                                    resblock cin 256, T 5: h1
  5 no_eps      eps dropped from the LayerNorm                                                 head T 16: [Q | K] (near-constant and zero rows)
  6 swap_tiles  output column tiles 1 and 2 swapped                                            head T 1: [Q | K]
  7 vt_straddle the V^T group that straddles T dropped                                         head T 5: V^T keeps its NaN
  8 ln_tile_row LN statistics of the tile's first row for rows >= T and row T - 1              head T 66, 64-row tiles: [Q | K] row 65
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

gpu = pytest.mark.gpu
DTS = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
F32, F64 = torch.float32, torch.float64
C_, INNER, FF = 256, 512, 1024
R, GUARD, EPS = 3, 3, 1e-5
LENGTHS = [1, 5, 16, 17, 47, 49, 64, 66, 131]          # both sides of every 16 / 32 / 48 / 64-row tile edge, a one-row last tile, T % 4 = 0..3
MTS = [(0, 0), (0, 192), (1, 0), (2, 0), (3, 0), (4, 0)]   # (mt, cus): mt = 0 is pick_mt's own choice, on the whole chip and on 192 CUs
MT_IDS = ["mt0", "mt0-cus192", "mt1", "mt2", "mt3", "mt4"]
LDX, LDQK, LDAO, LDOA, OA_COL, LDH1, LDO = 264, 1032, 520, 264, 8, 264, 260


def _vt_ld(T):
    return (T + 7) // 8 * 8 + 8


# ============================================================================= weights and inputs (CPU, fp32 values of the rounded operands)
@functools.lru_cache(maxsize=None)
def _tb_weights(dt, seed, sweep=False):
    """As test_tblock_gpu._weights: matrices scaled by fan-in and rounded to dt first; sweep: bf1 = linspace(-9, 9), so that GELU sees both
    tails and, on the negative side, fp16-subnormal outputs."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
    w = dict(g1=1 + 0.1 * r(C_), b1=0.1 * r(C_), wq=r(INNER, C_, sc=C_ ** -0.5), wk=r(INNER, C_, sc=C_ ** -0.5), wv=r(INNER, C_, sc=C_ ** -0.5),
             wo=r(C_, INNER, sc=INNER ** -0.5), bo=0.1 * r(C_), g3=1 + 0.1 * r(C_), b3=0.1 * r(C_),
             w1=r(FF, C_, sc=C_ ** -0.5), bf1=0.2 * r(FF), w2=r(C_, FF, sc=FF ** -0.5), bf2=0.1 * r(C_))
    if sweep:
        w["bf1"] = torch.linspace(-9, 9, FF)
    for k in ("wq", "wk", "wv", "wo", "w1", "w2"):
        w[k] = w[k].to(dt).float()
    w["wqkv"] = torch.cat([w["wq"], w["wk"], w["wv"]], 0)
    return w


@functools.lru_cache(maxsize=None)
def _tb_dev(dt, seed, sweep=False):
    from cosyvoice_amd import ops
    w = _tb_weights(dt, seed, sweep)
    d = {k: w[k].cuda() for k in ("g1", "b1", "bo", "g3", "b3", "bf1", "bf2")}
    for k, src in (("wqkv_p", "wqkv"), ("wo_p", "wo"), ("w1_p", "w1"), ("w2_p", "w2")):
        d[k] = ops.pack_skinny(w[src].to(dt).cuda().contiguous())
    return d


@functools.lru_cache(maxsize=None)
def _rb_weights(dt, cin, sweep=False):
    """As test_tblock_gpu.test_resblock_vs_torch; sweep: be1 / be2 = -25 .. 25, so that Mish sees inputs beyond the fminf(x, 20) clamp and
    far-negative ones."""
    g = torch.Generator().manual_seed(cin)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    w = dict(w1=r(C_, cin, 3, sc=(3 * cin) ** -0.5).to(dt).float(), w2=r(C_, C_, 3, sc=(3 * C_) ** -0.5).to(dt).float(),
             wr=r(C_, cin, sc=cin ** -0.5).to(dt).float(), b1=0.1 * r(C_), b2=0.1 * r(C_), br=0.1 * r(C_),
             g1=1 + 0.1 * r(C_), be1=0.1 * r(C_), g2=1 + 0.1 * r(C_), be2=0.1 * r(C_), tadd=0.3 * r(C_))
    if sweep:
        w["be1"], w["be2"] = torch.linspace(-25, 25, C_), torch.linspace(25, -25, C_)
    return w


@functools.lru_cache(maxsize=None)
def _rb_dev(dt, cin, sweep=False):
    from cosyvoice_amd import ops
    w = _rb_weights(dt, cin, sweep)

    def packed(wc):              # (Co, Ci, k) -> (Co, k * Ci) with k = tap * Ci + ci, K zero-padded to a multiple of 128
        wm = wc.permute(0, 2, 1).reshape(wc.shape[0], -1)
        kp = (wm.shape[1] + 127) // 128 * 128
        wp = torch.zeros(wc.shape[0], kp, dtype=dt)
        wp[:, :wm.shape[1]] = wm
        return ops.pack_skinny(wp.cuda().contiguous())
    d = {k: w[k].cuda() for k in ("b1", "b2", "br", "g1", "be1", "g2", "be2", "tadd")}
    d["w1_p"], d["w2_p"], d["wr_p"] = packed(w["w1"]), packed(w["w2"]), packed(w["wr"][:, :, None])
    return d


@functools.lru_cache(maxsize=None)
def _x_rows(T, seed):
    return H.flow_rows(R, T, C_, torch.Generator().manual_seed(seed + T))


@functools.lru_cache(maxsize=None)
def _ao_rows(T, dt):
    return H.flow_rows(R, T, INNER, torch.Generator().manual_seed(900 + T)).to(dt)


@functools.lru_cache(maxsize=None)
def _a_rows(T, cin, dt):
    return H.flow_rows(R, T, cin, torch.Generator().manual_seed(500 + cin + T)).to(dt)


# ============================================================================= float64 references and bounds
def _head_expect(x, w, dt):
    """x (R', T, 256) fp32 as stored -> [Q | K | V] reference (R', T, 1536) and bound."""
    y, by = H.ln_ref64(x, None, w["g1"], w["b1"], EPS)
    bA = H.carry16(y, by, dt)
    Wa = w["wqkv"].double().abs().t()
    ref = y @ w["wqkv"].double().t()
    return ref, bA @ Wa + H.sum_bound(C_, (y.abs() + bA) @ Wa, ref, dt)


@functools.lru_cache(maxsize=None)
def _head_expect_cached(T, dt):
    return _head_expect(_x_rows(T, 100), _tb_weights(dt, 0), dt)


def _head_checks(who, dt, qk, vt, exp):
    """qk (R', T, 1024), vt (R', 512, T) CPU tensors, whoever made them."""
    ref, bound = exp
    rq = H.check(f"{who} [Q | K]", qk, ref[..., :2 * INNER], bound[..., :2 * INNER])[1]
    rv = H.check(f"{who} V^T", vt, ref[..., 2 * INNER:].transpose(1, 2), bound[..., 2 * INNER:].transpose(1, 2))[1]
    return rq, rv


@functools.lru_cache(maxsize=None)
def _tail_expect(T, dt, with_ao, seed, sweep):
    w = _tb_weights(dt, seed, sweep)
    x = _x_rows(T, 300).double()
    if with_ao:
        ao = _ao_rows(T, dt).double()
        x1 = x + ao @ w["wo"].double().t() + w["bo"].double()
        dx1 = H.sum_bound(INNER + 2, x.abs() + ao.abs() @ w["wo"].double().abs().t() + w["bo"].double().abs(), x1, F32)
    else:
        x1, dx1 = x, torch.zeros_like(x)
    y, by = H.ln_ref64(x1, dx1 if with_ao else None, w["g3"], w["b3"], EPS)
    bA = H.carry16(y, by, dt)
    W1, W2 = w["w1"].double(), w["w2"].double()
    pre = y @ W1.t() + w["bf1"].double()
    bp = bA @ W1.abs().t() + H.sum_bound(C_ + 1, (y.abs() + bA) @ W1.abs().t() + w["bf1"].double().abs(), pre, F32)
    g, bg, e32 = H.gelu_bound(pre, bp, dt)
    ref = x1 + g @ W2.t() + w["bf2"].double()
    sabs = x1.abs() + dx1 + (g.abs() + bg) @ W2.abs().t() + w["bf2"].double().abs()
    return ref, dx1 + bg @ W2.abs().t() + H.sum_bound(FF + 2, sabs, ref, F32)


def _tail_checks(who, dt, xo, oa, exp):
    """xo (R', T, 256) fp32 as stored, oa its 16-bit copy or None."""
    ratio = H.check(f"{who} x", xo, *exp)[1]
    if oa is not None:
        assert torch.equal(H.bits(oa), H.bits(xo.to(dt))), f"{who}: out_act is not T(x as stored)"
    return ratio


def _conv_terms(a, w, bias):
    """float64 causal k3 conv + bias of exact operands: reference and sum |terms|."""
    a, w = a.double(), w.double()
    return H.causal_conv3_64(a, w) + bias.double(), H.causal_conv3_64(a.abs(), w.abs()) + bias.double().abs()


def _res_stage(a, wc, bias, gam, bet, n):
    """k3 conv (rule 2, n terms) -> LayerNorm from the accumulators -> Mish: value and fp32 bound."""
    c, sabs = _conv_terms(a, wc, bias)
    y, by = H.ln_ref64(c, H.sum_bound(n, sabs, c, F32), gam, bet, EPS)
    m, bm, _ = H.mish_bound(y, by)
    return m, bm


@functools.lru_cache(maxsize=None)
def _res1_expect(T, cin, dt, sweep):
    w = _rb_weights(dt, cin, sweep)
    m, bm = _res_stage(_a_rows(T, cin, dt), w["w1"], w["b1"], w["g1"], w["be1"], 3 * cin + 1)
    h = m + w["tadd"].double()
    b32 = bm + 0.5 * H.ulp(h.abs() + bm, F32)                      # fl(mish + tadd)
    return h, H.carry16(h, b32, dt)


def _res2_expect(h1, a, w, cin):
    """h1 (R', T, 256) 16-bit as conv1 stored it, a the block input."""
    m, bm = _res_stage(h1, w["w2"], w["b2"], w["g2"], w["be2"], 3 * C_ + 1)
    a64, wr, br = a.double(), w["wr"].double(), w["br"].double()
    r = a64 @ wr.t() + br
    ref = m + r
    dr = H.sum_bound(cin + 1, a64.abs() @ wr.abs().t() + br.abs(), r, F32)
    return ref, bm + dr + 0.5 * H.ulp(m.abs() + bm + br.abs(), F32) + 0.5 * H.ulp(ref.abs() + bm + dr, F32)   # fl(fl(mish + br) + acc)


# ============================================================================= fp32 emulations of the kernels' arithmetic (CPU twins)
def _emu_ln_rows(x, gam, bet, fault, T, mt):
    if fault == "no_eps":
        return H.ln_emulate(x, gam, bet, 0.0)
    if fault == "ln_tile_row":       # rows >= T are never stored; row T - 1 takes the statistics of its tile's first row
        src = x.clone()
        src[:, T - 1] = x[:, (T - 1) // (16 * mt) * (16 * mt)]
        return H.ln_emulate(x, gam, bet, EPS, stats_from=src)
    return H.ln_emulate(x, gam, bet, EPS)


def _emu_head(x, w, dt, fault=None, mt=4):
    T = x.shape[1]
    xn = _emu_ln_rows(x, w["g1"], w["b1"], fault, T, mt).to(dt).float()
    o = (xn @ w["wqkv"].t()).to(dt)
    if fault == "swap_tiles":
        o = torch.cat([o[..., :16], o[..., 32:48], o[..., 16:32], o[..., 48:]], -1)
    qk, vt = o[..., :2 * INNER].contiguous(), o[..., 2 * INNER:].transpose(1, 2).contiguous()
    if fault == "vt_straddle" and T % 4:
        vt[..., T - T % 4:] = float("nan")          # what the NaN-prefilled buffer keeps
    return qk, vt


def _emu_tail(x, ao, w, dt, fault=None):
    x1 = x if ao is None else x + ao.float() @ w["wo"].t() + (0.0 if fault == "no_bo" else w["bo"])
    xn = H.ln_emulate(x1, w["g3"], w["b3"], EPS).to(dt).float()
    h = H.gelu_emulate(xn @ w["w1"].t() + w["bf1"]).to(dt).float()
    xo = (x1 + w["bf2"]) + h @ w["w2"].t()
    return xo, xo.to(dt)


def _emu_conv3(a, wc, bias, fault=None):
    """a (R', T, Ci) fp32: rows t - 2, t - 1, t; before the start zeros (fault clamp0: row 0; prev_seq: the last rows of sequence r - 1)."""
    Rr, T, _ = a.shape
    pad = torch.zeros(Rr, 2, a.shape[2])
    if fault == "clamp0":
        pad = a[:, :1].expand(-1, 2, -1).clone()
    if fault == "prev_seq":
        flat = torch.cat([torch.zeros(2, a.shape[2]), a.reshape(Rr * T, -1)], 0)
        pad = torch.stack([flat[r * T:r * T + 2] for r in range(Rr)])
    ap = torch.cat([pad, a], 1)
    return sum(ap[:, k:k + T] @ wc[:, :, k].t() for k in range(3)) + bias


def _emu_res1(a, w, dt, fault=None):
    y = H.ln_emulate(_emu_conv3(a.float(), w["w1"], w["b1"], fault), w["g1"], w["be1"], EPS)
    h = H.mish_emulate(y + w["tadd"]) if fault == "tadd_first" else H.mish_emulate(y) + w["tadd"]
    return h.to(dt)


def _emu_res2(h1, a, w):
    y = H.ln_emulate(_emu_conv3(h1.float(), w["w2"], w["b2"]), w["g2"], w["be2"], EPS)
    return (H.mish_emulate(y) + w["br"]) + a.float() @ w["wr"].t()


# ============================================================================= device side
def _nanbuf(rows, ld, dt, data=None, col0=0):
    """(rows + GUARD, ld) of NaN on the device with ``data`` (.., width) in rows [0, rows), columns [col0, col0 + width)."""
    buf = H.nan_like((rows + GUARD, ld), dt)
    if data is not None:
        buf[:rows, col0:col0 + data.shape[-1]] = data.reshape(rows, -1).to(dt).cuda()
    return buf


def _unchanged(name, buf, before):
    assert torch.equal(H.bits(buf.cpu()), H.bits(before)), f"{name}: a read-only input was written"


def _window(buf, rows, c0, width, shape):
    return buf[:rows, c0:c0 + width].reshape(shape).contiguous()


def _launch_tblock(kind, x, ao, wd, wd_next, dt, mt, cus, with_oa=False):
    """kind: head | tail | tail_head.  x (R', T, 256) fp32, ao (R', T, 512) dt or None: CPU.  Checks guards, slack
    and read-only inputs; returns the CPU windows x, oa, qk (R', T, 1024), vt (R', 512, T) (None where the kind has none)."""
    from cosyvoice_amd import ops
    Rr, T, _ = x.shape
    rows = Rr * T
    xb = _nanbuf(rows, LDX, F32, x)
    x0 = xb.cpu()
    p = ops.tblock_params(xb, Rr, T, EPS, dt)
    assert p.ldx == LDX
    p.mt, p.cus = mt, cus
    qkb = vtb = aob = oab = None
    if kind != "tail":
        hw = wd if kind == "head" else wd_next
        qkb, vtb = _nanbuf(rows, LDQK, dt), _nanbuf(Rr * INNER, _vt_ld(T), dt)
        p.g1, p.b1n, p.wqkv_p = hw["g1"].data_ptr(), hw["b1"].data_ptr(), hw["wqkv_p"].data_ptr()
        p.qk, p.ldqk, p.vt, p.vt_ld = qkb.data_ptr(), LDQK, vtb.data_ptr(), _vt_ld(T)
    if kind != "head":
        if ao is not None:
            aob = _nanbuf(rows, LDAO, dt, ao)
            ao0 = aob.cpu()
            p.ao, p.ldao, p.wo_p, p.bo = aob.data_ptr(), LDAO, wd["wo_p"].data_ptr(), wd["bo"].data_ptr()
        p.g3, p.b3n = wd["g3"].data_ptr(), wd["b3"].data_ptr()
        p.w1_p, p.bf1, p.w2_p, p.bf2 = wd["w1_p"].data_ptr(), wd["bf1"].data_ptr(), wd["w2_p"].data_ptr(), wd["bf2"].data_ptr()
        if with_oa:
            oab = _nanbuf(rows, LDOA, dt)
            p.out_act, p.ldoa = oab.data_ptr() + OA_COL * 2, LDOA       # the last row ends with the buffer's last data row
    getattr(ops, "tblock_" + kind)(p)
    torch.cuda.synchronize()
    out = dict(x=None, oa=None, qk=None, vt=None)
    xc = xb.cpu()
    if kind == "head":
        _unchanged(f"{kind} x", xb, x0)
    else:
        H.window_only(f"{kind} x", xc, rows, 0, C_)
        out["x"] = _window(xc, rows, 0, C_, (Rr, T, C_))
        if aob is not None:
            _unchanged(f"{kind} ao", aob, ao0)
        if oab is not None:
            oc = oab.cpu()
            H.window_only(f"{kind} out_act", oc, rows, OA_COL, OA_COL + C_)
            out["oa"] = _window(oc, rows, OA_COL, C_, (Rr, T, C_))
    if qkb is not None:
        qc, vc = qkb.cpu(), vtb.cpu()
        H.window_only(f"{kind} qk", qc, rows, 0, 2 * INNER)
        H.window_only(f"{kind} vt", vc, Rr * INNER, 0, T)
        out["qk"] = _window(qc, rows, 0, 2 * INNER, (Rr, T, 2 * INNER))
        out["vt"] = _window(vc, Rr * INNER, 0, T, (Rr, INNER, T))
    return out


def _launch_resblock(a, wd, dt, cin, lda, mt, cus):
    """conv1 then conv2 on a (R', T, cin) dt CPU; returns the CPU windows h1 (R', T, 256) dt and out (R', T, 256) fp32."""
    from cosyvoice_amd import _lib as L
    from cosyvoice_amd import ops
    Rr, T, _ = a.shape
    rows = Rr * T
    ab, h1b, ob = _nanbuf(rows, lda, dt, a), _nanbuf(rows, LDH1, dt), _nanbuf(rows, LDO, F32)
    a0 = ab.cpu()
    p = L.ResblockParams()
    p.dtype, p.R, p.T, p.C, p.cin = L.TORCH_DT[dt], Rr, T, C_, cin
    p.a, p.lda = ab.data_ptr(), lda
    p.w1_p, p.b1, p.g1, p.be1, p.tadd = (wd[k].data_ptr() for k in ("w1_p", "b1", "g1", "be1", "tadd"))
    p.h1, p.ldh1 = h1b.data_ptr(), LDH1
    p.w2_p, p.b2, p.g2, p.be2 = (wd[k].data_ptr() for k in ("w2_p", "b2", "g2", "be2"))
    p.wr_p, p.br = wd["wr_p"].data_ptr(), wd["br"].data_ptr()
    p.out, p.ldo, p.eps = ob.data_ptr(), LDO, EPS
    p.mt, p.cus = mt, cus
    ops._issue("cv_resblock_conv1", p)
    torch.cuda.synchronize()
    h1c = h1b.cpu()
    ops._issue("cv_resblock_conv2", p)
    torch.cuda.synchronize()
    _unchanged("resblock a", ab, a0)
    _unchanged("conv2 h1", h1b, h1c)
    oc = ob.cpu()
    H.window_only("conv1 h1", h1c, rows, 0, C_)
    H.window_only("conv2 out", oc, rows, 0, C_)
    return _window(h1c, rows, 0, C_, (Rr, T, C_)), _window(oc, rows, 0, C_, (Rr, T, C_))


def _same(name, batch, alone, r):
    for k, v in alone.items():
        if v is not None:
            assert torch.equal(H.bits(batch[k][r:r + 1]), H.bits(v)), f"{name}: {k} of sequence {r} alone differs from its rows in the batch"


# ============================================================================= cases
TAIL_VARIANTS = {"ao+oa": (True, True), "ao": (True, False), "oa": (False, True), "plain": (False, False)}
TAIL_CASES = [(v, T, False) for v in TAIL_VARIANTS for T in LENGTHS] + [("oa", 17, True), ("ao+oa", 17, True)]
TAIL_IDS = [f"{v}-T{T}" + ("-gelu-sweep" if s else "") for v, T, s in TAIL_CASES]
RES_CASES = [(cin, lda, T, False) for cin, lda in ((256, 264), (256, 512), (320, 328), (512, 520)) for T in LENGTHS] + [(320, 328, 47, True)]
RES_IDS = [f"cin{c}-lda{l}-T{T}" + ("-mish-sweep" if s else "") for c, l, T, s in RES_CASES]


# ----------------------------------------------------------------------------- head
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("T", LENGTHS)
def test_cpu_head_emulation_meets_bound(T, dt):
    qk, vt = _emu_head(_x_rows(T, 100), _tb_weights(dt, 0), dt)
    _head_checks(f"emulation head T={T} [{dt}]", dt, qk, vt, _head_expect_cached(T, dt))


@gpu
@pytest.mark.parametrize("mt,cus", MTS, ids=MT_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("T", LENGTHS)
def test_head(T, dt, mt, cus):
    x, wd = _x_rows(T, 100), _tb_dev(dt, 0)
    o = _launch_tblock("head", x, None, wd, None, dt, mt, cus)
    _head_checks(f"head T={T} mt={mt} cus={cus} [{dt}]", dt, o["qk"], o["vt"], _head_expect_cached(T, dt))
    if mt:
        for r in range(R):
            _same(f"head T={T} mt={mt}", o, _launch_tblock("head", x[r:r + 1], None, wd, None, dt, mt, cus), r)


# ----------------------------------------------------------------------------- tail
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("variant,T,sweep", TAIL_CASES, ids=TAIL_IDS)
def test_cpu_tail_emulation_meets_bound(variant, T, sweep, dt):
    with_ao, _ = TAIL_VARIANTS[variant]
    xo, oa = _emu_tail(_x_rows(T, 300), _ao_rows(T, dt) if with_ao else None, _tb_weights(dt, 2, sweep), dt)
    _tail_checks(f"emulation tail {variant} T={T} [{dt}]", dt, xo, oa, _tail_expect(T, dt, with_ao, 2, sweep))


@gpu
@pytest.mark.parametrize("mt,cus", MTS, ids=MT_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("variant,T,sweep", TAIL_CASES, ids=TAIL_IDS)
def test_tail(variant, T, sweep, dt, mt, cus):
    with_ao, with_oa = TAIL_VARIANTS[variant]
    x, ao, wd = _x_rows(T, 300), (_ao_rows(T, dt) if with_ao else None), _tb_dev(dt, 2, sweep)
    o = _launch_tblock("tail", x, ao, wd, None, dt, mt, cus, with_oa)
    _tail_checks(f"tail {variant} T={T} mt={mt} cus={cus} [{dt}]", dt, o["x"], o["oa"], _tail_expect(T, dt, with_ao, 2, sweep))
    if mt:
        for r in range(R):
            _same(f"tail {variant} T={T} mt={mt}", o,
                  _launch_tblock("tail", x[r:r + 1], None if ao is None else ao[r:r + 1], wd, None, dt, mt, cus, with_oa), r)


# ----------------------------------------------------------------------------- tail + head of the next block in one launch
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("T", LENGTHS)
def test_cpu_tail_head_emulation_meets_bound(T, dt):
    """The fused form's statistics come from the fp32 block output the kernel holds: the emulation normalises the x it stores."""
    xo, _ = _emu_tail(_x_rows(T, 300), _ao_rows(T, dt), _tb_weights(dt, 2), dt)
    _tail_checks(f"emulation tail_head T={T} [{dt}]", dt, xo, None, _tail_expect(T, dt, True, 2, False))
    qk, vt = _emu_head(xo, _tb_weights(dt, 7), dt)
    _head_checks(f"emulation tail_head T={T} [{dt}]", dt, qk, vt, _head_expect(xo, _tb_weights(dt, 7), dt))


@gpu
@pytest.mark.parametrize("mt,cus", MTS, ids=MT_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("T", LENGTHS)
def test_tail_head(T, dt, mt, cus):
    """x bit-identical to cv_tblock_tail alone; [Q | K] and V^T against float64 from that stored x with the next block's weights."""
    x, ao, wd, wn = _x_rows(T, 300), _ao_rows(T, dt), _tb_dev(dt, 2), _tb_dev(dt, 7)
    o = _launch_tblock("tail_head", x, ao, wd, wn, dt, mt, cus)
    alone = _launch_tblock("tail", x, ao, wd, None, dt, mt, cus)
    assert torch.equal(H.bits(o["x"]), H.bits(alone["x"])), "x of cv_tblock_tail_head differs from cv_tblock_tail alone"
    who = f"tail_head T={T} mt={mt} cus={cus} [{dt}]"
    _tail_checks(who, dt, o["x"], None, _tail_expect(T, dt, True, 2, False))
    _head_checks(who, dt, o["qk"], o["vt"], _head_expect(o["x"], _tb_weights(dt, 7), dt))
    if mt:
        for r in range(R):
            _same(f"tail_head T={T} mt={mt}", o, _launch_tblock("tail_head", x[r:r + 1], ao[r:r + 1], wd, wn, dt, mt, cus), r)


# ----------------------------------------------------------------------------- causal resnet block
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cin,lda,T,sweep", [c for c in RES_CASES if c[1] != 512], ids=[i for i, c in zip(RES_IDS, RES_CASES) if c[1] != 512])
def test_cpu_resblock_emulation_meets_bound(cin, lda, T, sweep, dt):
    a, w = _a_rows(T, cin, dt), _rb_weights(dt, cin, sweep)
    h1 = _emu_res1(a, w, dt)
    H.check(f"emulation conv1 h1 cin={cin} T={T} [{dt}]", h1, *_res1_expect(T, cin, dt, sweep))
    H.check(f"emulation conv2 out cin={cin} T={T} [{dt}]", _emu_res2(h1, a, w), *_res2_expect(h1, a, w, cin))


@gpu
@pytest.mark.parametrize("mt,cus", MTS, ids=MT_IDS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cin,lda,T,sweep", RES_CASES, ids=RES_IDS)
def test_resblock(cin, lda, T, sweep, dt, mt, cus):
    a, w, wd = _a_rows(T, cin, dt), _rb_weights(dt, cin, sweep), _rb_dev(dt, cin, sweep)
    h1, out = _launch_resblock(a, wd, dt, cin, lda, mt, cus)
    who = f"cin={cin} lda={lda} T={T} mt={mt} cus={cus} [{dt}]"
    H.check(f"conv1 h1 {who}", h1, *_res1_expect(T, cin, dt, sweep))
    H.check(f"conv2 out {who}", out, *_res2_expect(h1, a, w, cin))
    if mt:
        for r in range(R):
            h1r, outr = _launch_resblock(a[r:r + 1], wd, dt, cin, lda, mt, cus)
            _same(f"resblock {who}", dict(h1=h1, out=out), dict(h1=h1r, out=outr), r)


# ----------------------------------------------------------------------------- across mt
def _all_equal(name, runs):
    same = all(torch.equal(H.bits(runs[0][k]), H.bits(o[k])) for o in runs[1:] for k in runs[0] if runs[0][k] is not None)
    print(f"{name}: mt = 1 .. 4 bit-identical: {same}")
    assert same, f"{name}: outputs depend on mt"


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("T", LENGTHS)
def test_tblock_identical_across_mt(T, dt):
    x, ao, wd, wn = _x_rows(T, 300), _ao_rows(T, dt), _tb_dev(dt, 2), _tb_dev(dt, 7)
    _all_equal(f"head T={T} [{dt}]", [_launch_tblock("head", x, None, wn, None, dt, mt, 0) for mt in (1, 2, 3, 4)])
    _all_equal(f"tail T={T} [{dt}]", [_launch_tblock("tail", x, ao, wd, None, dt, mt, 0, True) for mt in (1, 2, 3, 4)])
    _all_equal(f"tail (no ao) T={T} [{dt}]", [_launch_tblock("tail", x, None, wd, None, dt, mt, 0, True) for mt in (1, 2, 3, 4)])
    _all_equal(f"tail_head T={T} [{dt}]", [_launch_tblock("tail_head", x, ao, wd, wn, dt, mt, 0) for mt in (1, 2, 3, 4)])


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cin", [256, 320, 512])
@pytest.mark.parametrize("T", LENGTHS)
def test_resblock_identical_across_mt(T, cin, dt):
    a, wd = _a_rows(T, cin, dt), _rb_dev(dt, cin)
    runs = [_launch_resblock(a, wd, dt, cin, cin + 8, mt, 0) for mt in (1, 2, 3, 4)]
    _all_equal(f"resblock cin={cin} T={T} [{dt}]", [dict(h1=h, out=o) for h, o in runs])


# ----------------------------------------------------------------------------- the bounds have teeth
def _fault_ratio(fault, dt):
    if fault in ("clamp0", "prev_seq", "tadd_first"):
        a, w = _a_rows(5, 256, dt), _rb_weights(dt, 256)
        return H.worst_ratio(_emu_res1(a, w, dt, fault), *_res1_expect(5, 256, dt, False))
    if fault == "no_bo":
        xo, _ = _emu_tail(_x_rows(17, 300), _ao_rows(17, dt), _tb_weights(dt, 2), dt, fault)
        return H.worst_ratio(xo, *_tail_expect(17, dt, True, 2, False))
    T = {"no_eps": 16, "swap_tiles": 1, "vt_straddle": 5, "ln_tile_row": 66}[fault]
    qk, vt = _emu_head(_x_rows(T, 100), _tb_weights(dt, 0), dt, fault)
    ref, bound = _head_expect_cached(T, dt)
    if fault == "vt_straddle":
        return H.worst_ratio(vt, ref[..., 2 * INNER:].transpose(1, 2), bound[..., 2 * INNER:].transpose(1, 2))
    return H.worst_ratio(qk, ref[..., :2 * INNER], bound[..., :2 * INNER])


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("fault", ["clamp0", "prev_seq", "no_bo", "tadd_first", "no_eps", "swap_tiles", "vt_straddle", "ln_tile_row"])
def test_cpu_injected_fault_misses(fault, dt):
    """Each of the eight faults of the module docstring, injected into the emulation, misses a bound in the case named there; without the fault
    the same emulation meets it (test_cpu_*_emulation_meets_bound)."""
    ratio = _fault_ratio(fault, dt)
    print(f"fault {fault} [{dt}]: max err / bound {ratio:.3g}")
    assert ratio > 1.0, f"fault {fault} [{dt}] stays within the bound: max err / bound {ratio:.3f}"
