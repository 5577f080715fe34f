"""Op-level parity of cv_attention (csrc/attention.hip: the 16x16x32, 32x32x16 and 64-query forms, 2 and 4 waves) through the C ABI against
a float64 softmax(scale q k^T + bias) v computed on the CPU from the already rounded 16-bit operands, element-wise (tests/_helpers.py).

Guards and poison: ``out`` is NaN with ldo > H * 64 and extra rows per batch, everything outside [B][Tq][H * 64] must stay NaN; Q rows >= Tq,
K rows in [klen, Tk), the K / Q row slack, V^T columns >= klen up to vt_ld and bias entries at masked (i, j) or outside [0, Tk) hold NaN: the
ABI says none of them is read into a result.  Rows without a visible key must be exact zeros.

The bound (H.attn_bound).  With p the float64 softmax over the visible keys, A_id = sum_j p_ij |v_jd| and S_i = max_j (scale sum_d |q_id k_jd|
+ |bias_ij|):
    |out - ref| <= (u_P + c_s 2^-23 S_i + (Tk + 2 ceil(Tk / 64) + c) 2^-23) A_id + half an ulp of the output type (+ the fp16 term below)
  u_P = 2^-(MANT + 1): the one rounding of P to the operand type in front of the P V MFMA; the denominator is summed from the unrounded P.
  c_s = 136 = 2 x (64 + 4): a score is a 64-term fp32 MFMA sum of exact products, each partial sum rounded (rule 2: <= 64 x 2^-23 S_i in
      natural-log units), then scale * log2(e) (one constant rounding), bias * log2(e) (one), the FMA that joins them (one) and the
      subtraction of the running maximum (one): 4 more roundings of values <= S_i.  p_ij depends on s_ij - max_j s_ij, two scores, hence
      the factor 2; d exp(x) = exp(x) dx turns the absolute score error into a relative error of p.
  Tk + 2 ceil(Tk / 64): the fp32 accumulation of the numerator (MFMA, Tk terms of one sign pattern |p v|: <= Tk 2^-24 A) and of the denominator
      (Tk positive terms: Tk 2^-24), and per 64-key tile one rounding of each by the alpha rescale (the error of alpha itself is common to
      both and cancels in the quotient).
  c = 10: v_exp_f32 on the numerator's and on the denominator's P (1 ulp each: 2), the three-step cross-lane sum of l (1.5), 1 / l (<= 2.5 ulp
      as the compiler may expand it), the product with it (0.5), rounded up with the second-order terms.
  fp16: a probability below 2^-14 of the row maximum is subnormal in fp16; hardware may round it gradually or flush it.  The bound admits
      both by adding sub_id = sum_j [p_ij / max_j p_ij < 2^-14] p_ij |v_jd| (taken against the final maximum, a superset of what is subnormal
      against the running maximum at the time P is rounded).
Nothing here is fitted to the kernels.  ``test_cpu_attention_bound`` (no gpu mark) runs a plain torch emulation of the tiled arithmetic
(H.attn_emulate) on every GPU case: it meets the bound, and it misses it as soon as one mask is widened by one key, so the cases have teeth
and a miss on the device belongs to the kernel.

Dispatch (cv_attention): cv_attn_params.mfma 16 -> attn_kernel, 32 -> attn32_kernel, 64 -> attn64_kernel, which takes no bias: with a bias the
dispatcher falls through to the 16 form; cv_attn_params.waves 2 / 4 the workgroup shape of the 16 and 32 forms.  Every case runs all six."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

gpu = pytest.mark.gpu
DTS = [torch.bfloat16, torch.float16]
NAN = float("nan")


def _case(name, B, Hh, Hkv, Tq, Tk, klen=None, chunk=0, causal=False, coff=0, q_off=0, bias=False, layout="packed", data="randn", vt8=False,
          scale=0.125):
    return dict(name=name, B=B, H=Hh, Hkv=Hkv, Tq=Tq, Tk=Tk, klen=klen, chunk=chunk, causal=causal, coff=coff, q_off=q_off, bias=bias,
                layout=layout, data=data, vt8=vt8, scale=scale)


LENS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
CASES = [_case(f"len{T}", 2 if T < 1000 else 1, 2, 2, T, T, vt8=bool(n & 1)) for n, T in enumerate(LENS)]
CASES += [
    # Tq != Tk, both directions
    _case("tq33_tk257", 2, 2, 1, 33, 257, vt8=True), _case("tq257_tk33", 2, 2, 2, 257, 33), _case("tq1_tk129", 2, 4, 2, 1, 129),
    _case("tq129_tk1", 1, 2, 2, 129, 1, vt8=True),
    # per-batch klen: 0, 1, around the 64-key tile edge, Tk - 1, Tk, beyond Tk (clamped)
    _case("klen_mix_tk130", 8, 2, 2, 130, 130, klen=(0, 1, 63, 64, 65, 129, 130, 137), vt8=True),
    _case("klen_mix_tk257", 4, 2, 1, 257, 257, klen=(65, 256, 257, 264)),
    # causal offsets
    _case("causal_m5", 1, 2, 2, 150, 150, causal=True, coff=-5), _case("causal_0", 2, 2, 2, 150, 150, causal=True, vt8=True),
    _case("causal_p3", 1, 2, 2, 150, 150, causal=True, coff=3), _case("causal_tk", 1, 2, 2, 150, 150, causal=True, coff=150),
    _case("causal_tq77_tk300_off223", 1, 2, 2, 77, 300, causal=True, coff=223, vt8=True),
    # chunk masks; q_off puts a chunk boundary inside a wave's 32-query block and inside a 64-key tile
    _case("chunk1", 1, 2, 2, 70, 70, chunk=1), _case("chunk25_qoff10", 1, 2, 2, 120, 130, chunk=25, q_off=10, vt8=True),
    _case("chunk50_qoff223", 1, 2, 2, 77, 300, chunk=50, q_off=223), _case("chunk64_qoff40", 1, 2, 2, 100, 140, chunk=64, q_off=40),
    _case("chunk100", 1, 2, 2, 257, 257, chunk=100, vt8=True), _case("chunk_ge_tk", 1, 2, 2, 129, 129, chunk=512),
    # the production layouts with their stride arguments
    _case("prefill_gqa14_2_causal_klen", 3, 14, 2, 107, 107, klen=(107, 64, 1), causal=True, layout="prefill"),
    _case("prefill_gqa14_2_causal", 1, 14, 2, 282, 282, causal=True, layout="prefill"),
    _case("encoder_inc_chunk_klen_bias_qoff", 1, 2, 2, 77, 300, klen=(291,), chunk=50, q_off=223, bias=True, layout="encoder"),
    _case("encoder_inc_first_call", 1, 2, 2, 100, 100, chunk=50, bias=True, layout="encoder"),
    _case("v1step_tk1", 1, 4, 4, 1, 1, bias=True, layout="v1step"), _case("v1step_tk65", 1, 4, 4, 1, 65, bias=True, layout="v1step"),
    _case("v1step_tk200", 1, 4, 4, 1, 200, bias=True, layout="v1step"),
    _case("bias_causal_m5", 2, 2, 2, 100, 100, causal=True, coff=-5, bias=True),
    _case("bias_klen", 2, 2, 1, 65, 129, klen=(129, 70), bias=True, vt8=True),
    # peaked scores: the largest score of a row sits on its first masked key / on its last visible key
    _case("peak_masked_causal_1000", 1, 1, 1, 1000, 1000, causal=True, data="peak_masked"),
    _case("peak_visible_causal_1000", 1, 1, 1, 1000, 1000, causal=True, data="peak_visible"),
    _case("peak_masked_chunk50_qoff223", 1, 2, 2, 77, 300, chunk=50, q_off=223, data="peak_masked"),
    _case("peak_visible_chunk50_qoff223", 1, 2, 2, 77, 300, chunk=50, q_off=223, data="peak_visible"),
    _case("peak_masked_klen", 2, 2, 2, 257, 257, klen=(200, 65), data="peak_masked"),
    _case("peak_visible_klen", 2, 2, 2, 257, 257, klen=(200, 65), data="peak_visible"),
    _case("peak_masked_causal_gqa_klen", 2, 4, 2, 129, 129, klen=(129, 100), causal=True, data="peak_masked", layout="prefill"),
    # exponent range: |scores| up to about 40
    _case("big_scores", 1, 2, 2, 257, 257, data="big"), _case("big_scores_causal", 1, 2, 2, 257, 257, causal=True, data="big", vt8=True),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
NAMES = list(CASE_BY_NAME)


def _mask(c, klen_d=0, coff_d=0, chunk_d=0):
    klen = None if c["klen"] is None else [k + klen_d for k in c["klen"]]
    return H.attn_mask(c["B"], c["Tq"], c["Tk"], klen, c["chunk"] + (chunk_d if c["chunk"] else 0), c["causal"], c["coff"] + coff_d, c["q_off"])


@functools.lru_cache(maxsize=4)
def _data(name, dt):
    """Clean operands of a case on the CPU, rounded to ``dt``: q (B, H, Tq, 64), k / v (B, Hkv, Tk, 64), bias (B, H, Tq, Tk) fp32 or None, and
    the visibility mask.  No poison here: the GPU test poisons its device buffers, the CPU twin needs real keys behind the masks."""
    c = CASE_BY_NAME[name]
    B, Hh, Hkv, Tq, Tk = c["B"], c["H"], c["Hkv"], c["Tq"], c["Tk"]
    g = torch.Generator().manual_seed(NAMES.index(name) + 1)
    ok = _mask(c)
    q, k, v = torch.randn(B, Hh, Tq, 64, generator=g), torch.randn(B, Hkv, Tk, 64, generator=g), torch.randn(B, Hkv, Tk, 64, generator=g)
    if c["data"] == "big":
        q, k = q * 3, k * 3
    elif c["data"].startswith("peak"):
        # rotary-style: k_j = [cos(j th) | sin(j th)], q_i = 4 [cos(j* th) | sin(j* th)] + noise: q_i . k_j = 4 sum_m cos((j* - j) th_m), 128 at
        # j = j* (score 16) and a random sum of 32 cosines elsewhere; j* = the row's first masked key (a leak of one key takes the row over)
        # or its last visible key (an over-mask by one key loses it)
        th = torch.rand(32, generator=g, dtype=torch.float64) * 2.7 + 0.3
        jj = torch.arange(Tk, dtype=torch.float64)[:, None] * th
        k = torch.cat([jj.cos(), jj.sin()], -1).float()[None, None].expand(B, Hkv, Tk, 64).clone()
        nvis = ok.sum(-1)                                                       # every mask here is a prefix of the keys
        jstar = (nvis if c["data"] == "peak_masked" else nvis - 1).clamp(0, Tk - 1).double()          # (B, Tq)
        a = jstar[..., None] * th
        q = 4 * torch.cat([a.cos(), a.sin()], -1).float()[:, None] + 0.1 * q
    bias = torch.randn(B, Hh, Tq, Tk, generator=g) if c["bias"] else None
    return q.to(dt), k.to(dt), v.to(dt), bias, ok


@functools.lru_cache(maxsize=4)
def _reference(name, dt):
    c = CASE_BY_NAME[name]
    q, k, v, bias, ok = _data(name, dt)
    ref, A, S, sub = H.attn_ref64(q, k, v, c["scale"], ok, bias)
    return ref, H.attn_bound(ref, A, S, sub, c["Tk"], dt)


# ----------------------------------------------------------------------------- CPU twin
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", NAMES)
def test_cpu_attention_bound(name, dt):
    """The torch emulation of the tiled arithmetic meets the bound on every GPU case (fp16: with gradual underflow of P and with P flushed), and
    misses it when klen, causal_off or chunk is widened by one key (each tried wherever it changes the mask; the peak_visible cases, whose
    largest score sits on the last visible key, are narrowed by one key instead: that is the mistake they are built to see)."""
    c = CASE_BY_NAME[name]
    q, k, v, bias, ok = _data(name, dt)
    ref, bound = _reference(name, dt)
    H.check(f"emulated attention {name}", H.attn_emulate(q, k, v, c["scale"], ok, dt, bias), ref, bound)
    if dt == torch.float16:
        H.check(f"emulated attention {name}, P flushed", H.attn_emulate(q, k, v, c["scale"], ok, dt, bias, flush=True), ref, bound)
    step = -1 if c["data"] == "peak_visible" else 1          # peak on the last visible key: the case is built to see an OVER-mask by one key
    for what, wide in ((f"klen {step:+d}", dict(klen_d=step)), (f"causal_off {step:+d}", dict(coff_d=step)), (f"chunk {step:+d}", dict(chunk_d=step))):
        okw = _mask(c, **wide)
        if torch.equal(okw, ok):
            continue
        got = H.attn_emulate(q, k, v, c["scale"], okw, dt, bias).double()
        ratio = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"{name}: {what} -> max err/bound {ratio:.3g}")
        assert ratio > 1.0, f"{name}: {what} stays inside the bound (ratio {ratio:.3g}): the case cannot see a mask that is off by one key"


def test_cpu_every_mask_kind_is_widened_somewhere():
    hit = set()
    for c in CASES:
        ok = _mask(c)
        for what, wide in (("klen", dict(klen_d=1)), ("causal", dict(coff_d=1)), ("chunk", dict(chunk_d=1))):
            if not torch.equal(_mask(c, **wide), ok):
                hit.add(what)
    assert hit == {"klen", "causal", "chunk"}


# ----------------------------------------------------------------------------- device buffers per layout
def _r(x, m):
    return (x + m - 1) // m * m


def _launch(c, dt, q, k, v, bias, ok, mfma, waves):
    """Builds the poisoned / guarded device buffers of the case's layout, runs ops.attention (kernel variant ``mfma`` / ``waves``) and returns (out (B, H, Tq, 64) on the CPU, the
    whole guarded output buffer on the CPU as float, a bool tensor of the same shape marking what the op may write)."""
    from cosyvoice_amd import ops
    B, Hh, Hkv, Tq, Tk, lay = c["B"], c["H"], c["Hkv"], c["Tq"], c["Tk"], c["layout"]
    klen = [min(x, Tk) for x in c["klen"]] if c["klen"] is not None else [Tk] * B
    kw = dict(B=B, H=Hh, Hkv=Hkv, Tq=Tq, Tk=Tk, scale=c["scale"], chunk=c["chunk"], causal=c["causal"], causal_off=c["coff"], q_off=c["q_off"])
    if c["klen"] is not None:
        kw["klen"] = torch.tensor(c["klen"], dtype=torch.int32, device="cuda")
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    keep = []
    if lay == "packed":
        ldq, ldk, ldo = Hh * 64 + 8, Hkv * 64 + 16, Hh * 64 + 4
        vt_ld = _r(Tk, 8) if c["vt8"] else _r(Tk, 64)
        Q = H.nan_like((B, Tq + 2, ldq), dt)
        Q[:, :Tq, :Hh * 64] = qd.permute(0, 2, 1, 3).reshape(B, Tq, Hh * 64)
        K = H.nan_like((B, Tk, ldk), dt)
        for b in range(B):
            K[b, :klen[b], :Hkv * 64] = kd[b, :, :klen[b]].permute(1, 0, 2).reshape(klen[b], Hkv * 64)
        rows_o = Tq + 3
        kw.update(q_bs=(Tq + 2) * ldq, ldq=ldq, k_bs=Tk * ldk, ldk=ldk, vt_ld=vt_ld, o_bs=rows_o * ldo, ldo=ldo)
    elif lay == "prefill":      # llm.py prefill(): K = the row-major cache [B][Hkv][ctx_max][64], V^T [B][Hkv][64][ctx_max]
        ctx_max = _r(Tk, 64) + 64
        ldq = ldo = Hh * 64
        Q = H.nan_like((B * Tq + 2, ldq), dt)
        Q[:B * Tq] = qd.permute(0, 2, 1, 3).reshape(B * Tq, Hh * 64)
        K = H.nan_like((B, Hkv, ctx_max, 64), dt)
        for b in range(B):
            K[b, :, :klen[b]] = kd[b, :, :klen[b]]
        vt_ld, rows_o = ctx_max, Tq
        kw.update(q_bs=Tq * ldq, ldq=ldq, k_bs=Hkv * ctx_max * 64, k_hs=ctx_max * 64, ldk=64, vt_ld=vt_ld, o_bs=Tq * ldo, ldo=ldo)
    elif lay == "encoder":      # flow.py _layer_cached(): Q and K are column slices of one [cap][3 D] buffer, rows [s, n) are the queries
        assert B == 1 and Hh == Hkv and Tk == c["q_off"] + Tq
        D, s, n, cap = Hh * 64, c["q_off"], Tk, _r(Tk, 64) + 64
        qb = H.nan_like((cap, 3 * D), dt)
        qb[s:n, :D] = qd[0].permute(1, 0, 2).reshape(Tq, D)
        qb[:klen[0], 2 * D:] = kd[0, :, :klen[0]].permute(1, 0, 2).reshape(klen[0], D)
        Q, K = qb[s:], qb[:, 2 * D:]
        ldo, rows_o, vt_ld = D + 4, Tq + 3, _r(Tk, 8)
        kw.update(q_bs=0, ldq=3 * D, k_bs=0, ldk=3 * D, vt_ld=vt_ld, o_bs=0, ldo=ldo)
        ldb = _r(2 * n - 1, 4)          # the rel-shift view: bias[h][i][j] = bd[h][i][n - 1 - s - i + j]
        bd = H.nan_like((Hh, Tq, ldb), torch.float32)
        col = (n - 1 - s - torch.arange(Tq))[:, None] + torch.arange(Tk)[None, :]
        bvis = torch.where(ok[0], bias[0], torch.full((), NAN)).cuda()
        bd.scatter_(2, col.cuda()[None].expand(Hh, Tq, Tk), bvis)
        kw.update(bias=bd.view(-1)[n - 1 - s:], bias_bs=0, bias_hs=Tq * ldb, bias_ld=ldb - 1)
        keep.append(bd)
    else:                       # llm_v1.py decode step: one query against the cached rows, a bias row per head, Tk patched per step
        assert lay == "v1step" and B == 1 and Tq == 1 and Hh == Hkv
        D, max_len = Hh * 64, 256
        Q = H.nan_like((1, 2 * D), dt)          # [q + u | q + v]: the second half is not this op's
        Q[0, :D] = qd[0, :, 0].reshape(D)
        K = H.nan_like((max_len, D), dt)
        K[:Tk] = kd[0].permute(1, 0, 2).reshape(Tk, D)
        ldo, rows_o, vt_ld = D, 1 + 3, max_len
        kw.update(q_bs=2 * D, ldq=2 * D, k_bs=max_len * D, ldk=D, vt_ld=vt_ld, o_bs=D, ldo=ldo)
        bd = H.nan_like((Hh, max_len), torch.float32)
        bd[:, :Tk] = bias[0, :, 0].cuda()
        kw.update(bias=bd, bias_bs=0, bias_hs=max_len, bias_ld=max_len)
        keep.append(bd)
    if c["bias"] and lay in ("packed", "prefill"):
        ldbias = Tk + 3
        bd = H.nan_like((B, Hh, Tq, ldbias), torch.float32)
        bd[..., :Tk] = torch.where(ok[:, None], bias, torch.full((), NAN)).cuda()
        kw.update(bias=bd, bias_bs=Hh * Tq * ldbias, bias_hs=Tq * ldbias, bias_ld=ldbias)
        keep.append(bd)
    Vt = H.nan_like((B, Hkv, 64, vt_ld), dt)
    for b in range(B):
        Vt[b, :, :, :klen[b]] = vd[b, :, :klen[b]].transpose(1, 2)
    nb = 1 if kw["o_bs"] == 0 else B
    out = H.nan_like((nb * rows_o + (2 if lay == "prefill" else 0), kw["ldo"]), dt)
    ops.attention(Q, K, Vt, out, mfma=mfma, waves=waves, **kw)
    torch.cuda.synchronize()
    o = out.cpu().float()
    may = torch.zeros_like(o, dtype=torch.bool)
    res = torch.empty(B, Hh, Tq, 64)
    for b in range(nb):
        may[b * rows_o:b * rows_o + Tq, :Hh * 64] = True
        res[b] = o[b * rows_o:b * rows_o + Tq, :Hh * 64].reshape(Tq, Hh, 64).permute(1, 0, 2)
    return res, o, may


VARIANTS = [("16", "4"), ("16", "2"), ("32", "4"), ("32", "2"), ("64", "4"), ("64", "2")]


@gpu
@pytest.mark.parametrize("mfma,waves", VARIANTS, ids=[f"mfma{m}-waves{w}" for m, w in VARIANTS])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", NAMES)
def test_attention_op(name, dt, mfma, waves):
    c = CASE_BY_NAME[name]
    q, k, v, bias, ok = _data(name, dt)
    ref, bound = _reference(name, dt)
    res, o, may = _launch(c, dt, q, k, v, bias, ok, int(mfma), int(waves))
    assert bool(torch.isnan(o[~may]).all()), f"{name}: cv_attention wrote outside [B][Tq][H * 64]"
    H.check(f"attention {name} [{dt}] mfma {mfma} waves {waves}", res, ref, bound)
    dead = ~ok.any(-1)                                                      # (B, Tq): rows without a visible key
    if bool(dead.any()):
        z = res.permute(0, 2, 1, 3)[dead]
        assert bool((z == 0).all()), f"{name}: rows without a visible key must be exact zeros"


def test_cpu_cases_cover_the_issue_matrix():
    """The case list holds what the module promises: every tile-edge length, both Tq != Tk directions, the klen / causal_off / chunk values,
    rows without a visible key, and q_off putting a chunk boundary inside a 32-query block and inside a 64-key tile."""
    assert {c["Tq"] for c in CASES if c["Tq"] == c["Tk"]} >= set(LENS)
    assert any(c["Tq"] < c["Tk"] for c in CASES) and any(c["Tq"] > c["Tk"] for c in CASES)
    kl = {(x, c["Tk"]) for c in CASES if c["klen"] for x in c["klen"]}
    assert {0, 1, 63, 64, 65} <= {x for x, _ in kl} and any(x == t - 1 for x, t in kl) and any(x == t for x, t in kl) and any(x == t + 7 for x, t in kl)
    assert {c["coff"] for c in CASES if c["causal"]} >= {-5, 0, 3} and any(c["causal"] and c["coff"] == c["Tk"] for c in CASES)
    assert {c["chunk"] for c in CASES} >= {1, 25, 50, 64, 100} and any(c["chunk"] >= c["Tk"] for c in CASES)
    assert any(not bool(_mask(c).any(-1).all()) for c in CASES)
    c = CASE_BY_NAME["chunk50_qoff223"]
    edge_q = 250 - c["q_off"]                                               # first query of the chunk that starts at key 250
    assert edge_q % 32 != 0 and 250 % 64 != 0
    assert {c["layout"] for c in CASES} == {"packed", "prefill", "encoder", "v1step"}
